"""Plain-torch restatement of the reference's registration pieces (core/losses/metric_losses.py, utils/registration.py,
utils/geometry.py get_trans, metrics/registration_metrics.py, metrics/registration_tracker.py:123-145) that works in any
dtype: the tests evaluate it in fp32 and in float64 and hold it to tests/golden/registration.npz, which the reference's own
code produced.  Selections are explicit (the reference draws them with np.random.choice); everything is brute force."""
import math

import torch


def pdist(A, B, dist_type="L2"):
    D2 = torch.sum((A.unsqueeze(1) - B.unsqueeze(0)).pow(2), 2)
    return torch.sqrt(D2 + 1e-7) if dist_type == "L2" else D2


def allowed_pairs(pos_a, pos_b, min_dist):
    """pdist(pos_a, pos_b) > min_dist, evaluated in fp32 whatever the dtype of the pass (the masks of the fp32 and the
    float64 pass are the same pairs)"""
    return pdist(pos_a.float(), pos_b.float()) > min_dist


def feature_nn(a, b, pos_a=None, pos_b=None, min_dist=None):
    """(dist2 (P,), idx (P,), D2 (P, S) with +inf at the excluded pairs): the lowest index among exact ties, -1 / +inf for a
    row without a candidate"""
    D2 = pdist(a, b, "SquareL2")
    if pos_a is not None:
        D2 = torch.where(allowed_pairs(pos_a, pos_b, min_dist), D2, torch.full_like(D2, float("inf")))
    if D2.shape[1] == 0:
        return D2.new_full((len(a),), float("inf")), torch.full((len(a),), -1, dtype=torch.long, device=a.device), D2
    best = D2.min(1)[0]
    first = (D2 == best.unsqueeze(1)).to(torch.uint8).argmax(1)  # the first position of the minimum
    idx = torch.where(torch.isinf(best), torch.full_like(first, -1), first)
    return best, idx, D2


def nn_gap(D2):
    """per row: second smallest minus smallest entry of D2 (inf where fewer than two finite entries exist)"""
    if D2.shape[1] < 2:
        return D2.new_full((D2.shape[0],), float("inf"))
    two = torch.topk(D2, 2, dim=1, largest=False)[0]
    gap = two[:, 1] - two[:, 0]
    return torch.where(torch.isfinite(gap), gap, torch.full_like(gap, float("inf")))


def hardest_negative_parts(F0, F1, matches, sel0, sel1, pos_sel, pos_thresh, neg_thresh, num_pos):
    """every intermediate of ContrastiveHardestNegativeLoss.contrastive_hardest_negative_loss as a dict"""
    N0, N1 = len(F0), len(F1)
    hash_seed = max(N0, N1)
    sample = matches[pos_sel] if len(matches) > num_pos else matches
    pos_ind0, pos_ind1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[pos_ind0], F1[pos_ind1]
    D01 = pdist(posF0, F1[sel1])
    D10 = pdist(posF1, F0[sel0])
    D01min, D01ind = D01.min(1)
    D10min, D10ind = D10.min(1)
    D01ind, D10ind = sel1[D01ind], sel0[D10ind]
    pos_keys = matches[:, 0] + matches[:, 1] * hash_seed
    mask0 = ~torch.isin(pos_ind0 + D01ind * hash_seed, pos_keys)
    mask1 = ~torch.isin(D10ind + pos_ind1 * hash_seed, pos_keys)
    pos_arg = (posF0 - posF1).pow(2).sum(1) - pos_thresh
    neg_arg0 = neg_thresh - D01min[mask0]
    neg_arg1 = neg_thresh - D10min[mask1]
    pos_loss = torch.relu(pos_arg).mean()
    neg_loss = (torch.relu(neg_arg0).pow(2).mean() + torch.relu(neg_arg1).pow(2).mean()) / 2
    return {"loss": pos_loss + neg_loss, "relu_args": torch.cat([pos_arg, neg_arg0, neg_arg1]), "mask0": mask0, "mask1": mask1,
            "gap01": nn_gap(D01 ** 2 - 1e-7), "gap10": nn_gap(D10 ** 2 - 1e-7), "D01ind": D01ind, "D10ind": D10ind}


def hardest_negative_loss(F0, F1, matches, sel0, sel1, pos_sel, pos_thresh, neg_thresh, num_pos):
    return hardest_negative_parts(F0, F1, matches, sel0, sel1, pos_sel, pos_thresh, neg_thresh, num_pos)["loss"]


def batch_hard_parts(F0, F1, pairs, xyz0, pos_thresh, neg_thresh, min_dist):
    posF0, posF1 = F0[pairs[:, 0]], F1[pairs[:, 1]]
    sub = xyz0[pairs[:, 0]]
    closest, idx, D2 = feature_nn(posF0, posF1, sub, sub, min_dist)
    neg_arg = neg_thresh - closest
    neg_loss = (torch.relu(neg_arg).pow(2) / len(posF0)).sum()
    pos_arg = (posF0 - posF1).pow(2).max(1)[0] - pos_thresh
    pos_loss = torch.relu(pos_arg).pow(2).mean()
    return {"loss": pos_loss + neg_loss, "relu_args": torch.cat([pos_arg, neg_arg]), "gap": nn_gap(D2), "idx": idx}


def batch_hard_loss(F0, F1, pairs, xyz0, pos_thresh, neg_thresh, min_dist):
    return batch_hard_parts(F0, F1, pairs, xyz0, pos_thresh, neg_thresh, min_dist)["loss"]


def get_matches(feat_source, feat_target, sym=False):
    nearest = feature_nn(feat_source, feat_target)[1]
    rows = torch.arange(len(nearest), device=nearest.device)
    matches = torch.stack([rows, nearest], 1)
    if sym:
        back = feature_nn(feat_target, feat_source)[1]
        return matches[back[nearest] == rows]
    return matches


def estimate_transfo(xyz, xyz_target):
    xyz_c = xyz - xyz.mean(0)
    xyz_target_c = xyz_target - xyz_target.mean(0)
    Q = xyz_c.T.mm(xyz_target_c) / len(xyz)
    U, S, V = torch.svd(Q)
    diag = torch.ones(3, dtype=xyz.dtype, device=xyz.device)
    diag[2] = torch.det(V.mm(U.T))
    R = V.mm(torch.diag(diag)).mm(U.T)
    T = torch.eye(4, dtype=xyz.dtype, device=xyz.device)
    T[:3, :3] = R
    T[:3, 3] = xyz_target.mean(0) - R @ xyz.mean(0)
    return T


def get_trans(x):
    T = torch.eye(4, dtype=x.dtype, device=x.device)
    T[:3, 3] = x[3:]
    axis = x[:3]
    theta = torch.norm(axis)
    if theta > 0:
        axis = axis / theta
    K = torch.zeros(3, 3, dtype=x.dtype, device=x.device)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    T[:3, :3] = torch.eye(3, dtype=x.dtype, device=x.device) + torch.sin(theta) * K + (1 - torch.cos(theta)) * K.mm(K)
    return T


def get_matrix_system(xyz, xyz_target, weight):
    w = weight.view(-1)
    z = torch.zeros_like(w)
    A_x = torch.stack([z, w * xyz[:, 2], -w * xyz[:, 1], w, z, z], 1)
    A_y = torch.stack([-w * xyz[:, 2], z, w * xyz[:, 0], z, w, z], 1)
    A_z = torch.stack([w * xyz[:, 1], -w * xyz[:, 0], z, z, z, w], 1)
    b = torch.cat([w * (xyz_target[:, k] - xyz[:, k]) for k in range(3)], 0)
    return torch.cat([A_x, A_y, A_z], 0), b.view(-1, 1)


def fast_global_registration(xyz, xyz_target, mu_init=1.0, num_iter=20):
    T_res = torch.eye(4, dtype=xyz.dtype, device=xyz.device)
    mu = mu_init
    source = xyz.clone()
    weight = torch.ones(len(source), 1, dtype=xyz.dtype, device=xyz.device)
    for i in range(num_iter):
        if i > 0 and i % 5 == 0:
            mu /= 2.0
        A, b = get_matrix_system(source, xyz_target, weight)
        x = torch.linalg.solve(A.T.mm(A), A.T @ b)
        T = get_trans(x.view(-1))
        source = source.mm(T[:3, :3].T) + T[:3, 3]
        T_res = T @ T_res
        weight = (mu / (mu + torch.norm(xyz_target - source, dim=1) ** 2)).view(-1, 1)
    return T_res


def compute_hit_ratio(xyz, xyz_target, T_gt, tau_1):
    dist = torch.norm(xyz.mm(T_gt[:3, :3].T) + T_gt[:3, 3] - xyz_target, dim=1)
    return torch.mean((dist < tau_1).to(torch.float))  # (fp32 in every pass, as the reference)


def compute_transfo_error(T_gt, T_pred):
    rte = torch.norm(T_gt[:3, 3] - T_pred[:3, 3])
    cos_theta = torch.clamp((torch.trace(T_gt[:3, :3].mm(T_pred[:3, :3].T)) - 1) * 0.5, -1.0, 1.0)
    return rte, torch.acos(cos_theta) * 180 / math.pi


def compute_scaled_registration_error(xyz, T_gt, T_est, tol=1e-12):
    xyz_est = xyz @ T_est[:3, :3].T + T_est[:3, 3]
    xyz_gt = xyz @ T_gt[:3, :3].T + T_gt[:3, 3]
    dist1 = torch.sqrt(torch.sum((xyz_est - xyz_gt) ** 2, -1))
    dist2 = torch.sqrt(torch.sum((xyz_est - xyz_est.mean(0)) ** 2, -1))
    return torch.mean(dist1 / (dist2 + tol))


def compute_registration_recall(xyz_gt, xyz_target_gt, T_est, thresh=0.2):
    dist = torch.norm(xyz_gt @ T_est[:3, :3].T + T_est[:3, 3] - xyz_target_gt, dim=1)
    return bool(dist.mean() < thresh)


def evaluate_pair(feat, feat_target, xyz, xyz_target, matches_gt, rand, rand_target, tau_1=0.1, tau_2=0.05):
    """registration_tracker.py:123-145 for one pair, the drawn rows given"""
    T_gt = estimate_transfo(xyz[matches_gt[:, 0]], xyz_target[matches_gt[:, 1]])
    matches_pred = get_matches(feat[rand], feat_target[rand_target])
    src, tgt = xyz[rand][matches_pred[:, 0]], xyz_target[rand_target][matches_pred[:, 1]]
    T_pred = fast_global_registration(src, tgt)
    hit_ratio = compute_hit_ratio(src, tgt, T_gt, tau_1)
    trans_error, rot_error = compute_transfo_error(T_pred, T_gt)
    sr_err = compute_scaled_registration_error(xyz, T_gt, T_pred)
    return {"hit_ratio": hit_ratio, "feat_match_ratio": (hit_ratio > tau_2).to(torch.float), "trans_error": trans_error,
            "rot_error": rot_error, "sr_err": sr_err}


def rotation(axis, angle, dtype=torch.float64):
    """Rodrigues matrix of a (not necessarily unit) axis and an angle"""
    x = torch.as_tensor(axis, dtype=dtype)
    x = x / x.norm() * angle
    return get_trans(torch.cat([x, torch.zeros(3, dtype=dtype)]))[:3, :3]
