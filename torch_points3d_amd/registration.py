"""Registration descriptors (reference torch_points3d/models/registration/{base,kpconv,spconv3d}.py,
core/losses/metric_losses.py, utils/registration.py, metrics/registration_metrics.py, metrics/registration_tracker.py) on the
device: fragment descriptors trained with a mined contrastive loss, evaluated by feature matching and a robust pose solve.

  pdist                            the reference's broadcast form (small inputs, tests and baselines)
  ContrastiveHardestNegativeLoss   the argmin from torchpoints.feature_nn, the mined distance recomputed differentiably from
                                   torchpoints.gather_rows: the (P, S, C) tensor never exists; pair keys, `isin` and the masked
                                   means stay on the device (nothing is read back inside the training step)
  BatchHardContrastiveLoss         the per-pair Python loop as one feature_nn call with the spatial exclusion
  get_matches, estimate_transfo, fast_global_registration   utils/registration.py (1-NN by feature_nn, FGR by torchpoints.fgr)
  compute_hit_ratio, compute_transfo_error, compute_scaled_registration_error, compute_registration_recall
  ransac_registration              utils/registration.py:141-163 through torchpoints.ransac_pose (HIP hypothesis scoring, integer
                                   select, Kabsch refit over the inliers; nothing read back); CPU tensors: numpy float64
  evaluate_pair                    the tracker's sequence for one fragment pair (registration_tracker.py:123-145)
  compute_metrics                  the benchmark script's figures for one pair (scripts/test_registration_scripts/evaluate.py:
                                   46-142), with the RANSAC block the script left unimplemented
  FragmentDescriptor               backbone -> FC_layer head (FragmentKPConv's layout) -> unit rows; "match" mode loss

MS-SVConv lives in ms_svconv.py.  Not served: TEASER++, the Minkowski and patch models, and compute_loss_label's
pytorch_metric_learning miners.
"""
import math

import numpy as np
import torch
from torch import nn

from . import torchpoints as tp
from .kpconv_blocks import FastBatchNorm1d


def pdist(A, B, dist_type="L2"):
    """metric_losses.py:22-29: the (len(A), len(B)) distances from the broadcast difference"""
    D2 = torch.sum((A.unsqueeze(1) - B.unsqueeze(0)).pow(2), 2)
    if dist_type == "L2":
        return torch.sqrt(D2 + 1e-7)
    if dist_type == "SquareL2":
        return D2
    raise NotImplementedError("Not implemented")


def _draw(n, k, device, generator):
    """k of n rows without replacement, on the device"""
    return torch.randperm(n, device=device, generator=generator)[:k]


def _masked_mean(values, mask):
    """values[mask].mean() without the boolean index (no device read): NaN for an empty mask, like the mean of nothing"""
    zero = torch.zeros((), dtype=values.dtype, device=values.device)
    return torch.where(mask, values, zero).sum() / mask.sum().to(values.dtype)


def _isin(keys, sorted_table):
    """np.isin(keys, table) for int64 keys against an ascending table, by binary search (torch.isin removes duplicates first
    and reads their number back)"""
    if sorted_table.numel() == 0:
        return torch.zeros_like(keys, dtype=torch.bool)
    at = torch.searchsorted(sorted_table, keys).clamp(max=sorted_table.numel() - 1)
    return sorted_table[at] == keys


class ContrastiveHardestNegativeLoss(nn.Module):
    """metric_losses.py:32-119 (after FCGF): pos_loss = relu(|f0 - f1|^2 - pos_thresh).mean() over the sampled positive
    pairs; for every sampled pair the nearest of `num_hn_samples` drawn rows of the other fragment is mined on each side,
    neg = relu(neg_thresh - sqrt(d^2 + 1e-7))^2 averaged over the rows whose mined pair is not one of the positive pairs;
    loss = pos_loss + (neg0 + neg1) / 2.

    forward(F0, F1, matches, xyz0=None, xyz1=None, *, sel0=None, sel1=None, pos_sel=None): F0 (N0, C), F1 (N1, C), matches
    (M, 2) rows of (F0, F1).  sel0 / sel1: the mined rows of F0 / F1, pos_sel: the sampled positive pairs (used when
    M > num_pos, as in the reference); by default drawn with torch.randperm on the device (`generator` of the constructor),
    where the reference draws np.random.choice on the host.  If every mined pair is a positive pair the mean over nothing is
    NaN, as in the reference."""

    def __init__(self, pos_thresh, neg_thresh, num_pos=5192, num_hn_samples=2048, generator=None):
        super().__init__()
        self.pos_thresh = pos_thresh
        self.neg_thresh = neg_thresh
        self.num_pos = num_pos
        self.num_hn_samples = num_hn_samples
        self.generator = generator

    def contrastive_hardest_negative_loss(self, F0, F1, positive_pairs, sel0=None, sel1=None, pos_sel=None):
        dev = F0.device
        N0, N1 = len(F0), len(F1)
        positive_pairs = positive_pairs.to(dev).long()
        hash_seed = max(N0, N1)
        sel0 = _draw(N0, min(N0, self.num_hn_samples), dev, self.generator) if sel0 is None else sel0.to(dev).long()
        sel1 = _draw(N1, min(N1, self.num_hn_samples), dev, self.generator) if sel1 is None else sel1.to(dev).long()
        sample_pos_pairs = positive_pairs
        if len(positive_pairs) > self.num_pos:
            if pos_sel is None:
                pos_sel = _draw(len(positive_pairs), self.num_pos, dev, self.generator)
            sample_pos_pairs = positive_pairs[pos_sel.to(dev).long()]
        pos_ind0, pos_ind1 = sample_pos_pairs[:, 0], sample_pos_pairs[:, 1]
        posF0, posF1 = tp.gather_rows(F0, pos_ind0), tp.gather_rows(F1, pos_ind1)

        # the hardest negative of every positive row among the drawn rows of the other side: indices only
        F0d, F1d = F0.detach(), F1.detach()
        D01ind = sel1[tp.feature_nn(posF0, F1d[sel1])[1]]
        D10ind = sel0[tp.feature_nn(posF1, F0d[sel0])[1]]
        # ... and its distance again, differentiably, from the two gathered rows
        D01min = torch.sqrt((posF0 - tp.gather_rows(F1, D01ind)).pow(2).sum(1) + 1e-7)
        D10min = torch.sqrt((posF1 - tp.gather_rows(F0, D10ind)).pow(2).sum(1) + 1e-7)

        pos_keys = torch.sort(positive_pairs[:, 0] + positive_pairs[:, 1] * hash_seed)[0]
        mask0 = torch.logical_not(_isin(pos_ind0 + D01ind * hash_seed, pos_keys))
        mask1 = torch.logical_not(_isin(D10ind + pos_ind1 * hash_seed, pos_keys))
        pos_loss = torch.relu((posF0 - posF1).pow(2).sum(1) - self.pos_thresh)
        neg_loss0 = _masked_mean(torch.relu(self.neg_thresh - D01min).pow(2), mask0)
        neg_loss1 = _masked_mean(torch.relu(self.neg_thresh - D10min).pow(2), mask1)
        return pos_loss.mean(), (neg_loss0 + neg_loss1) / 2

    def forward(self, F0, F1, matches, xyz0=None, xyz1=None, *, sel0=None, sel1=None, pos_sel=None):
        pos_loss, neg_loss = self.contrastive_hardest_negative_loss(F0, F1, matches, sel0, sel1, pos_sel)
        return pos_loss + neg_loss


class BatchHardContrastiveLoss(nn.Module):
    """metric_losses.py:122-162, its arithmetic kept: the positive term is relu(max over the CHANNELS of (f0 - f1)^2 -
    pos_thresh)^2, averaged; the negative of pair i is the nearest posF1 row (squared distance, no root) among the pairs
    whose F0 point lies further than min_dist from pair i's, relu(neg_thresh - d2)^2 / len(pairs), summed.  The reference's
    loop over the pairs is one feature_nn call with the spatial exclusion.  A pair with no allowed negative contributes 0
    (the reference raises on the minimum of nothing)."""

    def __init__(self, pos_thresh, neg_thresh, min_dist=0.15):
        super().__init__()
        self.pos_thresh = pos_thresh
        self.neg_thresh = neg_thresh
        self.min_dist = min_dist

    def forward(self, F0, F1, positive_pairs, xyz0=None, xyz1=None):
        if xyz0 is None:
            raise ValueError("BatchHardContrastiveLoss needs xyz0 (the positions of F0's rows)")
        positive_pairs = positive_pairs.to(F0.device).long()
        posF0 = tp.gather_rows(F0, positive_pairs[:, 0])
        posF1 = tp.gather_rows(F1, positive_pairs[:, 1])
        subxyz0 = xyz0[positive_pairs[:, 0]]
        hardest = tp.feature_nn(posF0, posF1, subxyz0, subxyz0, self.min_dist)[1]
        found = hardest >= 0
        closest_neg = (posF0 - tp.gather_rows(posF1, hardest.clamp(min=0))).pow(2).sum(1)
        neg_terms = torch.relu(self.neg_thresh - closest_neg).pow(2) / len(posF0)
        neg_loss = torch.where(found, neg_terms, torch.zeros_like(neg_terms)).sum()
        furthest_pos = (posF0 - posF1).pow(2).max(1)[0]
        pos_loss = torch.relu(furthest_pos - self.pos_thresh).pow(2)
        return pos_loss.mean() + neg_loss


# ------------------------------------------------------------------------------------------------ matching and pose solve
def get_matches(feat_source, feat_target, sym=False):
    """(M, 2) int64: every source row with its nearest target row in feature space (utils/registration.py:13-21, whose
    torch_geometric knn is feature_nn here); sym=True keeps the mutual nearest neighbours only."""
    nearest = tp.feature_nn(feat_source, feat_target)[1]
    rows = torch.arange(len(nearest), device=nearest.device)
    matches = torch.stack([rows, nearest], 1)
    if sym:
        back = tp.feature_nn(feat_target, feat_source)[1]
        return matches[back[nearest] == rows]
    return matches


def _feature_nearest(a, b):
    """for every row of a the row of b nearest in feature space: feature_nn on the device, a float64 argmin (the lowest
    index among equal distances) for CPU tensors"""
    if a.device.type != "cpu":
        return tp.feature_nn(a, b)[1]
    A, B = a.detach().double(), b.detach().double()
    return torch.cat([((A[r0:r0 + 1024, None, :] - B[None]) ** 2).sum(-1).argmin(1) for r0 in range(0, len(A), 1024)])


def compute_matches(feature_source, feature_target, kp_source, kp_target, sym=False):
    """descriptor_matcher.py:40-59 of the reference's test_registration_scripts: every target keypoint with the source
    keypoint nearest in feature space; sym=True keeps the mutual nearest neighbours only.  Returns (new_kp_source,
    new_kp_target), row-aligned (M, 3), on the inputs' device (the script's KDTree queries are feature_nn here; its
    unused `ratio` argument is dropped)."""
    near_t = _feature_nearest(feature_target, feature_source)  # target row -> source row
    keep = torch.arange(len(near_t), device=near_t.device)
    if sym:
        near_s = _feature_nearest(feature_source, feature_target)
        keep = keep[near_s[near_t] == keep]
    return kp_source[near_t[keep]], kp_target[keep]


def compute_dists(kp_source, kp_target, trans):
    """descriptor_matcher.py:62-68: |kp_source - (R kp_target + t)| per matched pair under the (4, 4) pose `trans`"""
    trans = torch.as_tensor(trans, dtype=kp_target.dtype, device=kp_target.device)
    return torch.linalg.norm(kp_source - (kp_target @ trans[:3, :3].T + trans[:3, 3]), dim=1)


def compute_mean_correct_matches(dist, list_tau, is_leq=True):
    """descriptor_matcher.py:71-81: for every tau the share of entries below it (is_leq) or above it, over axis 0 of
    dist; a (len(list_tau), ...) tensor on dist's device"""
    dist = torch.as_tensor(dist)
    return torch.stack([((dist < tau) if is_leq else (dist > tau)).to(torch.float64).mean(0) for tau in list_tau])


def feature_match_recall(pairs, list_tau1=(0.1,), list_tau2=(0.05,)):
    """The feature-match recall of descriptor_matcher.py:121-142 over a list of pairs (feat_s, feat_t, kp_s, kp_t, T_gt):
    per pair the share of matches closer than tau_1 under T_gt, then for every tau_2 the share of pairs whose share
    exceeds it.  Returns (recall (len(list_tau2), len(list_tau1)), frac_correct (pairs, len(list_tau1))), float64 on the
    inputs' device; nothing is read back."""
    frac = torch.stack([compute_mean_correct_matches(compute_dists(*compute_matches(fs, ft, ks, kt), T), list_tau1)
                        for fs, ft, ks, kt, T in pairs])
    return compute_mean_correct_matches(frac, list_tau2, is_leq=False), frac


def estimate_transfo(xyz, xyz_target):
    """Kabsch (utils/registration.py:24-43): the (4, 4) pose that maps xyz onto xyz_target in the least-squares sense"""
    assert xyz.shape == xyz_target.shape
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


def fast_global_registration(xyz, xyz_target, mu_init=1, num_iter=20):
    """utils/registration.py:83-103 through torchpoints.fgr (two launches per iteration, no (3N, 6) matrix, no host read)"""
    assert xyz.shape == xyz_target.shape
    return tp.fgr(xyz, xyz_target, mu_init=float(mu_init), num_iter=num_iter)


def _horn_numpy(p, q, w=None):
    """(..., 3, 4) float64 [R | t]: the weighted least-squares rigid pose of p (..., n, 3) onto q by Horn's closed form, the
    unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix of the centred cross-covariance (what
    csrc/ransac_horn.h does with Jacobi sweeps, here numpy's eigh)"""
    w = np.ones(p.shape[:-1]) if w is None else w
    wsum = w.sum(-1)[..., None]
    mp, mq = (w[..., None] * p).sum(-2) / wsum, (w[..., None] * q).sum(-2) / wsum
    S = np.einsum("...n,...na,...nb->...ab", w, p - mp[..., None, :], q - mq[..., None, :])
    A = np.empty(S.shape[:-2] + (4, 4))
    A[..., 0, 0] = S[..., 0, 0] + S[..., 1, 1] + S[..., 2, 2]
    A[..., 1, 1] = S[..., 0, 0] - S[..., 1, 1] - S[..., 2, 2]
    A[..., 2, 2] = S[..., 1, 1] - S[..., 0, 0] - S[..., 2, 2]
    A[..., 3, 3] = S[..., 2, 2] - S[..., 0, 0] - S[..., 1, 1]
    A[..., 0, 1] = A[..., 1, 0] = S[..., 1, 2] - S[..., 2, 1]
    A[..., 0, 2] = A[..., 2, 0] = S[..., 2, 0] - S[..., 0, 2]
    A[..., 0, 3] = A[..., 3, 0] = S[..., 0, 1] - S[..., 1, 0]
    A[..., 1, 2] = A[..., 2, 1] = S[..., 0, 1] + S[..., 1, 0]
    A[..., 1, 3] = A[..., 3, 1] = S[..., 2, 0] + S[..., 0, 2]
    A[..., 2, 3] = A[..., 3, 2] = S[..., 1, 2] + S[..., 2, 1]
    qw, qx, qy, qz = np.moveaxis(np.linalg.eigh(A)[1][..., :, 3], -1, 0)  # (eigh: ascending eigenvalues, unit vectors)
    R = np.stack([np.stack([qw * qw + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)], -1),
                  np.stack([2 * (qx * qy + qw * qz), qw * qw - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - qw * qx)], -1),
                  np.stack([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz], -1)], -2)
    t = mq - np.einsum("...ab,...b->...a", R, mp)
    return np.concatenate([R, t[..., None]], -1)


def _ransac_numpy(xyz, xyz_target, threshold, samples, refine=1):
    """the algorithm of torchpoints.ransac_pose in numpy float64, for CPU tensors: (pose (3, 4), best index, counts (H,))"""
    p, q = xyz.astype(np.float64), xyz_target.astype(np.float64)
    H, N = len(samples), len(p)
    poses = _horn_numpy(p[samples], q[samples])
    counts = np.zeros(H, dtype=np.int64)
    step = max(1, (1 << 21) // N)  # (the (step, N, 3) residuals stay within a few tens of MB)
    for h0 in range(0, H, step):
        P = poses[h0:h0 + step]
        d = np.einsum("hab,nb->hna", P[:, :, :3], p) + P[:, None, :, 3] - q
        hit = (d * d).sum(-1) < threshold * threshold
        counts[h0:h0 + step] = np.where(np.isfinite(P).all((1, 2)), hit.sum(1), 0)
    best = int(np.argmax(counts))  # the first of equal counts
    pose = poses[best] if np.isfinite(poses[best]).all() else np.eye(4)[:3]
    for _ in range(refine):
        d = p @ pose[:, :3].T + pose[:, 3] - q
        inl = (d * d).sum(1) < threshold * threshold
        if inl.sum() >= 3:
            fresh = _horn_numpy(p[inl], q[inl])
            pose = fresh if np.isfinite(fresh).all() else pose
    return pose, best, counts


def ransac_registration(xyz, xyz_target, distance_threshold=0.05, num_iterations=80000, *, generator=None, samples=None):
    """utils/registration.py:141-163 (open3d's registration_ransac_based_on_correspondence with ransac_n = 4 and point-to-
    point estimation) for the correspondences xyz[i] <-> xyz_target[i]: `num_iterations` hypotheses from 4 correspondences
    drawn with replacement (samples (H, 4) int64; default torch.randint on the inputs' device with `generator`), each
    scored by its number of correspondences within distance_threshold, the best refitted once by Kabsch over its inliers.
    Device tensors go through torchpoints.ransac_pose (HIP, nothing read back), CPU tensors through a numpy float64
    restatement of the same algorithm.  Returns the (4, 4) float pose ON THE INPUTS' DEVICE (the reference returns a CPU
    tensor).  Differences from open3d: every hypothesis is scored (no early exit on a confidence bound, no edge-length
    or distance checkers), and among hypotheses with equal inlier counts the lowest index wins, an integer rule (open3d
    compares their inlier RMSE)."""
    assert xyz.shape == xyz_target.shape
    if xyz.device.type != "cpu":
        return tp.ransac_pose(xyz, xyz_target, float(distance_threshold), num_iterations=num_iterations, ransac_n=4, refine=1,
                              samples=samples, generator=generator)[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or len(xyz) < 3:
        raise ValueError("ransac_registration: xyz and xyz_target must both be (N, 3) with N >= 3")
    if samples is None:
        if num_iterations < 1:
            raise ValueError("ransac_registration: at least one hypothesis is needed")
        samples = torch.randint(0, len(xyz), (int(num_iterations), 4), generator=generator)
    if samples.dim() != 2 or not 3 <= samples.shape[1] <= tp.RANSAC_MAX_N or len(samples) < 1:
        raise ValueError("ransac_registration: samples must be (H, n) with H >= 1 and 3 <= n <= %d" % tp.RANSAC_MAX_N)
    pose = _ransac_numpy(xyz.detach().numpy(), xyz_target.detach().numpy(), float(distance_threshold), samples.long().numpy())[0]
    T = torch.eye(4)
    T[:3] = torch.from_numpy(pose).float()
    return T


# ------------------------------------------------------------------------------------------------------------------ metrics
def compute_hit_ratio(xyz, xyz_target, T_gt, tau_1):
    """the share of correspondences closer than tau_1 under T_gt (registration_metrics.py:30-37)"""
    assert xyz.shape == xyz_target.shape
    dist = torch.norm(xyz.mm(T_gt[:3, :3].T) + T_gt[:3, 3] - xyz_target, dim=1)
    return torch.mean((dist < tau_1).to(torch.float))


def compute_transfo_error(T_gt, T_pred):
    """(translation error, rotation error in degrees) (registration_metrics.py:40-50)"""
    rte = torch.norm(T_gt[:3, 3] - T_pred[:3, 3])
    cos_theta = (torch.trace(T_gt[:3, :3].mm(T_pred[:3, :3].T)) - 1) * 0.5
    cos_theta = torch.clamp(cos_theta, -1.0, 1.0)
    rre = torch.acos(cos_theta) * 180 / math.pi
    return rte, rre


def compute_scaled_registration_error(xyz, T_gt, T_est, tol=1e-12):
    """registration_metrics.py:53-66 (https://arxiv.org/pdf/2003.12841.pdf)"""
    xyz_est = xyz @ T_est[:3, :3].T + T_est[:3, 3]
    xyz_gt = xyz @ T_gt[:3, :3].T + T_gt[:3, 3]
    centroid = xyz_est.mean(0)
    dist1 = torch.sqrt(torch.sum((xyz_est - xyz_gt) ** 2, -1))
    dist2 = torch.sqrt(torch.sum((xyz_est - centroid) ** 2, -1))
    return torch.mean(dist1 / (dist2 + tol))


def compute_registration_recall(xyz_gt, xyz_target_gt, T_est, thresh=0.2):
    """registration_metrics.py:69-76: whether the mean distance of the true correspondences under T_est is below thresh.
    A boolean scalar on the inputs' device (the reference reads it back with .item())."""
    dist = torch.norm(xyz_gt @ T_est[:3, :3].T + T_est[:3, 3] - xyz_target_gt, dim=1)
    return dist.mean() < thresh


def evaluate_pair(feat, feat_target, xyz, xyz_target, matches_gt, num_points=5000, tau_1=0.1, tau_2=0.05, rand=None,
                  rand_target=None):
    """What FragmentRegistrationTracker.track does for one fragment pair (registration_tracker.py:123-145): the pose of the
    true matches by Kabsch, 1-NN feature matches between `num_points` drawn rows of each side (rand / rand_target: the
    drawn rows, default torch.randperm on the device), FGR on the matched positions, and the tracker's figures as a dict of
    device scalars: hit_ratio, feat_match_ratio (hit_ratio > tau_2), trans_error, rot_error, sr_err."""
    dev = feat.device
    if rand is None:
        rand = torch.randperm(len(feat), device=dev)[:num_points]
    if rand_target is None:
        rand_target = torch.randperm(len(feat_target), device=dev)[:num_points]
    matches_gt = matches_gt.to(dev).long()
    T_gt = estimate_transfo(xyz[matches_gt[:, 0]], xyz_target[matches_gt[:, 1]])
    matches_pred = get_matches(feat[rand], feat_target[rand_target])
    src = xyz[rand][matches_pred[:, 0]]
    tgt = xyz_target[rand_target][matches_pred[:, 1]]
    T_pred = fast_global_registration(src, tgt)
    hit_ratio = compute_hit_ratio(src, tgt, T_gt, tau_1)
    trans_error, rot_error = compute_transfo_error(T_pred, T_gt)
    sr_err = compute_scaled_registration_error(xyz, T_gt, T_pred)
    return {"hit_ratio": hit_ratio, "feat_match_ratio": (hit_ratio > tau_2).to(torch.float), "trans_error": trans_error,
            "rot_error": rot_error, "sr_err": sr_err}


def _pose_figures(res, tag, xyz, T_gt, T_est, rot_thresh, trans_thresh, xyz_gt, xyz_target_gt, recall_thresh):
    trans_error, rot_error = compute_transfo_error(T_est, T_gt)
    res["trans_error_" + tag] = trans_error
    res["rot_error_" + tag] = rot_error
    res["rre_" + tag] = (rot_error < rot_thresh).to(torch.float)
    res["rte_" + tag] = (trans_error < trans_thresh).to(torch.float)
    res["sr_" + tag] = compute_scaled_registration_error(xyz, T_gt, T_est)
    if xyz_gt is not None and xyz_target_gt is not None:
        res["registration_recall_" + tag] = compute_registration_recall(xyz_gt, xyz_target_gt, T_est, recall_thresh)


def compute_metrics(xyz, xyz_target, feat, feat_target, T_gt, sym=False, tau_1=0.1, tau_2=0.05, rot_thresh=5, trans_thresh=5,
                    use_ransac=False, ransac_thresh=0.02, registration_recall_thresh=0.2, xyz_gt=None, xyz_target_gt=None, *,
                    ransac_iterations=80000, generator=None, samples=None):
    """The figures of scripts/test_registration_scripts/evaluate.py:46-142 for one fragment pair, as a dict of scalars on
    the inputs' device (the script reads every one back with .item(); its time_* entries are not kept): 1-NN feature
    matches (mutual ones with sym), hit_ratio under T_gt at tau_1, feat_match_ratio = hit_ratio > tau_2, and for the
    FGR pose of the matched positions trans_error_fgr, rot_error_fgr, rre_fgr = rot_error < rot_thresh, rte_fgr =
    trans_error < trans_thresh, sr_fgr, and registration_recall_fgr when xyz_gt and xyz_target_gt are given.
    use_ransac=True adds the same entries with the suffix _ransac for ransac_registration(..., ransac_thresh), the block
    the script ends in NotImplementedError (ransac_iterations, generator, samples: its hypotheses).  TEASER++ is not
    served: there is no use_teaser."""
    res = dict()
    matches_pred = get_matches(feat, feat_target, sym=sym)
    src, tgt = xyz[matches_pred[:, 0]], xyz_target[matches_pred[:, 1]]
    hit_ratio = compute_hit_ratio(src, tgt, T_gt, tau_1)
    res["hit_ratio"] = hit_ratio
    res["feat_match_ratio"] = (hit_ratio > tau_2).to(torch.float)
    T_fgr = fast_global_registration(src, tgt)
    _pose_figures(res, "fgr", xyz, T_gt, T_fgr, rot_thresh, trans_thresh, xyz_gt, xyz_target_gt, registration_recall_thresh)
    if use_ransac:
        T_ransac = ransac_registration(src, tgt, ransac_thresh, ransac_iterations, generator=generator, samples=samples)
        _pose_figures(res, "ransac", xyz, T_gt, T_ransac, rot_thresh, trans_thresh, xyz_gt, xyz_target_gt,
                      registration_recall_thresh)
    return res


# -------------------------------------------------------------------------------------------------------------------- model
class FragmentDescriptor(nn.Module):
    """Per-point descriptors of a fragment (FragmentKPConv, models/registration/kpconv.py:127-245; FragmentBaseModel,
    base.py:77-138, in "match" mode).  `backbone`: any module with an `output_nc` attribute that maps the batch to (N, C)
    features or to a batch object whose `.x` holds them.  The head carries FragmentKPConv's names: FC_layer.<i> = Linear
    without bias - FastBatchNorm1d - LeakyReLU(0.2) for mlp_nn[i - 1] -> mlp_nn[i], an optional FC_layer.Dropout, and
    FC_layer.Last = Linear(mlp_nn[-1], out_channels) without bias; rows are divided by (norm + eps) when
    normalize_feature.  metric_loss: a module called as (F0, F1, matches, xyz0, xyz1), e.g. the two losses above.

    forward(data, data_target=None, match=None): `output`; with a target and `match` (M, 2) also `output_target` and
    `loss`.  `data.pos` is handed to the loss as the positions."""

    def __init__(self, backbone, mlp_nn, out_channels=32, normalize_feature=True, eps=1e-3, bn_momentum=0.02, dropout=0,
                 metric_loss=None):
        super().__init__()
        if len(mlp_nn) < 1 or mlp_nn[0] != backbone.output_nc:
            raise ValueError("mlp_nn must start with the backbone's output_nc (%d)" % backbone.output_nc)
        self.backbone = backbone
        self.out_channels = out_channels
        self.FC_layer = nn.Sequential()
        in_feat = mlp_nn[0]
        for i in range(1, len(mlp_nn)):
            self.FC_layer.add_module(str(i), nn.Sequential(nn.Linear(in_feat, mlp_nn[i], bias=False),
                                                           FastBatchNorm1d(mlp_nn[i], momentum=bn_momentum),
                                                           nn.LeakyReLU(0.2)))
            in_feat = mlp_nn[i]
        if dropout:
            self.FC_layer.add_module("Dropout", nn.Dropout(p=dropout))
        self.FC_layer.add_module("Last", nn.Linear(in_feat, out_channels, bias=False))
        self.normalize_feature = normalize_feature
        self.eps = eps
        self.metric_loss_module = metric_loss
        self.output = self.output_target = self.loss = None

    @classmethod
    def sparse(cls, input_nc, in_feat=32, mlp_nn=None, eps=1e-20, **kwargs):
        """the sparse voxel U-Net (SparseConv3dUnet("unet_4")) under the head; eps as in models/registration/spconv3d.py"""
        from .sparseconv import SparseConv3dUnet
        backbone = SparseConv3dUnet("unet_4", input_nc, in_feat=in_feat)
        nc = backbone.output_nc
        return cls(backbone, [nc, nc] if mlp_nn is None else mlp_nn, eps=eps, **kwargs)

    @classmethod
    def kpconv(cls, input_nc, in_feat=64, in_grid_size=0.02, num_layers=4, mlp_nn=None, **kwargs):
        """the KPConv U-Net (applications KPConv(architecture="unet")) under the head, conf/models/registration/kpconv.yaml"""
        from .kpconv_unet import KPConv
        backbone = KPConv("unet", input_nc=input_nc, num_layers=num_layers, in_feat=in_feat, in_grid_size=in_grid_size)
        nc = backbone.output_nc
        return cls(backbone, [nc, nc] if mlp_nn is None else mlp_nn, **kwargs)

    def apply_nn(self, data):
        out = self.backbone(data)
        feats = out if torch.is_tensor(out) else out.x
        output = self.FC_layer(feats)
        if self.normalize_feature:
            return output / (torch.norm(output, p=2, dim=1, keepdim=True) + self.eps)
        return output

    def forward(self, data, data_target=None, match=None):
        self.output = self.apply_nn(data)
        self.output_target = self.loss = None
        if data_target is None or match is None:
            return self.output
        self.output_target = self.apply_nn(data_target)
        if self.metric_loss_module is None:
            raise ValueError("a target and matches were given but the model has no metric_loss")
        self.loss = self.metric_loss_module(self.output, self.output_target, match[:, :2], getattr(data, "pos", None),
                                            getattr(data_target, "pos", None))
        return self.output

    def get_output(self):
        return self.output, self.output_target
