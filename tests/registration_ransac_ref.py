"""Float64 restatement of RANSAC over correspondences (torch on the CPU) for tests/test_gpu_ransac.py and
tests/test_ransac_cpu.py: per-hypothesis Kabsch with the arithmetic of the reference's estimate_transfo
(utils/registration.py:24-43: centred cross-covariance, SVD, determinant correction), batched; distances; counts at
threshold - band, threshold, threshold + band; the refit started from a given hypothesis; and the two test cases.  See
tests/golden/README_ransac.md for what anchors it."""
import torch

import registration_ref as rr

F64 = torch.float64
OUTLIER_ROWS = [1, 5, 20, 32, 74, 17, 27, 77, 88, 89]  # test/test_registration_metrics.py:69


def estimate_transfo(xyz, xyz_target, weight=None):
    """estimate_transfo in float64 for (..., n, 3) inputs, with optional weights (..., n): (..., 3, 4) [R | t]"""
    p, q = xyz.to(F64), xyz_target.to(F64)
    w = torch.ones(p.shape[:-1], dtype=F64) if weight is None else weight.to(F64)
    w = (w / w.sum(-1, keepdim=True)).unsqueeze(-1)
    mp, mq = (w * p).sum(-2), (w * q).sum(-2)
    Q = ((p - mp.unsqueeze(-2)) * w).transpose(-1, -2) @ (q - mq.unsqueeze(-2))
    U, S, Vh = torch.linalg.svd(Q)
    V = Vh.transpose(-1, -2)
    diag = torch.ones(Q.shape[:-1], dtype=F64)
    diag[..., 2] = torch.det(V @ U.transpose(-1, -2))
    R = (V * diag.unsqueeze(-2)) @ U.transpose(-1, -2)
    t = mq - (R @ mp.unsqueeze(-1)).squeeze(-1)
    return torch.cat([R, t.unsqueeze(-1)], -1)


def to4x4(pose):
    T = torch.eye(4, dtype=pose.dtype)
    T[:3] = pose
    return T


def hypotheses(xyz, xyz_target, samples):
    """(H, 3, 4) float64 poses of the sampled correspondences"""
    return estimate_transfo(xyz.to(F64)[samples], xyz_target.to(F64)[samples])


def well_posed(xyz, xyz_target, samples, sv_ratio=1e-2, gap=1e-3):
    """(H,) bool: the hypotheses whose pose is well determined -- the second singular value of the centred source sample
    above sv_ratio of the first, and the two largest eigenvalues of Horn's 4 x 4 matrix apart by more than gap of the
    largest magnitude"""
    p, q = xyz.to(F64)[samples], xyz_target.to(F64)[samples]
    pc, qc = p - p.mean(1, keepdim=True), q - q.mean(1, keepdim=True)
    sv = torch.linalg.svdvals(pc)
    S = pc.transpose(1, 2) @ qc
    A = torch.zeros(len(S), 4, 4, dtype=F64)
    A[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    A[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    A[:, 2, 2] = S[:, 1, 1] - S[:, 0, 0] - S[:, 2, 2]
    A[:, 3, 3] = S[:, 2, 2] - S[:, 0, 0] - S[:, 1, 1]
    A[:, 0, 1] = A[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    A[:, 0, 2] = A[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    A[:, 0, 3] = A[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    A[:, 1, 2] = A[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    A[:, 1, 3] = A[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    A[:, 2, 3] = A[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    ev = torch.linalg.eigvalsh(A)  # ascending
    scale = ev.abs().max(1)[0]
    return (sv[:, 1] > sv_ratio * sv[:, 0]) & (ev[:, 3] - ev[:, 2] > gap * scale) & (scale > 0)


def ill_posed_allowance(n_rows, ransac_n):
    """the share of hypotheses well_posed may exclude: 2 % for samples of 4 or more; a sample of 3 drawn with replacement
    repeats a row with probability 1 - (1 - 1/N)(1 - 2/N), which leaves two distinct points and no unique pose, so that
    share comes on top"""
    return 0.02 + (1.0 - (1.0 - 1.0 / n_rows) * (1.0 - 2.0 / n_rows) if ransac_n == 3 else 0.0)


def distances(poses, xyz, xyz_target):
    """(H, N) float64 |R p_i + t - q_i| for poses (H, 3, 4) (any float dtype, promoted)"""
    P = poses.to(F64)
    p, q = xyz.to(F64), xyz_target.to(F64)
    return ((p @ P[:, :, :3].transpose(1, 2)) + P[:, None, :, 3] - q).norm(dim=2)


def counts_banded(poses, xyz, xyz_target, threshold, band):
    """(lo, mid, hi) int64 (H,): the counts at threshold - band, threshold, threshold + band; a pose that is not finite
    counts 0"""
    out = []
    P = poses.to(F64)
    finite = torch.isfinite(P).all(2).all(1)
    d = distances(torch.where(finite[:, None, None], P, torch.zeros_like(P)), xyz, xyz_target)
    for thr in (threshold - band, threshold, threshold + band):
        out.append(torch.where(finite, (d < thr).sum(1), torch.zeros(len(P), dtype=torch.int64)))
    return out


def refit(xyz, xyz_target, threshold, pose, refine=1):
    """the pose after `refine` rounds of Kabsch over the inliers of the current pose (fewer than 3: it stays), then the
    inlier count and the sum of squared inlier distances under the final pose, and the least | |d| - threshold | met
    on the way (the margin every decision had)"""
    pose = pose.to(F64)
    margin = float("inf")
    for _ in range(refine):
        d = distances(pose[None], xyz, xyz_target)[0]
        margin = min(margin, float((d - threshold).abs().min()))
        inl = d < threshold
        if int(inl.sum()) >= 3:
            pose = estimate_transfo(xyz[inl], xyz_target[inl])
    d = distances(pose[None], xyz, xyz_target)[0]
    margin = min(margin, float((d - threshold).abs().min()))
    inl = d < threshold
    return pose, int(inl.sum()), float((d[inl] ** 2).sum()), margin


def case_a():
    """the reference's test_ransac (test/test_registration_metrics.py:61-72) with a fixed generator and a fixed pose:
    (xyz, target, T_gt) fp32, threshold 0.01"""
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(100, 3, generator=gen)
    T = torch.eye(4)
    T[:3, :3] = rr.rotation([1.0, 1.0, 1.0], 0.9).float()
    T[:3, 3] = torch.tensor([0.2, 0.3, -0.15])
    b = a.mm(T[:3, :3].T) + T[:3, 3]
    b[OUTLIER_ROWS] *= 42
    return a, b, T


def case_b(n=1025, seed=1025):
    """test_gpu_registration._fgr_case: 30 % outliers, noise 0.003; threshold 0.05"""
    gen = torch.Generator().manual_seed(seed)
    T = torch.eye(4, dtype=F64)
    T[:3, :3] = rr.rotation([0.5, 0.2, -0.7], 0.5)
    T[:3, 3] = torch.tensor([0.2, 0.3, -0.15], dtype=F64)
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    tgt = (xyz.double() @ T[:3, :3].T + T[:3, 3]).float() + 0.003 * torch.randn(n, 3, generator=gen)
    bad = torch.randperm(n, generator=gen)[: (3 * n) // 10]
    tgt[bad] = torch.rand(len(bad), 3, generator=gen) * 3 - 1.5
    return xyz, tgt, T


def draw(n_rows, H, ransac_n, seed):
    return torch.randint(0, n_rows, (H, ransac_n), generator=torch.Generator().manual_seed(seed))
