"""FPFH, the hand-crafted baseline of the registration benchmark (reference scripts/test_registration_scripts/fpfh.py:
open3d's estimate_normals(KDTreeSearchParamHybrid) followed by compute_fpfh_feature(KDTreeSearchParamHybrid)).

open3d is not available, so its documented algorithm is restated here, as recalled and not compared with open3d.  The
numpy float64 functions of this file ARE the definition: csrc/fpfh.hip implements the same rules on the device
(torchpoints.hybrid_search / estimate_normals / spfh_counts / fpfh), and CPU tensors are served by the numpy forms.

Stated deviations from open3d:
  * normals without a viewpoint are signed so that their component of largest magnitude (lowest axis on ties) is
    positive (open3d leaves the eigen solver's sign);
  * the swap test of the pair feature compares |a1| < |a2| where open3d compares acos|a1| > acos|a2| (the same order,
    without the transcendental);
  * the bin of the angle feature is decided by comparing (cos, sin) against ten edge directions held as literals, never
    by a library atan2: with +, -, *, /, sqrt only the device's counts equal numpy's exactly.
"""
import numpy as np
import torch

from . import torchpoints as tp

BINS = 11
# (cos, sin) of the ten interior bin edges -pi + 2 pi e / 11, e = 1 .. 10 (FPFH_EDGE of csrc/fpfh.hip holds the same
# literals; tp3d_fpfh_edge_table exports them)
EDGE_TABLE = (
    (-0.84125353283118109, -0.54064081745559778),
    (-0.41541501300188632, -0.90963199535451844),
    (0.14231483827328512, -0.98982144188093268),
    (0.6548607339452851, -0.75574957435425827),
    (0.95949297361449748, -0.2817325568414295),
    (0.95949297361449748, 0.2817325568414295),
    (0.6548607339452851, 0.75574957435425827),
    (0.14231483827328512, 0.98982144188093268),
    (-0.41541501300188616, 0.90963199535451855),
    (-0.84125353283118132, 0.54064081745559744),
)


def fpfh_config():
    """the four numbers of the reference's conf/fpfh.yaml"""
    return dict(radius=0.3, max_nn=256, radius_normal=0.093, max_nn_normal=17)


# ------------------------------------------------------------------------------------------------------------ hybrid search
def hybrid_search_numpy(x, y, radius, max_nn, batch_x=None, batch_y=None):
    """(idx (Nq, max_nn) int32, dist2 (Nq, max_nn) float32, count (Nq,) int32), padded with -1: of the rows of x in the
    query's own cloud with (dx*dx + dy*dy) + dz*dz < radius*radius in float32, the max_nn smallest by (dist2, index)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    bx = np.zeros(len(x), np.int64) if batch_x is None else np.asarray(batch_x, dtype=np.int64)
    by = np.zeros(len(y), np.int64) if batch_y is None else np.asarray(batch_y, dtype=np.int64)
    if len(bx) > 1 and (bx[1:] < bx[:-1]).any():
        raise ValueError("batch_x must be sorted")
    max_nn = int(max_nn)
    r2 = np.float32(radius) * np.float32(radius)
    Nq = len(y)
    idx = np.full((Nq, max_nn), -1, np.int32)
    dist2 = np.full((Nq, max_nn), -1.0, np.float32)
    count = np.zeros(Nq, np.int32)
    for b in np.unique(by):
        lo, hi = np.searchsorted(bx, b, "left"), np.searchsorted(bx, b, "right")
        rows = np.nonzero(by == b)[0]
        if hi == lo:
            continue
        xs = x[lo:hi]
        step = max(1, (1 << 22) // (hi - lo))
        for r0 in range(0, len(rows), step):
            q = rows[r0:r0 + step]
            dx = xs[None, :, 0] - y[q, None, 0]
            dy = xs[None, :, 1] - y[q, None, 1]
            dz = xs[None, :, 2] - y[q, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            qi, ci = np.nonzero(d < r2)  # ascending (query, index)
            dv = d[qi, ci]
            order = np.lexsort((ci, dv, qi))  # by query, then distance, then index
            qi, ci, dv = qi[order], ci[order], dv[order]
            first = np.searchsorted(qi, np.arange(len(q)), "left")
            rank = np.arange(len(qi)) - first[qi]
            keep = rank < max_nn
            idx[q[qi[keep]], rank[keep]] = (ci[keep] + lo).astype(np.int32)
            dist2[q[qi[keep]], rank[keep]] = dv[keep]
            count[q] = np.minimum(np.bincount(qi, minlength=len(q)), max_nn).astype(np.int32)
    return idx, dist2, count


# ------------------------------------------------------------------------------------------------------------------ normals
def _jacobi_rotate(A, V, p, q, on):
    """one Jacobi rotation in the (p, q) plane of the symmetric 3 x 3 matrices A (n, 3, 3) with eigenvector columns V, on
    the rows `on` (csrc/ransac_horn.h: horn_rotate)"""
    apq = A[:, p, q].copy()
    do = on & (apq != 0.0)
    safe = np.where(do, apq, 1.0)
    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * safe)
    t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    t, c, s = np.where(do, t, 0.0), np.where(do, c, 1.0), np.where(do, s, 0.0)
    A[:, p, p] = np.where(do, A[:, p, p] - t * apq, A[:, p, p])
    A[:, q, q] = np.where(do, A[:, q, q] + t * apq, A[:, q, q])
    A[:, p, q] = A[:, q, p] = np.where(do, 0.0, apq)
    k = 3 - p - q
    akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
    A[:, k, p] = A[:, p, k] = np.where(do, c * akp - s * akq, akp)
    A[:, k, q] = A[:, q, k] = np.where(do, s * akp + c * akq, akq)
    for r in range(3):
        vp, vq = V[:, r, p].copy(), V[:, r, q].copy()
        V[:, r, p] = np.where(do, c * vp - s * vq, vp)
        V[:, r, q] = np.where(do, s * vp + c * vq, vq)


JACOBI_MAX_SWEEPS = 16


def smallest_eigenvector(cov):
    """(n, 3) unit eigenvectors of the smallest eigenvalue (the lowest index among equal ones) of the symmetric matrices
    cov (n, 3, 3), by cyclic Jacobi sweeps (0,1) (0,2) (1,2)"""
    with np.errstate(all="ignore"):
        A = np.array(cov, dtype=np.float64)
        V = np.broadcast_to(np.eye(3), A.shape).copy()
        for _ in range(JACOBI_MAX_SWEEPS):
            off = (A[:, 0, 1] * A[:, 0, 1] + A[:, 0, 2] * A[:, 0, 2]) + A[:, 1, 2] * A[:, 1, 2]
            diag = (A[:, 0, 0] * A[:, 0, 0] + A[:, 1, 1] * A[:, 1, 1]) + A[:, 2, 2] * A[:, 2, 2]
            on = off > 1e-36 * diag
            if not on.any():
                break
            _jacobi_rotate(A, V, 0, 1, on)
            _jacobi_rotate(A, V, 0, 2, on)
            _jacobi_rotate(A, V, 1, 2, on)
        best = np.zeros(len(A), np.int64)
        lam = A[:, 0, 0].copy()
        for m in (1, 2):
            less = A[:, m, m] < lam
            lam = np.where(less, A[:, m, m], lam)
            best = np.where(less, m, best)
        n = V[np.arange(len(A)), :, best]
        return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


def neighbourhood_covariance(pos, idx, count):
    """(N, 3, 3) float64: sum (p - m)(p - m)^T / k over the k = count neighbours of every row in slot order, m their mean in
    slot order, from the float32 coordinates (rows with k == 0: zeros)"""
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    N, K = idx.shape
    k = count.astype(np.int64)
    m = np.zeros((N, 3))
    for s in range(K):
        m += np.where((s < k)[:, None], p[idx[:, s]], 0.0)
    with np.errstate(all="ignore"):
        m = m / k[:, None]
        cov = np.zeros((N, 3, 3))
        for s in range(K):
            d = np.where((s < k)[:, None], p[idx[:, s]] - m, 0.0)
            cov += d[:, :, None] * d[:, None, :]
        cov = cov / k[:, None, None]
    return np.where((k > 0)[:, None, None], cov, 0.0)


def estimate_normals_numpy(pos, idx, count, viewpoint=None):
    """(N, 3) float32 normals from the neighbour table of hybrid_search (slot 0 included); viewpoint (3,) or (N, 3)"""
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    cov = neighbourhood_covariance(pos, idx, count)
    n = smallest_eigenvector(cov)
    if viewpoint is not None:
        d = np.asarray(viewpoint, dtype=np.float64).reshape(-1, 3) - p
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] < 0.0
    else:
        a = np.abs(n)
        top = np.where(a[:, 1] > a[:, 0], 1, 0)
        top = np.where(a[:, 2] > a[np.arange(len(a)), top], 2, top)
        flip = n[np.arange(len(n)), top] < 0.0
    n = np.where(flip[:, None], -n, n)
    n = np.where((count < 3)[:, None], np.array([0.0, 0.0, 1.0]), n)
    return n.astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- pair feature
def angle_bin(c, s):
    """the bin floor(11 (angle + pi) / 2 pi), clamped to [0, 10], of the direction (c, s), decided against EDGE_TABLE;
    (0, 0) goes to bin 5"""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    b = np.zeros(c.shape, np.int64)
    for e, (ec, es) in enumerate(EDGE_TABLE):
        cross = ec * s - es * c
        if e < 5:  # an edge below the axis: the direction is past it unless it lies below the axis and before the edge
            b += ~((s < 0.0) & (cross < 0.0))
        else:
            b += (s >= 0.0) & (cross >= 0.0)
    return np.where((c == 0.0) & (s == 0.0), 5, b)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_bins(p1, n1, p2, n2):
    """(..., 3) int64: the bins of the three Darboux-frame features (angle, v . n2, the larger-angle cosine) of the pairs,
    in double from the given coordinates"""
    with np.errstate(all="ignore"):
        p1, n1, p2, n2 = (np.asarray(a, dtype=np.float64) for a in (p1, n1, p2, n2))
        dp = p2 - p1
        d = np.sqrt(_dot(dp, dp))
        a1 = _dot(n1, dp) / d
        a2 = _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        f2 = np.where(swap, -a2, a1)
        m1 = np.where(swap[..., None], n2, n1)
        m2 = np.where(swap[..., None], n1, n2)
        dp = np.where(swap[..., None], -dp, dp)
        v = _cross(dp, m1)
        vn = np.sqrt(_dot(v, v))
        zero = (d == 0.0) | (vn == 0.0)
        v = v / vn[..., None]
        w = _cross(m1, v)
        f1 = np.where(zero, 0.0, _dot(v, m2))
        f2 = np.where(zero, 0.0, f2)
        c = np.where(zero, 1.0, _dot(m1, m2))
        s = np.where(zero, 0.0, _dot(w, m2))
        b0 = np.where(zero, 5, angle_bin(c, s))
        f1 = np.where(np.isnan(f1), 0.0, f1)
        f2 = np.where(np.isnan(f2), 0.0, f2)
        b1 = np.clip(np.floor((11.0 * (f1 + 1.0)) * 0.5), 0, 10).astype(np.int64)
        b2 = np.clip(np.floor((11.0 * (f2 + 1.0)) * 0.5), 0, 10).astype(np.int64)
    return np.stack([b0, b1, b2], -1)


def spfh_counts_numpy(pos, normals, idx, count):
    """(N, 33) int32: for every row the number of its slots 1 .. k - 1 that fall into each bin of the three blocks"""
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    n = np.asarray(normals, dtype=np.float32).astype(np.float64)
    N, K = idx.shape
    out = np.zeros((N, 3 * BINS), np.int32)
    for s in range(1, K):
        rows = np.nonzero(s < count)[0]
        if len(rows) == 0:
            break
        j = idx[rows, s]
        bins = pair_bins(p[rows], n[rows], p[j], n[j])
        for blk in range(3):
            out[rows, blk * BINS + bins[:, blk]] += 1
    return out


def spfh_values(counts, count):
    """(N, 33) float64 SPFH: counts * hist_incr with hist_incr = 100 / (k - 1); rows with k <= 1 are zero"""
    k = np.asarray(count, dtype=np.int64)
    incr = np.where(k > 1, 100.0 / np.maximum(k - 1, 1).astype(np.float64), 0.0)
    return np.asarray(counts).astype(np.float64) * incr[:, None]


def fpfh_numpy(pos, idx, count, counts, rows=None):
    """(R, 33) float64 FPFH of `rows` (default: all): the SPFH rows of the slots 1 .. k - 1 weighted by 1 / d2 (slots with
    d2 == 0 skipped), each block normalised to 100, plus the row's own SPFH; sums in slot order, bins ascending"""
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    spfh = spfh_values(counts, count)
    rows = np.arange(len(p)) if rows is None else np.asarray(rows, dtype=np.int64)
    R, K = len(rows), idx.shape[1]
    acc = np.zeros((R, 3 * BINS))
    tot = np.zeros((R, 3))
    k = count[rows]
    with np.errstate(all="ignore"):
        for s in range(1, K):
            j = np.where(s < k, idx[rows, s], 0)
            d = p[j] - p[rows]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            use = (s < k) & (d2 != 0.0)
            if not (s < k).any():
                break
            term = np.where(use[:, None], spfh[j] / np.where(use, d2, 1.0)[:, None], 0.0)
            acc += term
            for b in range(3 * BINS):
                tot[:, b // BINS] += term[:, b]
        t = np.repeat(tot, BINS, axis=1)
        out = np.where(t != 0.0, (acc * 100.0) / np.where(t != 0.0, t, 1.0), 0.0) + spfh[rows]
    return out


# ---------------------------------------------------------------------------------------------------------------- the class
class FPFH(object):
    """The descriptor of the reference's script, with its signature and defaults: callable on an attribute bag with `pos`
    (N, 3), an optional sorted `batch` (several fragments per call) and optional `keypoints` (rows of pos); returns the
    (len(keypoints), 33) float32 rows (all rows without keypoints) on the device of `pos`.  `viewpoint` ((3,) or
    (clouds, 3)) orients the normals; without it the largest component of every normal is positive."""

    def __init__(self, radius=0.3, max_nn=128, radius_normal=0.3, max_nn_normal=17, viewpoint=None):
        self.radius, self.max_nn = float(radius), int(max_nn)
        self.radius_normal, self.max_nn_normal = float(radius_normal), int(max_nn_normal)
        self.viewpoint = viewpoint

    def __call__(self, data):
        pos = data.pos
        batch = getattr(data, "batch", None)
        keypoints = getattr(data, "keypoints", None)
        normals = tp.estimate_normals(pos, batch, self.radius_normal, self.max_nn_normal, viewpoint=self.viewpoint)
        idx, _, count = tp.hybrid_search(pos, pos, self.radius, self.max_nn, batch, batch)
        counts = tp.spfh_counts(pos, normals, idx, count)
        return tp.fpfh(pos, normals, idx, count, counts, rows=keypoints)
