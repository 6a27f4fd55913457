"""What the FPFH tests share: an independent brute-force form of the hybrid search (one query at a time, a Python sort on
(dist2, index)), the seeded inputs, and the known answers derived by hand.  Every other rule is defined by the numpy
restatement in torch_points3d_amd/fpfh.py."""
import numpy as np

# Points on the plane z = 0 with all normals (0, 0, 1): for every pair n1 . dp = n2 . dp = 0, so a1 = a2 = 0 (no swap,
# f2 = 0), v = dp x n1 is a unit vector in the plane, v . n2 = 0 (f1 = 0), w = n1 x v lies in the plane, so the angle is
# atan2(w . n2, n1 . n2) = atan2(0, 1) = 0: each feature falls into floor(11 * 0.5) = 5 of its block.
PLANE_BINS = (5, 16, 27)


def brute_search(x, y, radius, max_nn, batch_x=None, batch_y=None):
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    bx = np.zeros(len(x), np.int64) if batch_x is None else np.asarray(batch_x)
    by = np.zeros(len(y), np.int64) if batch_y is None else np.asarray(batch_y)
    r2 = np.float32(radius) * np.float32(radius)
    idx = np.full((len(y), max_nn), -1, np.int32)
    dist2 = np.full((len(y), max_nn), -1.0, np.float32)
    count = np.zeros(len(y), np.int32)
    for q in range(len(y)):
        hits = []
        for j in np.nonzero(bx == by[q])[0]:
            dx, dy, dz = x[j, 0] - y[q, 0], x[j, 1] - y[q, 1], x[j, 2] - y[q, 2]
            d = np.float32(np.float32(dx * dx + dy * dy) + dz * dz)
            if d < r2:
                hits.append((d, int(j)))
        hits.sort()
        hits = hits[:max_nn]
        count[q] = len(hits)
        for s, (d, j) in enumerate(hits):
            idx[q, s], dist2[q, s] = j, d
    return idx, dist2, count


def sheet(n=600, seed=5):
    """a noisy sheet over the unit square, z = 0.02 randn"""
    g = np.random.default_rng(seed)
    p = g.random((n, 3))
    p[:, 2] = 0.02 * g.standard_normal(n)
    return p.astype(np.float32)


def cube(n=600, seed=6):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def batched():
    """the sheet, the cube, a 2-point and a 1-point cloud: (pos, batch)"""
    parts = [sheet(), cube(), np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]], np.float32), np.array([[1.0, 2.0, 3.0]], np.float32)]
    batch = np.concatenate([np.full(len(p), b, np.int64) for b, p in enumerate(parts)])
    return np.concatenate(parts), batch


def plane(n=200, seed=7):
    g = np.random.default_rng(seed)
    p = g.random((n, 3))
    p[:, 2] = 0.0
    return p.astype(np.float32)


def on_radius_pair():
    """two clouds' worth of points of which rows 0 and 1 lie exactly radius = 0.25 apart in fp32 (d2 == r2: no hit), and
    rows 0 and 2 one ulp inside"""
    p = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [np.nextafter(np.float32(0.25), np.float32(0)), 0.0, 0.0],
                  [0.0, 0.5, 0.0]], np.float32)
    return p, 0.25


def rigid(seed=3):
    """a rotation (Rodrigues, angle 0.7 about a seeded axis) and a translation, float64"""
    g = np.random.default_rng(seed)
    a = g.standard_normal(3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    return R, np.array([0.3, -0.2, 0.5])
