"""Shared inputs of the TSDF tests: the golden archive and hand-derived cases whose answers are written out here.

Every hand case is a dict: origin (3,) fp32, dims, voxel (trunc = 5 * voxel), depths (F, H, W) float64 metres, K (3, 3),
poses (F, 4, 4), weights (F,), and the expected tsdf / weight volumes.  All inputs are exact binary fractions, so the
expected values follow from the rules of torch_points3d_amd/tsdf.py with pencil and paper."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsdf.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def golden_bar(name):
    """0.0 where the generator found the float64 restatement bit-equal to the reference; otherwise 4 x the deviation it
    measured for that array (README_tsdf.md)"""
    g = golden()
    dev = dict(zip((str(n) for n in g["dev_names"]), g["dev_values"]))
    return 4.0 * float(dev[name])


def assert_golden(name, got, want):
    bar = golden_bar(name)
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if bar == 0.0:
        assert np.array_equal(got, want), name
    else:
        assert np.abs(got - want).max() <= bar, (name, np.abs(got - want).max(), bar)


def _pose(tx=0.0, ty=0.0, tz=0.0):
    p = np.eye(4)
    p[:3, 3] = (tx, ty, tz)
    return p


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _f32(x):
    return np.float32(x)


def hand_cases():
    cases = []
    T = 1.25  # trunc of every case: 5 voxels of 0.25

    # half-even rounding: identity pose, origin 0, fx = 2, cx = 0.  The voxels (i, 0, 4) lie at depth 1 and project to
    # column 0.5 i: i = 1, 3, 5 sit on 0.5, 1.5, 2.5 and must read columns 0, 2, 2 (roundf would read 1, 2, 3).
    row = np.array([1.0, 1.125, 1.25, 1.375])
    cols = [0, 0, 1, 2, 2, 2]  # rint(0, 0.5, 1, 1.5, 2, 2.5)
    tsdf = np.ones((6, 1, 5), np.float32)
    weight = np.zeros((6, 1, 5), np.float32)
    for k in range(1, 5):       # depth 0.25 k, column rint(0.5 i / (0.25 k)) = rint(2 i / k)
        for i in range(6):
            c = int(np.rint(2.0 * i / k))
            if c < 4:
                tsdf[i, 0, k] = _f32(min(1.0, (row[c] - 0.25 * k) / T))
                weight[i, 0, k] = 1.0
    for i in range(6):  # the row the case is about, written out: diff = row[col] - 1
        assert tsdf[i, 0, 4] == _f32((row[cols[i]] - 1.0) / T)
    assert [float(tsdf[i, 0, 4]) for i in (1, 3, 5)] == [0.0, float(_f32(0.2)), float(_f32(0.2))]
    cases.append(dict(name="half_even", origin=(0.0, 0.0, 0.0), dims=(6, 1, 5), voxel=0.25, depths=row.reshape(1, 1, 4),
                      K=_K(2.0, 2.0, 0.0, 0.0), poses=_pose()[None], weights=np.array([1.0]), tsdf=tsdf, weight=weight))

    # truncation edge and c_z == 0: one pixel, a column of voxels at depth 0.25 k, reading d = 0.75.  k = 0 has c_z == 0
    # (skipped), k = 8 has diff == -trunc exactly (integrated, dist = -1), k = 9 lies behind the margin (skipped).
    tsdf = np.ones((1, 1, 10), np.float32)
    weight = np.zeros((1, 1, 10), np.float32)
    for k in range(1, 9):
        tsdf[0, 0, k] = _f32((0.75 - 0.25 * k) / T)
        weight[0, 0, k] = 1.0
    assert tsdf[0, 0, 8] == -1.0 and tsdf[0, 0, 9] == 1.0 and weight[0, 0, 0] == 0.0
    cases.append(dict(name="trunc_edge", origin=(0.0, 0.0, 0.0), dims=(1, 1, 10), voxel=0.25,
                      depths=np.full((1, 1, 1), 0.75), K=_K(1.0, 1.0, 0.0, 0.0), poses=_pose()[None],
                      weights=np.array([1.0]), tsdf=tsdf, weight=weight))

    # clamp: the same column reading d = 5: diff >= 2.75 > trunc everywhere, dist = 1, t stays 1 while the weight counts
    tsdf = np.ones((1, 1, 10), np.float32)
    weight = np.ones((1, 1, 10), np.float32)
    weight[0, 0, 0] = 0.0
    cases.append(dict(name="clamp", origin=(0.0, 0.0, 0.0), dims=(1, 1, 10), voxel=0.25, depths=np.full((1, 1, 1), 5.0),
                      K=_K(1.0, 1.0, 0.0, 0.0), poses=_pose()[None], weights=np.array([1.0]), tsdf=tsdf, weight=weight))

    # behind the camera: the camera stands at z = 0.5, so k = 0, 1 have c_z < 0 and k = 2 has c_z == 0
    tsdf = np.ones((1, 1, 10), np.float32)
    weight = np.zeros((1, 1, 10), np.float32)
    for k in range(3, 10):
        tsdf[0, 0, k] = _f32(min(1.0, (0.75 - (0.25 * k - 0.5)) / T))
        weight[0, 0, k] = 1.0
    cases.append(dict(name="behind", origin=(0.0, 0.0, 0.0), dims=(1, 1, 10), voxel=0.25, depths=np.full((1, 1, 1), 0.75),
                      K=_K(1.0, 1.0, 0.0, 0.0), poses=_pose(tz=0.5)[None], weights=np.array([1.0]), tsdf=tsdf,
                      weight=weight))

    # image borders and holes: voxels (i, j, 0) at depth 1 with fx = fy = 4: px = i, py = j - 1 on a 2 x 2 image.
    # px == W (i = 2, 3) and py == -1 (j = 0) are skipped, the pixel (py 0, px 1) holds d == 0.
    depth = np.array([[1.5, 0.0], [1.25, 1.75]])
    tsdf = np.ones((4, 3, 1), np.float32)
    weight = np.zeros((4, 3, 1), np.float32)
    for (i, j), d in {(0, 1): 1.5, (0, 2): 1.25, (1, 2): 1.75}.items():
        tsdf[i, j, 0] = _f32((d - 1.0) / T)
        weight[i, j, 0] = 1.0
    cases.append(dict(name="borders", origin=(0.0, -0.25, 1.0), dims=(4, 3, 1), voxel=0.25, depths=depth[None],
                      K=_K(4.0, 4.0, 0.0, 0.0), poses=_pose()[None], weights=np.array([1.0]), tsdf=tsdf, weight=weight))

    # running mean: one voxel at depth 1 over three frames with weights 1, 0.5, 2 reading 1.25, 0.75, 1.5
    dist = [(1.25 - 1.0) / T, (0.75 - 1.0) / T, (1.5 - 1.0) / T]  # 0.2, -0.2, 0.4 as doubles
    t1 = _f32((np.float64(_f32(0.0) * _f32(1.0)) + 1.0 * dist[0]) / np.float64(_f32(1.0)))
    t2 = _f32((np.float64(_f32(1.0) * t1) + 0.5 * dist[1]) / np.float64(_f32(1.5)))
    t3 = _f32((np.float64(_f32(1.5) * t2) + 2.0 * dist[2]) / np.float64(_f32(3.5)))
    assert type(_f32(1.5) * t2) is np.float32
    cases.append(dict(name="running_mean", origin=(0.0, 0.0, 1.0), dims=(1, 1, 1), voxel=0.25,
                      depths=np.array([1.25, 0.75, 1.5]).reshape(3, 1, 1), K=_K(1.0, 1.0, 0.0, 0.0),
                      poses=np.stack([_pose()] * 3), weights=np.array([1.0, 0.5, 2.0]),
                      tsdf=np.full((1, 1, 1), t3, np.float32), weight=np.full((1, 1, 1), 3.5, np.float32),
                      steps=[(t1, 1.0), (t2, 1.5), (t3, 3.5)]))
    return cases


def random_scene(seed, dims, F, H=8, W=8, voxel=None, raw=True):
    """a small volume (longest side 0.6 m unless a voxel size is given) in front of F slightly moved cameras looking at a
    wavy wall about 0.6 m away; raw uint16 depth with holes (raw=False: the same in float64 metres)"""
    rng = np.random.default_rng(seed)
    X, Y, Z = dims
    voxel = 0.6 / max(dims) if voxel is None else voxel
    origin = np.array([-0.5 * X * voxel, -0.5 * Y * voxel, 0.55 - 0.5 * Z * voxel], np.float32)
    v, u = np.mgrid[0:H, 0:W]
    depths, poses = [], []
    for f in range(F):
        z = 0.6 + 0.08 * np.sin(u * 0.9 + f) + 0.05 * np.cos(v * 0.7 - f) + 0.004 * rng.standard_normal((H, W))
        r = np.round(z * 1000.0).astype(np.uint16)
        r[rng.random((H, W)) < 0.1] = 0
        depths.append(r)
        a = 0.05 * rng.standard_normal()
        p = np.eye(4)
        p[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        p[:3, 3] = 0.03 * rng.standard_normal(3)
        poses.append(p)
    depths = np.stack(depths) if F else np.zeros((0, H, W), np.uint16)
    poses = np.stack(poses) if F else np.zeros((0, 4, 4))
    span = max(X, Y) * voxel
    K = _K(0.2 * W / span + 0.013, 0.2 * H / span + 0.007, 0.5 * W - 0.31, 0.5 * H - 0.27)
    weights = np.array([(1.0, 0.5, 2.0)[f % 3] for f in range(F)])
    if not raw:
        depths = depths.astype(np.float64) / 1000.0
    return dict(origin=origin, dims=dims, voxel=voxel, depths=depths, K=K, poses=poses, weights=weights)
