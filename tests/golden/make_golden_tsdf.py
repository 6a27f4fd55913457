"""Writes tests/golden/tsdf.npz and README_tsdf.md: what the reference's own TSDF fusion computes on small inputs.

Run in the build container only (needs the reference checkout next to this repository's parent, as the other generators
do).  The reference's datasets/registration/fusion.py and utils.py are imported UNMODIFIED; the third-party names they
import are stubbed here, in this file: numba (njit / jit pass through, prange = range: the decorated functions run as the
plain numpy they are), an empty skimage.measure, an empty imageio (the two path-taking helpers get an `imread` that looks
the path up in a table of arrays), torch_geometric.data.Data as an attribute bag, and the rest as names that are never
called.  pycuda is absent, so the reference runs its CPU mode.  The archive holds data only.

Besides writing the arrays the generator asserts that the inputs sit away from every discontinuity of the rules (a pixel
coordinate on a half-integer, diff == -trunc, c_z == 0, |t| == 0.35) and that the float64 restatement of
torch_points3d_amd/tsdf.py reproduces every stored array; both tables go into the README.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

IMAGES = {}  # path -> array, served by the stubbed imageio.imread


class Data(object):
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def _na(*a, **k):
    raise RuntimeError("stubbed third-party function called")


def load_reference():
    def passthrough(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    _stub("numba", njit=passthrough, jit=passthrough, prange=range)
    _stub("skimage")
    _stub("skimage.measure")
    _stub("imageio")
    _stub("torch_geometric")
    _stub("torch_geometric.data", Data=Data)
    _stub("torch_geometric.transforms", Compose=_na)
    _stub("torch_points_kernels")
    _stub("torch_points_kernels.points_cpu", ball_query=_na)
    _stub("torch_cluster", fps=_na)
    _stub("torch_points3d")
    _stub("torch_points3d.core")
    _stub("torch_points3d.core.data_transform", GridSampling3D=_na, SaveOriginalPosId=_na)
    _stub("torch_points3d.datasets")
    _stub("torch_points3d.datasets.registration")
    mods = []
    for leaf in ("fusion", "utils"):
        name = "torch_points3d.datasets.registration." + leaf
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "torch_points3d/datasets/registration", leaf + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        setattr(sys.modules["torch_points3d.datasets.registration"], leaf, m)
        spec.loader.exec_module(m)
        mods.append(m)
    assert mods[0].FUSION_GPU_MODE == 0
    sys.modules["imageio"].imread = lambda path: IMAGES[path].copy()
    return mods


# ------------------------------------------------------------------------------------------------------------------ inputs
def rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_frames(rng, F, H, W, far=0):
    """raw uint16 depth (a wavy wall about 1.2 m away) with 10 % holes and `far` readings beyond 6 m, and poses"""
    v, u = np.mgrid[0:H, 0:W]
    depths, poses = [], []
    for f in range(F):
        z = 1.2 + 0.18 * np.sin(u / 7.0 + 0.9 * f) + 0.12 * np.cos(v / 5.0 - 0.4 * f) + 0.01 * rng.standard_normal((H, W))
        raw = np.round(z * 1000.0).astype(np.uint16)
        raw[rng.random((H, W)) < 0.10] = 0
        for _ in range(far):
            raw[rng.integers(H), rng.integers(W)] = 6000 + rng.integers(1, 3000)
        pose = np.eye(4)
        pose[:3, :3] = rot(rng.standard_normal(3), 0.12 * rng.standard_normal())
        pose[:3, 3] = 0.08 * rng.standard_normal(3)
        depths.append(raw)
        poses.append(pose)
    return np.stack(depths), np.stack(poses)


def register(tmp, depths, K, poses, tag):
    """the frames as the path lists the reference's helpers take"""
    imgs, trans = [], []
    kpath = os.path.join(tmp, tag + "_K.txt")
    np.savetxt(kpath, K, fmt="%.18e")
    for i in range(len(depths)):
        p = os.path.join(tmp, "%s_%03d.png" % (tag, i))
        IMAGES[p] = depths[i]
        t = os.path.join(tmp, "%s_%03d.txt" % (tag, i))
        np.savetxt(t, poses[i], fmt="%.18e")
        assert np.array_equal(np.loadtxt(t), poses[i])
        imgs.append(p)
        trans.append(t)
    assert np.array_equal(np.loadtxt(kpath), K)
    return imgs, kpath, trans


# --------------------------------------------------------------------------------------------------------------------- gaps
def margins(T, origin, dim, vs, metres, consts, tsdf_before, weight_before):
    """smallest distances of one frame's voxels from the discontinuities of the rules"""
    trunc = 5 * vs
    ax = [T.voxel_axis(origin[a], vs, int(dim[a])).astype(np.float64) for a in range(3)]
    px, py, pz = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    M = consts[:12].reshape(3, 4)
    c = [((M[r, 0] * px + M[r, 1] * py) + M[r, 2] * pz) + M[r, 3] for r in range(3)]
    H, W = metres.shape
    front = c[2] > 0
    cz = np.where(front, c[2], 1.0)
    u = c[0] * consts[12] / cz + consts[14]
    v = c[1] * consts[13] / cz + consts[15]
    near = front & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
    half = np.minimum(np.abs(u - np.floor(u) - 0.5), np.abs(v - np.floor(v) - 0.5))
    ok = front & (np.rint(u) >= 0) & (np.rint(u) < W) & (np.rint(v) >= 0) & (np.rint(v) < H)
    d = np.where(ok, metres[np.where(ok, np.rint(v), 0).astype(int), np.where(ok, np.rint(u), 0).astype(int)], 0.0)
    ok &= d > 0
    edge = np.abs((d - c[2]) + trunc)
    return dict(half=float(half[near].min()) if near.any() else np.inf, czero=float(np.abs(c[2]).min()),
                edge=float(edge[ok].min()) if ok.any() else np.inf)


def main():
    fusion, utils = load_reference()
    from torch_points3d_amd import tsdf as T
    rng = np.random.default_rng(20240611)
    out, gaps, devs = {}, {"half": np.inf, "czero": np.inf, "edge": np.inf, "surface": np.inf}, {}

    def compare(name, ref, mine):
        ref, mine = np.asarray(ref), np.asarray(mine)
        assert ref.shape == mine.shape, (name, ref.shape, mine.shape)
        devs[name] = float(np.abs(ref.astype(np.float64) - mine.astype(np.float64)).max()) if ref.size else 0.0

    def take(g):
        for k in ("half", "czero", "edge"):
            gaps[k] = min(gaps[k], g[k])

    # ---- A: the class on one volume, frame by frame
    H, W, F = 48, 64, 5
    K = np.array([[58.3, 0.0, 31.7], [0.0, 57.9, 23.6], [0.0, 0.0, 1.0]])
    depths, poses = make_frames(rng, F, H, W, far=3)
    weights = np.array([1.0, 0.5, 2.0, 1.0, 0.5])
    bnds = np.array([[-0.713, 0.771], [-0.507, 0.481], [0.633, 1.771]])
    vs = 0.05
    vol = fusion.TSDFVolume(bnds.copy(), vs)
    geo = T.volume_geometry(bnds, vs)
    assert np.array_equal(geo[1], vol._vol_dim) and np.array_equal(geo[2], vol._vol_origin)
    mine_t = np.ones(tuple(geo[1]), np.float32)
    mine_w = np.zeros(tuple(geo[1]), np.float32)
    consts = T.integrate_consts(K, poses, weights, F)
    ts, ws, touched = [], [], 0
    for f in range(F):
        metres = depths[f].astype(float) / 1000.0
        metres[metres > 6] = 0
        assert np.array_equal(metres, T.depth_metres_numpy(depths[f], 1000.0, 6))
        take(margins(T, geo[2], geo[1], vs, metres, consts[f], mine_t, mine_w))
        vol.integrate(metres, K, poses[f], obs_weight=float(weights[f]))
        touched += T.integrate_numpy(mine_t, mine_w, geo[2], vs, metres, consts[f])
        t, w = vol.get_volume()
        ts.append(t.copy())
        ws.append(w.copy())
        compare("vol_tsdf[%d]" % f, t, mine_t)
        compare("vol_weight[%d]" % f, w, mine_w)
    pcd = vol.get_point_cloud(0.35, 0.0)
    gaps["surface"] = min(gaps["surface"], float(np.abs(np.abs(ts[-1][ws[-1] > 0]) - 0.35).min()))
    compare("vol_cloud", pcd, T.surface_numpy(mine_t, mine_w, geo[2], vs, 0.35, 0.0)[0])
    out.update(vol_depths=depths, vol_poses=poses, vol_K=K, vol_weights=weights, vol_bnds=bnds, vol_voxel=np.float64(vs),
               vol_dim=np.asarray(geo[1], np.int64), vol_origin=geo[2], vol_tsdf=np.stack(ts), vol_weight=np.stack(ws),
               vol_cloud=pcd, vol_touched=np.int64(touched))

    with tempfile.TemporaryDirectory() as tmp:
        # ---- B: frusta and bounds (limit_size trims the x axis)
        imgs, kpath, trans = register(tmp, depths, K, poses, "b")
        fr = []
        for f in range(F):
            metres = depths[f] / 1000.0
            metres[metres > 6] = 0
            fr.append(fusion.get_view_frustum(metres, K, poses[f]))
            compare("frustum[%d]" % f, fr[-1], T.get_view_frustum(metres, K, poses[f]))
        bound_free = utils.get_3D_bound(imgs, kpath, trans, 6, limit_size=600, voxel_size=0.05)
        bound_trim = utils.get_3D_bound(imgs, kpath, trans, 6, limit_size=35, voxel_size=0.05)
        dims = (bound_free[:, 1] - bound_free[:, 0]) / 0.05
        assert (dims > 35).sum() == 1, dims  # exactly one axis is trimmed
        compare("bound_free", bound_free, T.get_3D_bound(depths, K, poses, 6, limit_size=600, voxel_size=0.05))
        compare("bound_trim", bound_trim, T.get_3D_bound(depths, K, poses, 6, limit_size=35, voxel_size=0.05))
        out.update(frustum=np.stack(fr), bound_free=bound_free, bound_trim=bound_trim, bound_limit=np.int64(35))

        # ---- C: unprojection with colour
        colour = rng.integers(0, 256, (F, H, W, 3)).astype(np.uint8)
        pcd0, col0 = utils.extract_pcd(depths[0], K, colour[0])
        uc = T.unproject_consts(K, None, 1)
        s, p, pix = T.unproject_numpy(depths[:1], uc)
        compare("extract_pos", pcd0, p)
        assert np.array_equal(col0, colour[0].reshape(-1, 3)[pix])
        worlds, starts = [], [0]
        for f in range(F):
            IMAGES[imgs[f] + ".colour"] = colour[f]
            wpts, wcol = utils.rgbd2pcd(imgs[f], kpath, trans[f], imgs[f] + ".colour")
            worlds.append(wpts)
            starts.append(starts[-1] + len(wpts))
        s, p, pix = T.unproject_numpy(depths, T.unproject_consts(K, poses, F))
        assert np.array_equal(s, np.asarray(starts))
        compare("world_pos", np.concatenate(worlds), p)
        out.update(colour=colour, extract_pos=pcd0, extract_colour=col0, world_pos=np.concatenate(worlds),
                   world_start=np.asarray(starts, np.int64))

        # ---- D: the fragments of 11 frames, 5 per fragment (the third window is one frame long and gives none)
        d11, p11 = make_frames(rng, 11, H, W, far=2)
        imgs, kpath, trans = register(tmp, d11, K, p11, "d")
        frag_dir = os.path.join(tmp, "frag")
        os.makedirs(frag_dir)
        utils.rgbd2fragment_fine(imgs, kpath, trans, frag_dir, num_frame_per_fragment=5, voxel_size=0.06, depth_thresh=6,
                                 limit_size=26)
        names = sorted(os.listdir(frag_dir))
        frags = [torch.load(os.path.join(frag_dir, n), weights_only=False).pos.numpy() for n in names]
        mine = T.rgbd2fragment_fine(d11, K, p11, num_frame_per_fragment=5, voxel_size=0.06, depth_thresh=6, limit_size=26)
        assert len(frags) == len(mine) == 2, (len(frags), len(mine))
        for i, fpos in enumerate(frags):
            compare("fragment[%d]" % i, fpos, mine[i].pos.numpy())
            out["fragment_%d" % i] = fpos
            # gaps of the fragment's own volume
            sel = slice(5 * i, 5 * i + 5)
            b = T.get_3D_bound(d11[sel], K, p11[sel], 6, limit_size=26, voxel_size=0.06)
            compare("fragment_bound[%d]" % i, utils.get_3D_bound(imgs[sel], kpath, trans[sel], 6, limit_size=26, voxel_size=0.06), b)
            g = T.volume_geometry(b, 0.06)
            t = np.ones(tuple(g[1]), np.float32)
            w = np.zeros(tuple(g[1]), np.float32)
            cs = T.integrate_consts(K, p11[sel], 1.0, 5)
            for f in range(5):
                m = T.depth_metres_numpy(d11[sel][f], 1000.0, 6)
                take(margins(T, g[2], g[1], 0.06, m, cs[f], t, w))
                T.integrate_numpy(t, w, g[2], 0.06, m, cs[f])
            gaps["surface"] = min(gaps["surface"], float(np.abs(np.abs(t[w > 0]) - 0.35).min()))
            out["fragment_dim_%d" % i] = np.asarray(g[1], np.int64)
        out.update(frag_depths=d11, frag_poses=p11, frag_voxel=np.float64(0.06), frag_limit=np.int64(26),
                   frag_count=np.int64(len(frags)))

    assert gaps["half"] > 1e-9 and gaps["edge"] > 1e-9 and gaps["czero"] > 1e-9 and gaps["surface"] > 1e-6, gaps
    # the deviation of the float64 restatement from the reference, per stored array (0 = bit-equal); a test's bar for an
    # array with a non-zero entry is 4 x that entry
    out["dev_names"] = np.array(sorted(devs))
    out["dev_values"] = np.array([devs[k] for k in sorted(devs)])
    path = os.path.join(HERE, "tsdf.npz")
    np.savez_compressed(path, **out)

    lines = ["# tsdf.npz", "",
             "Written by `make_golden_tsdf.py` from the reference's own `datasets/registration/fusion.py` and `utils.py`,",
             "imported unmodified.  numba is stubbed (njit / jit pass through, prange = range), skimage.measure and imageio",
             "are empty modules (the path-taking helpers read arrays from a table through a stand-in `imread`), and pycuda",
             "is absent, so **the reference ran its CPU mode**.  numpy %s.  The archive holds data only (%d KB)." % (
                 np.__version__, os.path.getsize(path) // 1024), "",
             "| content | keys |", "|---|---|",
             "| %d frames of %d x %d raw uint16 depth (10 %% holes, readings beyond 6 m), poses, intrinsics, weights 1, 0.5, 2 | `vol_depths`, `vol_poses`, `vol_K`, `vol_weights` |" % (F, H, W),
             "| volume %s at voxel %.2f: tsdf and weight after every frame (%d voxel updates), `get_point_cloud(0.35, 0.0)` | `vol_tsdf`, `vol_weight`, `vol_cloud` |" % (
                 "x".join(str(int(d)) for d in geo[1]), vs, touched),
             "| `get_view_frustum` per frame, `get_3D_bound` free and with `limit_size=35` (trims x) | `frustum`, `bound_free`, `bound_trim` |",
             "| `extract_pcd` with colour of frame 0, `rgbd2pcd` world rows of every frame | `extract_pos`, `extract_colour`, `world_pos`, `world_start`, `colour` |",
             "| `rgbd2fragment_fine` on 11 frames, 5 per fragment, voxel 0.06, `limit_size=26`: %d fragments (%s points; volumes %s); the third window holds one frame and writes none | `frag_depths`, `frag_poses`, `fragment_0`, `fragment_1` |" % (
                 len(frags), ", ".join(str(len(f)) for f in frags),
                 ", ".join("x".join(str(int(d)) for d in out["fragment_dim_%d" % i]) for i in range(len(frags)))),
             "", "## Distance from the discontinuities (asserted by the generator)", "",
             "| quantity | smallest gap found | required |", "|---|---|---|",
             "| pixel coordinate from a half-integer (voxels within one pixel of the image) | %.3e | > 1e-9 |" % gaps["half"],
             "| `diff + trunc` from 0 | %.3e | > 1e-9 |" % gaps["edge"],
             "| `c_z` from 0 | %.3e | > 1e-9 |" % gaps["czero"],
             "| `abs(t)` from 0.35 at extraction | %.3e | > 1e-6 |" % gaps["surface"],
             "", "## The float64 restatement (`torch_points3d_amd/tsdf.py`) against the stored arrays", "",
             "Largest absolute difference per array; 0 means bit-equal.  Where an entry is not 0 (numpy's BLAS taking another",
             "summation order inside the reference's `np.dot`), the test's bar for that array alone is 4 x the entry.", "",
             "| array | max abs difference |", "|---|---|"]
    lines += ["| `%s` | %.3e |" % (k, devs[k]) for k in sorted(devs)]
    with open(os.path.join(HERE, "README_tsdf.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path, os.path.getsize(path), "bytes; gaps", gaps)
    print("non-zero deviations:", {k: v for k, v in devs.items() if v != 0.0})


if __name__ == "__main__":
    main()
