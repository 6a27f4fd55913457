"""TSDF fusion on the GPU (csrc/tsdf.hip; torchpoints.tsdf_integrate / tsdf_surface / depth_unproject; tsdf.TSDFVolume)
against the float64 numpy definition of torch_points3d_amd/tsdf.py, which tests/test_tsdf_cpu.py holds to the reference's
own results and to hand-derived answers.  Everything is compared with torch.equal: the device evaluates the same
operations in the same order with one rounding each."""
import numpy as np
import pytest
import torch

import tsdf_cases as tc
from torch_points3d_amd import tsdf as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tp():
    from torch_points3d_amd import torchpoints
    return torchpoints


def dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.uint16).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_depth(a):
    return torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint16 else np.ascontiguousarray(a))


def fresh(dims, device):
    return (torch.ones(tuple(dims), dtype=torch.float32, device=device),
            torch.zeros(tuple(dims), dtype=torch.float32, device=device))


def integrate(tp, c, device, depths=None, frames=None):
    t, w = fresh(c["dims"], device)
    d = c["depths"] if depths is None else depths
    sel = slice(None) if frames is None else frames
    d = d[sel]
    d = (dev(d) if device != "cpu" else host_depth(d)) if isinstance(d, np.ndarray) else d
    tp.tsdf_integrate(t, w, c["origin"], c["voxel"], d, c["K"], c["poses"][sel], c["weights"][sel], depth_thresh=6)
    return t, w


def both_equal(tp, c, what):
    t, w = integrate(tp, c, DEV)
    th, wh = integrate(tp, c, "cpu")
    assert torch.equal(w.cpu(), wh), what
    assert torch.equal(t.cpu(), th), what
    return t, w, th, wh


_host = {}


def host_scene(tp, seed, dims, F, **kw):
    """a random scene with its host volumes: computed once, never changed"""
    key = (seed, tuple(dims), F, tuple(sorted(kw.items())))
    if key not in _host:
        c = tc.random_scene(seed, dims, F, **kw)
        _host[key] = (c,) + tuple(integrate(tp, c, "cpu"))
    return _host[key]


# ------------------------------------------------------------------------------------------------------------ the rules
@pytest.mark.parametrize("case", tc.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(tp, case):
    t, w, _, _ = both_equal(tp, case, case["name"])
    assert torch.equal(t.cpu(), torch.from_numpy(case["tsdf"])) and torch.equal(w.cpu(), torch.from_numpy(case["weight"]))


def test_reference_volume_frame_by_frame(tp):
    g = tc.golden()
    vol = T.TSDFVolume(g["vol_bnds"], float(g["vol_voxel"]), device=DEV)
    for f in range(g["vol_depths"].shape[0]):
        vol.integrate(g["vol_depths"][f], g["vol_K"], g["vol_poses"][f], obs_weight=float(g["vol_weights"][f]), depth_thresh=6)
        t, w = vol.get_volume()
        assert t.device.type == "cuda"
        tc.assert_golden("vol_tsdf[%d]" % f, t.cpu().numpy(), g["vol_tsdf"][f])
        tc.assert_golden("vol_weight[%d]" % f, w.cpu().numpy(), g["vol_weight"][f])
    tc.assert_golden("vol_cloud", vol.get_point_cloud(0.35, 0.0).cpu().numpy(), g["vol_cloud"])


def test_reference_fragments_bounds_and_unprojection(tp):
    g = tc.golden()
    d11 = dev(g["frag_depths"])
    frags = T.rgbd2fragment_fine(d11, g["vol_K"], g["frag_poses"], num_frame_per_fragment=5,
                                 voxel_size=float(g["frag_voxel"]), depth_thresh=6, limit_size=int(g["frag_limit"]))
    assert len(frags) == 2 and frags[0].pos.device.type == "cuda"
    for i, f in enumerate(frags):
        tc.assert_golden("fragment[%d]" % i, f.pos.cpu().numpy(), g["fragment_%d" % i])
    d5 = dev(g["vol_depths"])
    tc.assert_golden("bound_trim", T.get_3D_bound(d5, g["vol_K"], g["vol_poses"], 6, limit_size=int(g["bound_limit"]),
                                                  voxel_size=0.05), g["bound_trim"])
    res = tp.depth_unproject(d5, g["vol_K"], g["vol_poses"])
    want = tp.depth_unproject(host_depth(g["vol_depths"]), g["vol_K"], g["vol_poses"])
    assert torch.equal(res.start.cpu(), want.start) and torch.equal(res.pixel.cpu(), want.pixel)
    assert torch.equal(res.pos.cpu(), want.pos)
    tc.assert_golden("world_pos", res.pos.cpu().numpy(), g["world_pos"])
    rough = T.rgbd2fragment_rough(d5, g["vol_K"], g["vol_poses"], colors=dev(g["colour"]), num_frame_per_fragment=1)
    assert np.array_equal(rough[0].color.cpu().numpy(), g["extract_colour"])


# ---------------------------------------------------------------------------------------------------------------- seams
@pytest.mark.parametrize("dims", [(5, 3, 63), (5, 3, 64), (5, 3, 65), (62, 32, 43), (1, 1, 1)])
def test_volume_shapes(tp, dims):
    c, th, wh = host_scene(tp, 3, dims, 4)
    t, w = integrate(tp, c, DEV)
    assert torch.equal(t.cpu(), th) and torch.equal(w.cpu(), wh)
    if dims != (1, 1, 1):
        assert int((wh > 0).sum()) > 0.2 * wh.numel()  # the frames do reach the volume
    got = tp.tsdf_surface(t, w, c["origin"], c["voxel"], 0.35, 0.0)
    want = tp.tsdf_surface(th, wh, c["origin"], c["voxel"], 0.35, 0.0)
    assert torch.equal(got.pos.cpu(), want.pos) and torch.equal(got.index.cpu(), want.index)
    assert got.status.tolist() == want.status.tolist()


def test_one_frame_and_no_frame(tp):
    c, th, wh = host_scene(tp, 5, (9, 7, 33), 1)
    t, w = integrate(tp, c, DEV)
    assert torch.equal(t.cpu(), th) and torch.equal(w.cpu(), wh) and float(wh.max()) == 1.0
    c0 = tc.random_scene(5, (9, 7, 33), 0)
    t, w = integrate(tp, c0, DEV)
    assert bool((t == 1).all()) and bool((w == 0).all())


@pytest.mark.parametrize("extra", [0, 1])
def test_frame_chunks_equal_single_frame_calls(tp, extra):
    F = tp.tsdf_max_frames() + extra
    c, th, wh = host_scene(tp, 7, (6, 5, 21), F)
    t, w = integrate(tp, c, DEV)  # one call: one launch per chunk of tsdf_max_frames() frames
    t1, w1 = fresh(c["dims"], DEV)
    d = dev(c["depths"])
    for f in range(F):
        tp.tsdf_integrate(t1, w1, c["origin"], c["voxel"], d[f:f + 1], c["K"], c["poses"][f:f + 1], c["weights"][f:f + 1],
                          depth_thresh=6)
    assert torch.equal(t, t1) and torch.equal(w, w1)
    assert torch.equal(t.cpu(), th) and torch.equal(w.cpu(), wh)
    assert float(wh.max()) > tp.tsdf_max_frames() * 0.5  # voxels that every frame reaches


def test_a_frame_that_sees_nothing(tp):
    c, _, _ = host_scene(tp, 9, (7, 6, 40), 3)
    blind = dict(c, depths=c["depths"].copy())
    blind["depths"][1] = 0
    t, w, _, _ = both_equal(tp, blind, "blind frame")
    two = dict(c, depths=c["depths"][[0, 2]], poses=c["poses"][[0, 2]], weights=c["weights"][[0, 2]])
    t2, w2 = integrate(tp, two, DEV)
    assert torch.equal(t, t2) and torch.equal(w, w2)
    away = dict(c, poses=c["poses"].copy())
    away["poses"][:, :3, :3] = np.diag([-1.0, 1.0, -1.0])  # every camera looks away from the volume
    t, w = integrate(tp, away, DEV)
    assert bool((t == 1).all()) and bool((w == 0).all())


def test_depth_element_types_agree(tp):
    c, th, wh = host_scene(tp, 11, (8, 9, 50), 5)
    metres = T.depth_metres_numpy(c["depths"], 1000.0, 6)
    for d in (dev(c["depths"]), dev(metres), dev(c["depths"].astype(np.int16)), dev(c["depths"].astype(np.int32))):
        t, w = integrate(tp, c, DEV, depths=d)
        assert torch.equal(t.cpu(), th) and torch.equal(w.cpu(), wh), d.dtype
    far = c["depths"].copy()
    far[:, ::2] = 7000  # beyond the threshold: zeroed in the load
    t, w = integrate(tp, c, DEV, depths=far)
    th2, wh2 = integrate(tp, c, "cpu", depths=far)
    assert torch.equal(t.cpu(), th2) and torch.equal(w.cpu(), wh2) and not torch.equal(wh2, wh)


def _surface_volume(kept, dims=(3, 7, 101)):
    """volumes whose surface is exactly the flat voxel ids `kept`"""
    n = int(np.prod(dims))
    t = np.ones(n, np.float32)
    w = np.zeros(n, np.float32)
    t[kept] = np.float32(0.1)
    w[kept] = 1.0
    # voxels that fail one half of the predicate each
    rest = np.setdiff1d(np.arange(n), kept)
    w[rest[::2]] = 1.0          # weight passes, |t| = 1 does not
    t[rest[1::2]] = np.float32(-0.2)  # |t| passes, weight 0 does not
    return torch.from_numpy(t.reshape(dims)), torch.from_numpy(w.reshape(dims))


@pytest.mark.parametrize("rows", ["tile-1", "tile", "tile+1", "none", "all", "random"])
def test_surface_rows_around_a_tile(tp, rows):
    tile = tp.tsdf_tile_rows()
    assert tile == tp.region_tile_rows()
    dims = (3, 7, 101)  # 2121 voxels: two full tiles and a part
    n = int(np.prod(dims))
    kept = {"tile-1": np.arange(tile - 1), "tile": np.arange(tile), "tile+1": np.arange(tile + 1),
            "none": np.zeros(0, np.int64), "all": np.arange(n),
            "random": np.sort(np.random.default_rng(1).choice(n, tile + 1, replace=False))}[rows]
    if rows in ("tile-1", "tile", "tile+1"):
        kept = kept + 5  # the list starts inside tile 0 and ends around the seam of tile 1
    t, w = _surface_volume(kept, dims)
    origin = np.array([0.1, -0.2, 0.3], np.float32)
    got = tp.tsdf_surface(t.to(DEV), w.to(DEV), origin, 0.07, 0.35, 0.0)
    want = tp.tsdf_surface(t, w, origin, 0.07, 0.35, 0.0)
    assert torch.equal(want.index, torch.from_numpy(kept.astype(np.int64)))
    assert torch.equal(got.index.cpu(), want.index) and torch.equal(got.pos.cpu(), want.pos)
    assert got.status.tolist() == [len(kept), 0]


def test_surface_capacity(tp):
    from torch_points3d_amd import _lib
    tile = tp.tsdf_tile_rows()
    kept = np.sort(np.random.default_rng(2).choice(2121, tile + 37, replace=False))
    t, w = _surface_volume(kept)
    origin = np.array([0.1, -0.2, 0.3], np.float32)
    td, wd = t.to(DEV), w.to(DEV)
    full = tp.tsdf_surface(td, wd, origin, 0.07, 0.35, 0.0)  # capacity None
    n = len(kept)
    assert full.pos.shape == (n, 3) and full.status.tolist() == [n, 0]
    exact = tp.tsdf_surface(td, wd, origin, 0.07, 0.35, 0.0, capacity=n)
    assert exact.status.tolist() == [n, 0] and torch.equal(exact.pos, full.pos) and torch.equal(exact.index, full.index)
    small = tp.tsdf_surface(td, wd, origin, 0.07, 0.35, 0.0, capacity=tile - 3)
    assert small.status.tolist() == [n, 1] and small.pos.shape == (tile - 3, 3)
    assert torch.equal(small.pos, full.pos[:tile - 3]) and torch.equal(small.index, full.index[:tile - 3])
    host = tp.tsdf_surface(t, w, origin, 0.07, 0.35, 0.0, capacity=tile - 3)
    assert host.status.tolist() == [n, 1] and torch.equal(small.pos.cpu(), host.pos)
    # nothing is written past the capacity: buffers of the full size, filled with a mark, emitted with a smaller bound
    cap = tile - 3
    pos = torch.full((n, 3), -7.0, dtype=torch.float64, device=DEV)
    index = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    status = torch.empty(2, dtype=torch.int64, device=DEV)
    nbytes = _lib.load().tp3d_tsdf_surface_workspace_bytes(2121)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))
    _lib.call("tp3d_tsdf_surface_count", td.data_ptr(), wd.data_ptr(), 2121, 0.35, 0.0, cap, status.data_ptr(), ws.data_ptr(),
              nbytes, s)
    _lib.call("tp3d_tsdf_surface_emit", td.data_ptr(), wd.data_ptr(), 3, 7, 101, float(origin[0]), float(origin[1]),
              float(origin[2]), 0.07, 0.35, 0.0, cap, pos.data_ptr(), index.data_ptr(), ws.data_ptr(), nbytes, s)
    assert status.tolist() == [n, 1]
    assert torch.equal(pos[:cap], full.pos[:cap]) and bool((pos[cap:] == -7.0).all()) and bool((index[cap:] == -7).all())


@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 33, 37), (2, 32, 32)])
def test_unproject_shapes_and_capacity(tp, shape):
    F, H, W = shape  # 64 pixels; 1221 = a tile and a part; 1024 = one tile exactly
    rng = np.random.default_rng(4)
    raw = rng.integers(300, 7000, shape).astype(np.uint16)  # some beyond 6 m
    raw[rng.random(shape) < 0.2] = 0
    poses = tc.random_scene(4, (2, 2, 2), F)["poses"]
    K = np.array([[31.3, 0, 0.5 * W - 0.2], [0, 30.7, 0.5 * H + 0.1], [0, 0, 1.0]])
    want = tp.depth_unproject(host_depth(raw), K, poses)
    got = tp.depth_unproject(dev(raw), K, poses)
    n = int(want.status[0])
    assert 0 < n < F * H * W
    assert torch.equal(got.start.cpu(), want.start) and torch.equal(got.pixel.cpu(), want.pixel)
    assert torch.equal(got.pos.cpu(), want.pos) and got.status.tolist() == [n, 0]
    small = tp.depth_unproject(dev(raw), K, poses, capacity=n - 1)
    assert small.status.tolist() == [n, 1] and torch.equal(small.pos.cpu(), want.pos[:n - 1])
    assert torch.equal(small.start.cpu(), want.start)
    empty = tp.depth_unproject(dev(np.zeros(shape, np.uint16)), K, poses)
    assert empty.pos.shape == (0, 3) and empty.start.tolist() == [0] * (F + 1)
    ones = tp.depth_unproject(dev(np.full(shape, 1500, np.uint16)), K, poses)
    assert ones.pos.shape == (F * H * W, 3) and torch.equal(ones.pixel.cpu(), torch.arange(F * H * W))


# ------------------------------------------------------------------------------------------------------------- behaviour
def test_repeats_streams_and_inputs(tp):
    c, th, wh = host_scene(tp, 13, (20, 9, 70), 6)
    d = dev(c["depths"])
    before = d.view(torch.int16).clone()
    t, w = integrate(tp, c, DEV, depths=d)
    t2, w2 = integrate(tp, c, DEV, depths=d)
    assert torch.equal(t, t2) and torch.equal(w, w2)  # bit-equal repeats
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t3, w3 = integrate(tp, c, DEV, depths=d)
        s3 = tp.tsdf_surface(t3, w3, c["origin"], c["voxel"], 0.35, 0.0)
        u3 = tp.depth_unproject(d, c["K"], c["poses"])
    side.synchronize()
    assert torch.equal(t3.cpu(), th) and torch.equal(w3.cpu(), wh)
    s1 = tp.tsdf_surface(t, w, c["origin"], c["voxel"], 0.35, 0.0)
    u1 = tp.depth_unproject(d, c["K"], c["poses"])
    assert torch.equal(s1.pos, s3.pos) and torch.equal(s1.index, s3.index) and s1.pos.shape[0] > 0
    assert torch.equal(u1.pos, u3.pos) and torch.equal(u1.pixel, u3.pixel)
    assert torch.equal(d.view(torch.int16), before)  # the frames are never modified
    assert torch.equal(t, t2) and torch.equal(t.cpu(), th)  # nor the volumes by surface extraction


def test_integrate_frames_allocates_nothing_of_volume_size(tp):
    vs = 0.0078125
    bnds = np.array([[-0.5, 0.5], [-0.5, 0.5], [0.25, 0.75]])
    vol = T.TSDFVolume(bnds, vs, device=DEV)  # 128 x 128 x 64 voxels: 4 MiB per array
    assert vol.get_volume()[0].numel() * 4 == 4 << 20
    c = tc.random_scene(15, (128, 128, 64), 5, voxel=vs)
    for d in (dev(c["depths"]), dev(c["depths"].astype(np.float64) / 1000.0)):
        tp.tsdf_integrate(*fresh((2, 2, 2), DEV), c["origin"], vs, d, c["K"], c["poses"], 1.0)  # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()  # the volumes and the depth stack are resident
        vol.integrate_frames(d, c["K"], c["poses"], c["weights"], depth_thresh=6)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base <= 1 << 20
    assert float(vol.get_volume()[1].max()) > 0
