"""TSDF fusion on the host: the float64 numpy definition (torch_points3d_amd/tsdf.py) against what the reference's own
fusion.py / utils.py computed (tests/golden/tsdf.npz, README_tsdf.md) and against hand-derived cases (tsdf_cases.py)."""
import numpy as np
import pytest
import torch

import tsdf_cases as tc
from torch_points3d_amd import torchpoints as tp, tsdf as T


def _integrate_case(c, upto=None):
    t = torch.ones(c["dims"], dtype=torch.float32)
    w = torch.zeros(c["dims"], dtype=torch.float32)
    F = c["depths"].shape[0] if upto is None else upto
    tp.tsdf_integrate(t, w, c["origin"], c["voxel"], torch.from_numpy(c["depths"][:F]), c["K"], c["poses"][:F],
                      c["weights"][:F], depth_thresh=6)
    return t.numpy(), w.numpy()


@pytest.mark.parametrize("case", tc.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(case):
    t, w = _integrate_case(case)
    assert np.array_equal(w, case["weight"]), (w, case["weight"])
    assert np.array_equal(t, case["tsdf"]), (t, case["tsdf"])


def test_half_even_reads_columns_0_2_2():
    case = [c for c in tc.hand_cases() if c["name"] == "half_even"][0]
    t, _ = _integrate_case(case)
    row = case["depths"][0, 0]
    got = [float(t[i, 0, 4]) for i in (1, 3, 5)]
    assert got == [float(np.float32((row[c] - 1.0) / 1.25)) for c in (0, 2, 2)]
    assert got != [float(np.float32((row[c] - 1.0) / 1.25)) for c in (1, 2, 3)]  # what roundf would read


def test_running_mean_steps():
    case = [c for c in tc.hand_cases() if c["name"] == "running_mean"][0]
    for n, (t_want, w_want) in enumerate(case["steps"], 1):
        t, w = _integrate_case(case, n)
        assert t[0, 0, 0] == t_want and w[0, 0, 0] == np.float32(w_want)


def test_volume_against_reference_frame_by_frame():
    g = tc.golden()
    vol = T.TSDFVolume(g["vol_bnds"], float(g["vol_voxel"]))
    assert np.array_equal(vol._vol_dim, g["vol_dim"]) and np.array_equal(vol._vol_origin, g["vol_origin"])
    assert vol._vol_origin.dtype == np.float32
    for f in range(g["vol_depths"].shape[0]):
        vol.integrate(g["vol_depths"][f], g["vol_K"], g["vol_poses"][f], obs_weight=float(g["vol_weights"][f]), depth_thresh=6)
        t, w = vol.get_volume()
        tc.assert_golden("vol_tsdf[%d]" % f, t, g["vol_tsdf"][f])
        tc.assert_golden("vol_weight[%d]" % f, w, g["vol_weight"][f])
    tc.assert_golden("vol_cloud", vol.get_point_cloud(0.35, 0.0), g["vol_cloud"])
    assert g["vol_cloud"].shape[0] > 100 and int(g["vol_touched"]) > 10000


def test_integrate_frames_equals_single_frames_and_depth_types():
    g = tc.golden()
    a = T.TSDFVolume(g["vol_bnds"], float(g["vol_voxel"]))
    a.integrate_frames(g["vol_depths"], g["vol_K"], g["vol_poses"], g["vol_weights"], depth_thresh=6)
    assert np.array_equal(a.get_volume()[0], g["vol_tsdf"][-1]) and np.array_equal(a.get_volume()[1], g["vol_weight"][-1])
    metres = T.depth_metres_numpy(g["vol_depths"], 1000.0, 6)
    for depths in (torch.from_numpy(metres), torch.from_numpy(g["vol_depths"].astype(np.int32)),
                   torch.from_numpy(g["vol_depths"].astype(np.int16))):
        b = T.TSDFVolume(g["vol_bnds"], float(g["vol_voxel"]))
        b.integrate_frames(depths, g["vol_K"], g["vol_poses"], g["vol_weights"], depth_thresh=6)
        assert np.array_equal(b.get_volume()[0], g["vol_tsdf"][-1]) and np.array_equal(b.get_volume()[1], g["vol_weight"][-1])


def test_frustum_and_bounds():
    g = tc.golden()
    F = g["vol_depths"].shape[0]
    for f in range(F):
        m = T.depth_metres_numpy(g["vol_depths"][f], 1000.0, 6)
        tc.assert_golden("frustum[%d]" % f, T.get_view_frustum(m, g["vol_K"], g["vol_poses"][f]), g["frustum"][f])
    free = T.get_3D_bound(g["vol_depths"], g["vol_K"], g["vol_poses"], 6, limit_size=600, voxel_size=0.05)
    trim = T.get_3D_bound(torch.from_numpy(g["vol_depths"].astype(np.int32)), g["vol_K"], g["vol_poses"], 6,
                          limit_size=int(g["bound_limit"]), voxel_size=0.05)
    tc.assert_golden("bound_free", free, g["bound_free"])
    tc.assert_golden("bound_trim", trim, g["bound_trim"])
    cut = np.abs(g["bound_free"] - g["bound_trim"]).max(1) > 1e-6
    assert cut.sum() == 1  # the limit trims exactly one axis


def test_raw_depth_is_divided_not_multiplied_by_a_reciprocal():
    raw = np.arange(0, 65536, dtype=np.int32)
    assert np.array_equal(T.true_divide(torch.from_numpy(raw), 1000.0).numpy(), raw.astype(np.float64) / 1000.0)
    assert not np.array_equal(raw.astype(np.float64) * (1.0 / 1000.0), raw.astype(np.float64) / 1000.0)
    g = tc.golden()
    want = T.depth_metres_numpy(g["vol_depths"], 1000.0, 6).reshape(g["vol_depths"].shape[0], -1).max(1)
    assert np.array_equal(T.frame_max_depth(torch.from_numpy(g["vol_depths"].astype(np.int32)), 6), want)
    assert np.array_equal(T.frame_max_depth(g["vol_depths"], 6), want)


def test_unprojection_with_colour():
    g = tc.golden()
    d = torch.from_numpy(g["vol_depths"].astype(np.int32))
    one = tp.depth_unproject(d[:1], g["vol_K"])
    tc.assert_golden("extract_pos", one.pos.numpy(), g["extract_pos"])
    assert np.array_equal(g["colour"][0].reshape(-1, 3)[one.pixel.numpy()], g["extract_colour"])
    res = tp.depth_unproject(d, g["vol_K"], g["vol_poses"])
    assert np.array_equal(res.start.numpy(), g["world_start"])
    tc.assert_golden("world_pos", res.pos.numpy(), g["world_pos"])
    assert res.pixel.dtype == torch.int64 and bool((res.pixel[1:] > res.pixel[:-1]).all())
    frags = T.rgbd2fragment_rough(g["vol_depths"], g["vol_K"], g["vol_poses"], colors=g["colour"], num_frame_per_fragment=2)
    assert len(frags) == 2 and frags[0].pos.shape[0] == int(g["world_start"][2])
    tc.assert_golden("world_pos", frags[1].pos.numpy(), g["world_pos"][g["world_start"][2]:g["world_start"][4]])
    assert np.array_equal(frags[0].color.numpy(), g["colour"].reshape(-1, 3)[res.pixel.numpy()[:int(g["world_start"][2])]])


def test_fragments_and_their_windows():
    g = tc.golden()
    assert T.fragment_windows(11, 5) == [(0, 5), (5, 10), (10, 11)]  # the last window is shorter
    assert T.fragment_windows(10, 5) == [(0, 5), (5, 10)] and T.fragment_windows(3, 5) == [(0, 3)]
    frags = T.rgbd2fragment_fine(g["frag_depths"], g["vol_K"], g["frag_poses"], num_frame_per_fragment=5,
                                 voxel_size=float(g["frag_voxel"]), depth_thresh=6, limit_size=int(g["frag_limit"]))
    assert len(frags) == int(g["frag_count"]) == 2
    for i, f in enumerate(frags):
        assert f.pos.dtype == torch.float64
        tc.assert_golden("fragment[%d]" % i, f.pos.numpy(), g["fragment_%d" % i])
    seen = []
    T.rgbd2fragment_fine(g["frag_depths"], g["vol_K"], g["frag_poses"], num_frame_per_fragment=5,
                         voxel_size=float(g["frag_voxel"]), limit_size=int(g["frag_limit"]),
                         pre_transform=lambda d: seen.append(d.pos.shape[0]) or d)
    assert seen == [g["fragment_0"].shape[0], g["fragment_1"].shape[0]]


def test_surface_capacity_and_mesh():
    g = tc.golden()
    t, w = torch.from_numpy(g["vol_tsdf"][-1]), torch.from_numpy(g["vol_weight"][-1])
    full = tp.tsdf_surface(t, w, g["vol_origin"], 0.05, 0.35, 0.0)
    T_ = full.pos.shape[0]
    assert full.status.tolist() == [T_, 0] and np.array_equal(full.pos.numpy(), g["vol_cloud"])
    ijk = np.stack(np.unravel_index(full.index.numpy(), t.shape), 1)
    assert np.array_equal(ijk.astype(np.float64) * 0.05 + g["vol_origin"].astype(np.float64), g["vol_cloud"])
    small = tp.tsdf_surface(t, w, g["vol_origin"], 0.05, 0.35, 0.0, capacity=T_ - 3)
    assert small.status.tolist() == [T_, 1] and torch.equal(small.pos, full.pos[:T_ - 3])
    big = tp.tsdf_surface(t, w, g["vol_origin"], 0.05, 0.35, 0.0, capacity=T_ + 2)
    assert big.status.tolist() == [T_, 0] and torch.equal(big.pos[:T_], full.pos) and not big.pos[T_:].any()
    with pytest.raises(NotImplementedError, match="marching cubes"):
        T.TSDFVolume(g["vol_bnds"], 0.05).get_mesh()


def test_header_declares_the_entry_points():
    from torch_points3d_amd import _lib
    for name in ("tp3d_tsdf_integrate", "tp3d_tsdf_surface_count", "tp3d_tsdf_surface_emit", "tp3d_depth_unproject_count",
                 "tp3d_depth_unproject_emit", "tp3d_tsdf_tile_rows"):
        assert name in _lib.FUNCTIONS
    assert tp.tsdf_max_frames() == _lib.CONSTANTS["TP3D_TSDF_MAX_FRAMES"] == 64
