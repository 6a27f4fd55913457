"""The host side of FPFH: the float64 numpy restatement of torch_points3d_amd/fpfh.py (the definition the kernels of
csrc/fpfh.hip are held to by tests/test_gpu_fpfh.py, and what CPU tensors take) against answers derived by hand
(tests/fpfh_ref.py), a brute-force search, the atan2 form of the angle bin, and the C side's edge table."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fpfh_ref as ref
from torch_points3d_amd import _lib
from torch_points3d_amd import fpfh as F
from torch_points3d_amd import registration as reg
from torch_points3d_amd import torchpoints as tp
from torch_points3d_amd.dense import Data


def test_header_declares_the_entry_points_at_abi_39():
    for name in ("tp3d_fpfh_edge_table", "tp3d_hybrid_search_workspace_bytes", "tp3d_hybrid_search_f32",
                 "tp3d_fpfh_normals_f32", "tp3d_spfh_counts_f32", "tp3d_fpfh_f32"):
        assert name in _lib.FUNCTIONS
    assert _lib.ABI_VERSION == 39
    assert _lib.CONSTANTS["TP3D_FPFH_MAX_NN"] == 256


def test_config_and_defaults_are_the_scripts():
    assert F.fpfh_config() == dict(radius=0.3, max_nn=256, radius_normal=0.093, max_nn_normal=17)
    f = F.FPFH()
    assert (f.radius, f.max_nn, f.radius_normal, f.max_nn_normal) == (0.3, 128, 0.3, 17)


# ------------------------------------------------------------------------------------------------------------- angle bin
def test_edge_table_is_the_edges():
    for e, (c, s) in enumerate(F.EDGE_TABLE, 1):
        t = -math.pi + 2 * math.pi * e / 11
        assert abs(c - math.cos(t)) <= 2e-16 and abs(s - math.sin(t)) <= 2e-16


def test_edge_table_equals_the_c_table():
    table = (ctypes.c_double * 20)()
    assert _lib.load().tp3d_fpfh_edge_table(ctypes.cast(table, ctypes.c_void_p)) == 0
    assert [tuple(table[2 * e:2 * e + 2]) for e in range(10)] == [tuple(r) for r in F.EDGE_TABLE]


def test_angle_bin_equals_the_atan2_form():
    g = np.random.default_rng(11)
    v = g.standard_normal((1000000, 2)) * np.exp(g.uniform(-20, 20, (1000000, 1)))
    want = np.clip(np.floor(11 * (np.arctan2(v[:, 1], v[:, 0]) + np.pi) / (2 * np.pi)), 0, 10).astype(np.int64)
    assert np.array_equal(F.angle_bin(v[:, 0], v[:, 1]), want)


def test_angle_bin_on_the_axes():
    # angle -pi/2, 0, pi/2 lie inside bins 2, 5, 8; the angle pi gives floor(11) = 11, clamped to 10, whatever the sign of
    # the zero sine; (0, 0) is bin 5 by rule
    assert F.angle_bin([0.0, 1.0, 0.0, -1.0, -1.0, 0.0], [-1.0, 0.0, 1.0, 0.0, -0.0, 0.0]).tolist() == [2, 5, 8, 10, 10, 5]


# ---------------------------------------------------------------------------------------------------------------- search
@pytest.mark.parametrize("max_nn", [1, 3, 17, 300])
def test_search_equals_brute_force(max_nn):
    pos, batch = ref.batched()
    pos, batch = np.concatenate([pos[:150], pos[600:750], pos[1200:]]), np.concatenate([batch[:150], batch[600:750], batch[1200:]])
    for radius in (0.06, 0.2):
        got = F.hybrid_search_numpy(pos, pos, radius, max_nn, batch, batch)
        want = ref.brute_search(pos, pos, radius, max_nn, batch, batch)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    assert (got[2] == max_nn).any() or max_nn == 300
    assert (got[0][:, 0] == np.arange(len(pos))).all()  # slot 0 is the point itself


def test_search_pair_on_the_radius_and_foreign_queries():
    p, r = ref.on_radius_pair()
    idx, d2, count = F.hybrid_search_numpy(p, p, r, 4)
    # row 0 sees itself and row 2, not row 1 (d2 == r2); row 1 itself and row 2; row 2 all three; row 3 itself
    assert idx[0].tolist() == [0, 2, -1, -1] and count.tolist() == [2, 2, 3, 1]
    assert d2[0, 1] < np.float32(r) * np.float32(r) and d2[0, 2] == -1
    # other queries than the support, one of them of a cloud without support rows
    q = np.array([[0.1, 0, 0], [0.1, 0, 0]], np.float32)
    got = F.hybrid_search_numpy(p, q, r, 3, np.zeros(4, np.int64), np.array([0, 1]))
    want = ref.brute_search(p, q, r, 3, np.zeros(4, np.int64), np.array([0, 1]))
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[2].tolist() == [3, 0]
    out = tp.hybrid_search(torch.from_numpy(p), torch.from_numpy(p), r, 4)
    assert torch.equal(out[0], torch.from_numpy(idx)) and out[2].dtype == torch.int32
    with pytest.raises(ValueError):
        tp.hybrid_search(torch.from_numpy(p), torch.from_numpy(p), r, 257)


# --------------------------------------------------------------------------------------------------------- known answers
def _plane_tables(radius=0.15, max_nn=16):
    p = ref.plane()
    idx, _, count = F.hybrid_search_numpy(p, p, radius, max_nn)
    n = np.tile(np.array([0, 0, 1], np.float32), (len(p), 1))
    return p, n, idx, count


def test_pair_function_on_a_plane_gives_the_centre_bins():
    assert F.pair_bins([0, 0, 0], [0, 0, 1], [0.3, 0.4, 0], [0, 0, 1]).tolist() == [5, 5, 5]


def test_plane_known_answer():
    p, n, idx, count = _plane_tables()
    assert count.min() >= 2 and (count == 16).any() and (count < 16).any()  # rows cut by max_nn, rows cut by the radius
    counts = F.spfh_counts_numpy(p, n, idx, count)
    want = np.zeros((len(p), 33), np.int64)
    want[:, ref.PLANE_BINS] = (count - 1)[:, None]
    assert np.array_equal(counts, want)
    spfh = F.spfh_values(counts, count)
    assert np.abs(spfh[:, ref.PLANE_BINS] - 100.0).max() <= 1e-11 and spfh.sum() <= 300.0 * len(p) * (1 + 1e-12)
    out = F.fpfh_numpy(p, idx, count, counts)
    want = np.zeros((len(p), 33))
    want[:, ref.PLANE_BINS] = 200.0
    assert np.abs(out - want).max() <= 1e-11
    # and the normals of the plane: the smallest eigenvalue is exactly 0 along z
    nn = F.estimate_normals_numpy(p, idx, count)
    assert np.array_equal(nn, n)
    down = F.estimate_normals_numpy(p, idx, count, viewpoint=np.array([0.5, 0.5, -3.0]))
    assert np.array_equal(down, -n)


# ------------------------------------------------------------------------------------------------------- degenerate cases
def test_pair_degenerate_cases():
    # a duplicate point: d == 0, the centre bins
    assert F.pair_bins([1, 2, 3], [0, 0, 1], [1, 2, 3], [1, 0, 0]).tolist() == [5, 5, 5]
    # dp parallel to n1 (and n2 = n1: no swap): v = dp x n1 = 0, features (0, 0, 0) -- f2 = a1 = 1 is dropped as well
    assert F.pair_bins([0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 1]).tolist() == [5, 5, 5]
    # |a1| < |a2|: the normals swap and dp turns round: n1' = (1, 0, 0), dp' = (-1, 0, 0), v = 0 again
    assert F.pair_bins([0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 0]).tolist() == [5, 5, 5]
    # a hand-worked general pair: p1 = 0, n1 = z, p2 = (1, 0, 1) / sqrt 2, n2 = x.  a1 = a2 = 1 / sqrt 2, no swap, f2 = a1
    # -> floor(5.5 * 1.707) = 9; v = dp x n1 = (0, -1, 0) / |.|, f1 = v . n2 = 0 -> 5; w = n1 x v = (1, 0, 0), angle =
    # atan2(w . n2, n1 . n2) = atan2(1, 0) = pi / 2 -> floor(11 * 0.75) = 8
    h = math.sqrt(0.5)
    assert F.pair_bins([0, 0, 0], [0, 0, 1], [h, 0, h], [1, 0, 0]).tolist() == [8, 5, 9]


def test_small_neighbourhoods_and_duplicates():
    # rows 0, 1 coincide; row 2 is 0.1 away from them; row 3 has only itself; rows 4, 5 a pair
    p = np.array([[0, 0, 0], [0, 0, 0], [0.1, 0, 0], [5, 5, 5], [9, 9, 9], [9, 9.1, 9]], np.float32)
    idx, d2, count = F.hybrid_search_numpy(p, p, 0.2, 8)
    assert count.tolist() == [3, 3, 3, 1, 2, 2]
    assert idx[0, :3].tolist() == [0, 1, 2] and idx[1, :3].tolist() == [0, 1, 2]  # slot 0 of row 1: its lower twin
    n = F.estimate_normals_numpy(p, idx, count)
    assert np.array_equal(n[3:], np.tile(np.array([0, 0, 1], np.float32), (3, 1)))  # k < 3
    n = np.tile(np.array([0, 0, 1], np.float32), (6, 1))
    counts = F.spfh_counts_numpy(p, n, idx, count)
    assert counts.sum(1).tolist() == [6, 6, 6, 0, 3, 3]  # k - 1 slots, three blocks each; k = 1: a zero row
    # row 0: slot 1 is its twin (d == 0: centre bins), slot 2 a plane pair (centre bins too)
    assert counts[0, list(ref.PLANE_BINS)].tolist() == [2, 2, 2]
    out = F.fpfh_numpy(p, idx, count, counts)
    assert np.array_equal(out[3], np.zeros(33))
    # row 0: the twin is skipped (d2 == 0), one term spfh_2 / 0.01 is left: 100 after normalising, plus its own 100
    want = np.zeros(33)
    want[list(ref.PLANE_BINS)] = 200.0
    assert np.abs(out[0] - want).max() <= 1e-11
    # row 1 differs from row 0 in nothing but its slot 0 (row 0, not itself): slot 1 is then ITSELF, d2 == 0, skipped
    assert np.array_equal(out[1], out[0])
    assert np.abs(out[4] - want).max() <= 1e-11  # k = 2: the one neighbour's SPFH, plus its own
    sub = F.fpfh_numpy(p, idx, count, counts, rows=np.array([4, 0]))
    assert np.array_equal(sub, out[[4, 0]])


def test_normals_against_eigh():
    pos, batch = ref.batched()
    idx, _, count = F.hybrid_search_numpy(pos, pos, 0.3, 17, batch, batch)
    n = F.estimate_normals_numpy(pos, idx, count).astype(np.float64)
    lam, vec = np.linalg.eigh(F.neighbourhood_covariance(pos, idx, count)[:1200])
    assert ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min() >= 1e-3
    assert (1.0 - np.abs((n[:1200] * vec[:, :, 0]).sum(1))).max() <= 1e-7  # (the fp32 rounding of the result)
    top = np.abs(n).argmax(1)
    assert (n[np.arange(len(n)), top] > 0).all()
    assert np.array_equal(n[1200:], np.tile([0.0, 0.0, 1.0], (3, 1)))


# ------------------------------------------------------------------------------------------------------------------ class
def test_class_on_cpu_tensors():
    pos, batch = ref.batched()
    keep = np.r_[0:120, 600:720, 1200:1203]
    pos, batch = torch.from_numpy(pos[keep]), torch.from_numpy(batch[keep])
    f = F.FPFH(radius=0.25, max_nn=20, radius_normal=0.25, max_nn_normal=9)
    full = f(Data(pos=pos, batch=batch))
    assert full.shape == (243, 33) and full.dtype == torch.float32
    kp = torch.tensor([200, 3, 3, 242])
    assert torch.equal(f(Data(pos=pos, batch=batch, keypoints=kp)), full[kp])
    # by hand from the pieces
    idx, _, count = F.hybrid_search_numpy(pos.numpy(), pos.numpy(), 0.25, 20, batch.numpy(), batch.numpy())
    idn, _, cn = F.hybrid_search_numpy(pos.numpy(), pos.numpy(), 0.25, 9, batch.numpy(), batch.numpy())
    n = F.estimate_normals_numpy(pos.numpy(), idn, cn)
    want = F.fpfh_numpy(pos.numpy(), idx, count, F.spfh_counts_numpy(pos.numpy(), n, idx, count))
    assert np.array_equal(full.numpy(), want.astype(np.float32))
    # every block of a row with neighbours sums to 200 (100 of its own SPFH + 100 of the normalised sum); the lone cloud
    # of one point is a zero row and the pair cloud holds the plane answer
    sums = full.double().reshape(-1, 3, 11).sum(2)
    assert torch.allclose(sums[:240], torch.full((240, 3), 200.0, dtype=torch.float64), atol=1e-3)
    assert torch.equal(full[242], torch.zeros(33))
    # the clouds do not see each other: the sheet alone gives the same rows
    alone = f(Data(pos=pos[:120]))
    assert torch.equal(alone, full[:120])
    # a viewpoint per cloud
    g = F.FPFH(radius=0.25, max_nn=20, radius_normal=0.25, max_nn_normal=9, viewpoint=torch.tensor([[0.5, 0.5, 4.0]] * 4))
    assert g(Data(pos=pos, batch=batch)).shape == (243, 33)


# --------------------------------------------------------------------------------------------------------------- matching
def test_matches_and_recall_on_cpu():
    g = torch.Generator().manual_seed(3)
    feat_t = torch.randn(40, 33, generator=g)
    perm = torch.randperm(40, generator=g)
    feat_s = feat_t[perm] + 1e-3 * torch.randn(40, 33, generator=g)  # source row r is target row perm[r]
    kp_t = torch.randn(40, 3, generator=g)
    R, t = ref.rigid()
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = torch.from_numpy(R), torch.from_numpy(t)
    kp_s = (kp_t.double() @ T[:3, :3].T + T[:3, 3])[perm].float()  # kp_s[r] = T kp_t[perm[r]]
    ks, kt = reg.compute_matches(feat_s, feat_t, kp_s, kp_t)
    assert torch.equal(kt, kp_t) and torch.equal(ks, kp_s[torch.argsort(perm)])
    ks2, kt2 = reg.compute_matches(feat_s, feat_t, kp_s, kp_t, sym=True)
    assert torch.equal(ks2, ks) and torch.equal(kt2, kt)
    d = reg.compute_dists(ks, kt, T.float())
    assert d.max() < 1e-5
    assert reg.compute_mean_correct_matches(d, [0.1, 0.0]).tolist() == [1.0, 0.0]
    bad = (feat_s.flip(0), feat_t, kp_s, kp_t, T.float())  # wrong features: hardly any correct match
    recall, frac = reg.feature_match_recall([(feat_s, feat_t, kp_s, kp_t, T.float()), bad], [0.1], [0.5])
    assert frac[0, 0] == 1.0 and frac[1, 0] < 0.5 and recall.tolist() == [[0.5]]
