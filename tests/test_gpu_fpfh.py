"""FPFH on the GPU (csrc/fpfh.hip; torchpoints.hybrid_search / estimate_normals / spfh_counts / fpfh; fpfh.FPFH) against
the float64 numpy restatement of torch_points3d_amd/fpfh.py, which tests/test_fpfh_cpu.py holds to hand-derived answers.

Search, SPFH counts: torch.equal (fp32 distances in one evaluation order; integer counts from +, -, *, /, sqrt in double
with contraction off).  Normals: 1 - |n . n_ref| <= 1e-12 against numpy.linalg.eigh of the restated covariance, on the
points whose relative gap (l1 - l0) / l2 is >= 1e-3 (at most 1 % may be excluded; none is here).  The device's normal is
its double result rounded once to fp32, so its LENGTH is 1 +- 6e-8: the direction is compared, the fp32 vector normalised
in double (a componentwise error of 2^-24 turns the direction by <= 1.1e-7 rad: 1 - cos <= 6e-15).  FPFH: 1e-11 on the
float64 output (a sum of at most 255 non-negative double terms is within 255 * 2^-53 = 2.8e-14 relative, values <= 200),
the float32 output its one rounding."""
import numpy as np
import numpy.testing as npt
import pytest
import torch

import fpfh_ref as ref
from torch_points3d_amd import fpfh as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_NN = [1, 2, 3, 17, 63, 64, 65, 128, 129, 200, 256]


@pytest.fixture(scope="module")
def tp():
    from torch_points3d_amd import torchpoints
    return torchpoints


@pytest.fixture(scope="module")
def reg():
    from torch_points3d_amd import registration
    return registration


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def search_equal(tp, x, y, radius, max_nn, bx, by, what):
    got = tp.hybrid_search(dev(x), dev(y), radius, max_nn, dev(bx), dev(by))
    want = F.hybrid_search_numpy(x, y, radius, max_nn, bx, by)
    for name, g, w in zip(("idx", "dist2", "count"), got, want):
        assert g.dtype == torch.from_numpy(w).dtype, (what, name)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)
    return got, want


_shared = {}


def tables(tp, radius=0.25, max_nn=40, max_nn_normal=17):
    """the batched input with its neighbour tables and teacher-forced normals: computed once, never changed"""
    key = (radius, max_nn, max_nn_normal)
    if key not in _shared:
        pos, batch = ref.batched()
        idx, d2, count = F.hybrid_search_numpy(pos, pos, radius, max_nn, batch, batch)
        idn, _, cn = F.hybrid_search_numpy(pos, pos, radius, max_nn_normal, batch, batch)
        normals = F.estimate_normals_numpy(pos, idn, cn)
        counts = F.spfh_counts_numpy(pos, normals, idx, count)
        _shared[key] = dict(pos=pos, batch=batch, idx=idx, count=count, idn=idn, cn=cn, normals=normals, counts=counts,
                            out=F.fpfh_numpy(pos, idx, count, counts))
    return _shared[key]


# ------------------------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("max_nn", MAX_NN)
def test_search_equals_numpy(tp, max_nn):
    pos, batch = ref.batched()
    # 0.04: most rows cut by the radius, some hold only themselves; 0.12: both cuts; 0.45: the sheet's balls hold up to ~380
    cut_r = cut_k = lone = False
    for radius in (0.04, 0.12, 0.45):
        _, (idx, d2, count) = search_equal(tp, pos, pos, radius, max_nn, batch, batch, "r %g k %d" % (radius, max_nn))
        assert np.array_equal(idx[:, 0], np.arange(len(pos)))
        cut_r, cut_k, lone = cut_r or (count < max_nn).any(), cut_k or (count == max_nn).any(), lone or (count == 1).any()
        if max_nn <= 128:  # the rows of knn cut at the radius
            kidx, kd2 = tp.knn(max_nn, dev(pos), dev(pos), dev(batch), dev(batch))
            inside = (kd2 < float(np.float32(radius) * np.float32(radius))) & (kidx >= 0)
            assert torch.equal(torch.where(inside, kidx, torch.full_like(kidx, -1)).cpu(), torch.from_numpy(idx).long())
            assert torch.equal(torch.where(inside, kd2, torch.full_like(kd2, -1.0)).cpu(), torch.from_numpy(d2))
    assert cut_k and lone and (cut_r or max_nn == 1)


@pytest.mark.parametrize("max_nn", [17, 256])
def test_search_in_balls_beyond_the_candidate_buffer(tp, max_nn):
    # 3000 points in the unit cube, radius 0.6: the balls hold up to ~2700 candidates, more than the 1024 slots a wave keeps,
    # so the buffer is cut at its max_nn-th distance once or more per query
    pos = np.random.default_rng(8).random((3000, 3)).astype(np.float32)
    _, (_, _, count) = search_equal(tp, pos, pos, 0.6, max_nn, None, None, "dense ball")
    assert (count == max_nn).all()


@pytest.mark.parametrize("max_nn", [5, 256])
def test_search_with_more_equal_distances_than_the_buffer_holds(tp, max_nn):
    # 1100 coincident rows among 400 others, and a lattice whose distances take few values: cutting the full buffer at its
    # max_nn-th distance wins no room (every pair lies AT it), so the cut must fall back on the indices
    g = np.random.default_rng(10)
    pos = g.random((1500, 3)).astype(np.float32)
    pos[g.permutation(1500)[:1100]] = np.float32(0.5)
    _, (idx, d2, _) = search_equal(tp, pos, pos, 0.4, max_nn, None, None, "coincident rows")
    twins = np.nonzero((pos == np.float32(0.5)).all(1))[0]
    assert np.array_equal(idx[twins[-1], :max_nn], twins[:max_nn]) and (d2[twins[-1], :max_nn] == 0).all()
    lattice = np.stack(np.meshgrid(*[np.arange(12, dtype=np.float32) / 8] * 3, indexing="ij"), -1).reshape(-1, 3)
    search_equal(tp, lattice, lattice, 1.0, max_nn, None, None, "lattice")


def test_search_foreign_queries_empty_rows_and_the_radius_itself(tp):
    pos, batch = ref.batched()
    g = np.random.default_rng(9)
    q = np.concatenate([g.random((200, 3)), g.random((100, 3)) + 3.0, g.random((50, 3))]).astype(np.float32)
    bq = np.concatenate([np.zeros(200, np.int64), np.ones(100, np.int64), np.full(50, 7, np.int64)])  # cloud 7: no support
    _, (_, _, count) = search_equal(tp, pos, q, 0.1, 20, batch, bq, "foreign queries")
    assert (count[:200] > 0).any() and (count[200:] == 0).all()
    p, r = ref.on_radius_pair()
    _, (idx, _, count) = search_equal(tp, p, p, r, 4, None, None, "pair on the radius")
    assert idx[0].tolist() == [0, 2, -1, -1] and count.tolist() == [2, 2, 3, 1]


def test_search_with_a_stale_workspace(tp):
    # the grid workspace of the stream still holds the tables of another radius, then of another support
    pos, batch = ref.batched()
    search_equal(tp, pos, pos, 0.3, 64, batch, batch, "first")
    search_equal(tp, pos, pos, 0.05, 64, batch, batch, "smaller radius on the same stream")
    search_equal(tp, pos[:600], pos[:600], 0.2, 64, None, None, "another support")
    search_equal(tp, pos, pos, 0.3, 64, batch, batch, "back")


# ----------------------------------------------------------------------------------------------------------------- normals
def unit64(n):
    n = n.double().cpu().numpy()
    return n / np.sqrt((n * n).sum(1))[:, None]


def test_normals_against_eigh(tp):
    t = tables(tp)
    pos, batch = t["pos"], t["batch"]
    lam, vec = np.linalg.eigh(F.neighbourhood_covariance(pos, t["idn"], t["cn"])[:1200])
    ok = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
    print("excluded %d of 1200, smallest gap %.3g" % ((~ok).sum(), ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min()))
    assert (~ok).sum() <= 12
    got = tp.estimate_normals(dev(pos), dev(batch), 0.25, 17)
    assert got.dtype == torch.float32 and got.shape == (1203, 3)
    n = unit64(got)
    err = 1.0 - np.abs((n[:1200] * vec[:, :, 0]).sum(1))
    print("1 - |n . n_ref| max %.3g" % err[ok].max())
    assert err[ok].max() <= 1e-12
    assert torch.equal(got[1200:].cpu(), torch.tensor([[0.0, 0.0, 1.0]] * 3))  # the clouds of 2 and 1 points: k < 3
    # the largest component is positive, where the top two magnitudes are apart
    a = np.sort(np.abs(n), 1)
    clear = a[:, 2] - a[:, 1] > 1e-6
    assert clear.sum() > 1000 and (n[np.arange(1203), np.abs(n).argmax(1)][clear] > 0).all()
    # and the numpy path gives the same vectors to fp32 rounding
    npt.assert_allclose(got.cpu().numpy(), t["normals"], atol=2e-7, rtol=0)


def test_normals_towards_a_viewpoint(tp):
    t = tables(tp)
    pos, batch = t["pos"], t["batch"]
    vps = np.array([[0.5, 0.5, 5.0], [3.0, -2.0, 0.5], [0.0, 0.0, -1.0], [9.0, 9.0, 9.0]], np.float32)
    got = tp.estimate_normals(dev(pos), dev(batch), 0.25, 17, viewpoint=dev(vps))
    free = tp.estimate_normals(dev(pos), dev(batch), 0.25, 17)
    d = (vps[batch].astype(np.float64) - pos.astype(np.float64))
    n = got.double().cpu().numpy()
    assert ((n[:1200] * d[:1200]).sum(1) >= 0).all()
    assert torch.equal(got.abs(), free.abs()) and not torch.equal(got, free)
    assert torch.equal(got[1200:].cpu(), torch.tensor([[0.0, 0.0, 1.0]] * 3))
    one = tp.estimate_normals(dev(pos[:600]), None, 0.25, 17, viewpoint=[0.5, 0.5, 5.0])
    assert torch.equal(one, got[:600])


# -------------------------------------------------------------------------------------------------------------- SPFH, FPFH
@pytest.mark.parametrize("radius,max_nn", [(0.25, 40), (0.3, 200), (0.1, 3)])
def test_spfh_counts_equal_numpy(tp, radius, max_nn):
    t = tables(tp, radius, max_nn)
    got = tp.spfh_counts(dev(t["pos"]), dev(t["normals"]), dev(t["idx"]), dev(t["count"]))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(t["counts"]))
    assert torch.equal(got.sum(1).cpu(), 3 * torch.from_numpy(np.maximum(t["count"] - 1, 0)))


@pytest.mark.parametrize("radius,max_nn", [(0.25, 40), (0.3, 200), (0.1, 3)])
def test_fpfh_against_numpy(tp, radius, max_nn):
    t = tables(tp, radius, max_nn)
    args = [dev(t[k]) for k in ("pos", "normals", "idx", "count", "counts")]
    got = tp.fpfh(*args, dtype=torch.float64)
    err = np.abs(got.cpu().numpy() - t["out"]).max()
    print("|fpfh - numpy|max %.3g, bit-equal %s" % (err, np.array_equal(got.cpu().numpy(), t["out"])))
    assert got.shape == (1203, 33) and err <= 1e-11
    assert torch.equal(got.cpu(), torch.from_numpy(t["out"]))  # one association per sum on both sides: the same bits
    got32 = tp.fpfh(*args)
    assert got32.dtype == torch.float32 and torch.equal(got32, got.float())
    rows = torch.tensor([1202, 5, 5, 700, 1200, 0], device=DEV)
    assert torch.equal(tp.fpfh(*args, rows=rows, dtype=torch.float64), got[rows])
    assert torch.equal(tp.fpfh(*args, rows=rows), got32[rows])


# -------------------------------------------------------------------------------------------------- end to end and plumbing
def test_plane_known_answer_on_the_device(tp):
    p = ref.plane()
    pos = dev(p)
    idx, _, count = tp.hybrid_search(pos, pos, 0.15, 16)
    assert int(count.min()) >= 2 and bool((count == 16).any()) and bool((count < 16).any())
    normals = tp.estimate_normals(pos, None, 0.15, 16)
    assert torch.equal(normals.cpu(), torch.tensor([[0.0, 0.0, 1.0]] * len(p)))
    counts = tp.spfh_counts(pos, normals, idx, count)
    want = torch.zeros((len(p), 33), dtype=torch.int32)
    want[:, list(ref.PLANE_BINS)] = (count - 1).cpu()[:, None]
    assert torch.equal(counts.cpu(), want)
    out = tp.fpfh(pos, normals, idx, count, counts, dtype=torch.float64).cpu()
    want = torch.zeros((len(p), 33), dtype=torch.float64)
    want[:, list(ref.PLANE_BINS)] = 200.0
    assert float((out - want).abs().max()) <= 1e-11


def test_class_equals_the_numpy_path_and_repeats_bit_equal(tp):
    from torch_points3d_amd.dense import Data
    pos, batch = ref.batched()
    f = F.FPFH(radius=0.25, max_nn=40, radius_normal=0.25, max_nn_normal=17)
    kp = torch.tensor([1200, 3, 3, 900, 1202])
    a = f(Data(pos=dev(pos), batch=dev(batch), keypoints=kp.to(DEV)))
    assert a.shape == (5, 33) and a.dtype == torch.float32 and a.device.type == "cuda"
    full = f(Data(pos=dev(pos), batch=dev(batch)))
    assert torch.equal(full[kp.to(DEV)], a)
    for _ in range(2):
        assert torch.equal(f(Data(pos=dev(pos), batch=dev(batch))), full)
    # the numpy path runs its own Jacobi on its own sums: the normals agree to fp32 rounding, so a pair next to a bin edge
    # may fall on the other side; a histogram then moves by 100 / (k - 1).  All but a few rows must agree closely.
    host = f(Data(pos=torch.from_numpy(pos), batch=torch.from_numpy(batch)))
    close = ((full.cpu() - host).abs().max(1)[0] <= 1e-3).double().mean()
    print("rows of the device within 1e-3 of the numpy path: %.4f" % close)
    assert close >= 0.98


def bumpy(n=800, seed=12):
    g = np.random.default_rng(seed)
    p = g.random((n, 3))
    p[:, 2] = 0.15 * np.sin(5.0 * p[:, 0]) * np.cos(4.0 * p[:, 1]) + 0.1 * p[:, 0] * p[:, 1]
    return p.astype(np.float32)


def test_fpfh_matches_ransac_recover_the_pose(tp, reg):
    from torch_points3d_amd.dense import Data
    p = bumpy()
    R, t = ref.rigid()
    q = (p.astype(np.float64) @ R.T + t).astype(np.float32)
    vp = np.array([0.5, 0.5, 3.0])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    kp = torch.arange(0, 800, 2, device=DEV)
    fs = F.FPFH(0.25, 64, 0.15, 17, viewpoint=vp.astype(np.float32))(Data(pos=dev(p), keypoints=kp))
    ft = F.FPFH(0.25, 64, 0.15, 17, viewpoint=(R @ vp + t).astype(np.float32))(Data(pos=dev(q), keypoints=kp))
    # compute_matches(source, target) pairs every TARGET keypoint with a source keypoint; the pose maps target onto source,
    # as compute_dists applies it: here the "source" is the moved copy q and the "target" the fragment p, so trans = T
    ks, kt = reg.compute_matches(ft, fs, dev(q)[kp], dev(p)[kp])
    dist = reg.compute_dists(ks, kt, dev(T.astype(np.float32)))
    share = float(reg.compute_mean_correct_matches(dist, [0.05])[0])
    print("share of correct matches %.3f" % share)
    assert share > 0.5
    gen = torch.Generator(device=DEV).manual_seed(4)
    T_got = reg.ransac_registration(kt, ks, distance_threshold=0.05, num_iterations=4096, generator=gen)
    npt.assert_allclose(T_got.cpu().numpy(), T, rtol=1e-3)  # the bar of the RANSAC tests
    recall, frac = reg.feature_match_recall([(ft, fs, dev(q)[kp], dev(p)[kp], dev(T.astype(np.float32)))], [0.05], [0.05])
    assert float(frac[0, 0]) == share and recall.cpu().tolist() == [[1.0]]
