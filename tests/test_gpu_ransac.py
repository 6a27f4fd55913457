"""RANSAC registration on the GPU (csrc/ransac.hip; torchpoints.ransac_score / kabsch / ransac_pose;
registration.ransac_registration / compute_metrics) against the float64 restatement of tests/registration_ransac_ref.py.

Poses: float64 SVD-Kabsch on the same fp32 inputs, on the hypotheses that are well posed in the reference (second singular
value of the centred source sample > 1e-2 of the first, Horn's two largest eigenvalues > 1e-3 apart, relatively); they
must be all but 2 % of a case with samples of 4 (a CPU probe: 0.2 % at case A, 0 % at B; samples of 3 repeat a row with
probability ~3 / N on top, ref.ill_posed_allowance).  atol 1e-6 on R, atol 1e-6 + rtol 1e-6 on t: one rounding of a double
result to fp32 (6e-8 relative) with ~10x margin; Horn and SVD-Kabsch are 3e-13 apart on the kept hypotheses.

Counts: count64(threshold - BAND) <= counts <= count64(threshold + BAND) under the device's own pose promoted to double,
BAND = 2e-5: |coordinates| <= 4.5, at most 5 fp32 roundings per component = 1.4e-6, <= 2.4e-6 on the distance, 1e-6 for
the rounded pose; ~5x margin.  The mean width of the band must be below 1 % of N (0 at A, 5e-4 counts at B in the probe),
so that it cannot hide a wrong kernel.  (Case A's outlier rows reach |q| ~ 100, where one fp32 rounding is 8e-6: those rows
are ~100 away from any threshold, so their sums need no band at all.)

Whole solve: the device's best index is a maximiser up to the band; the refined pose is held to the restatement's refit
started from that index with test_gpu_ppnet._close64 at rtol 1e-4 (the bar of test_fgr_against_float64), under the
precondition, asserted from the reference, that no correspondence lies within BAND of the threshold under the poses
the refit goes through."""
import numpy.testing as npt
import pytest
import torch

import registration_ransac_ref as ref
import registration_ref as rr
from test_gpu_ppnet import _close64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 2e-5


@pytest.fixture(scope="module")
def tp():
    from torch_points3d_amd import torchpoints
    return torchpoints


@pytest.fixture(scope="module")
def reg():
    from torch_points3d_amd import registration
    return registration


def _case(name):
    if name == "a":
        xyz, tgt, T = ref.case_a()
        return xyz, tgt, T, 0.01, 4096
    xyz, tgt, T = ref.case_b()
    return xyz, tgt, T, 0.05, 4097


_scored = {}


def scored(tp, name, n):
    """case `name` with samples of n, scored on the device once: everything the tests of that case share"""
    key = (name, n)
    if key not in _scored:
        xyz, tgt, T, thr, H = _case(name)
        samples = ref.draw(len(xyz), H, n, 11 + n)
        poses, counts = tp.ransac_score(xyz.to(DEV), tgt.to(DEV), samples.to(DEV), thr)
        _scored[key] = dict(xyz=xyz, tgt=tgt, T=T, thr=thr, samples=samples, poses=poses, counts=counts,
                            poses64=ref.hypotheses(xyz, tgt, samples), keep=ref.well_posed(xyz, tgt, samples))
    return _scored[key]


def check_score(poses, counts, xyz, tgt, samples, thr, what, share=None, poses64=None, keep=None):
    H, n = samples.shape
    poses64 = ref.hypotheses(xyz, tgt, samples) if poses64 is None else poses64
    keep = ref.well_posed(xyz, tgt, samples) if keep is None else keep
    excluded = float((~keep).double().mean())
    lo64, _, hi64 = ref.counts_banded(poses64[keep], xyz, tgt, thr, BAND)
    width = float((hi64 - lo64).double().mean()) if bool(keep.any()) else 0.0
    print("%s: %.2f %% of %d hypotheses ill-posed, mean band width %.3g counts of N = %d" % (what, 100 * excluded, H, width,
                                                                                           len(xyz)))
    if share is not None:
        assert excluded <= share
    assert width < 0.01 * len(xyz)
    assert poses.dtype == torch.float32 and tuple(poses.shape) == (H, 3, 4) and counts.dtype == torch.int32
    assert tuple(counts.shape) == (H,) and poses.device.type == "cuda" and counts.device.type == "cuda"
    P = poses.cpu().double()
    assert bool(torch.isfinite(P).all())
    err_R = (P[keep][:, :, :3] - poses64[keep][:, :, :3]).abs()
    err_t = (P[keep][:, :, 3] - poses64[keep][:, :, 3]).abs()
    if bool(keep.any()):
        print("%s: |R - R64|max %.3g, |t - t64|max %.3g at |t|max %.3g" % (what, float(err_R.max()), float(err_t.max()),
                                                                          float(poses64[keep][:, :, 3].abs().max())))
        assert float(err_R.max()) <= 1e-6
        assert bool((err_t <= 1e-6 + 1e-6 * poses64[keep][:, :, 3].abs()).all())
    # a proper rotation, whatever the sample
    assert float((torch.det(P[:, :, :3]) - 1).abs().max()) < 1e-5
    lo, _, hi = ref.counts_banded(P, xyz, tgt, thr, BAND)
    c = counts.cpu().long()
    assert float((hi - lo).double().mean()) < 0.01 * len(xyz)
    assert bool((lo <= c).all()) and bool((c <= hi).all()), "%s: %d counts outside the band" % (what, int(((c < lo) | (c > hi)).sum()))
    return lo, hi


@pytest.mark.parametrize("name,n", [("a", 4), ("b", 4), ("a", 3), ("b", 3)])
def test_score_against_float64(tp, name, n):
    s = scored(tp, name, n)
    check_score(s["poses"], s["counts"], s["xyz"], s["tgt"], s["samples"], s["thr"], "case %s, n = %d" % (name, n),
                share=ref.ill_posed_allowance(len(s["xyz"]), n), poses64=s["poses64"], keep=s["keep"])
    poses, counts = tp.ransac_score(s["xyz"].to(DEV), s["tgt"].to(DEV), s["samples"].to(DEV), s["thr"])
    assert torch.equal(poses, s["poses"]) and torch.equal(counts, s["counts"])
    if name == "a" and n == 4:
        c = s["counts"].cpu()
        assert int(c.max()) == 90 and int((c == 90).sum()) > 1000  # (ties for the lowest-index rule to break)


def _seam_sizes(tp):
    t, b = tp.RANSAC_TILE, tp.RANSAC_HYP_BLOCK
    return [(N, 257) for N in (3, 4, t - 1, t, t + 1, 2 * t + 1)] + [(100, H) for H in (1, b - 1, b + 1)]


@pytest.mark.parametrize("n", [3, 4])
def test_score_at_the_seams(tp, n):
    """N around the tile (the number of splits of N changes between RANSAC_TILE and RANSAC_TILE + 1 and again at
    2 RANSAC_TILE + 1: one, two and three workgroups per block of hypotheses), H around the block of hypotheses, and
    clouds that do not start on 16 bytes (the kernel's other load path)"""
    from torch_points3d_amd import _lib
    lib = _lib.load()
    splits = set()
    for N, H in _seam_sizes(tp):
        xyz, tgt, _ = ref.case_b(N, 100 + N)
        samples = ref.draw(N, H, n, N + H)
        poses, counts = tp.ransac_score(xyz.to(DEV), tgt.to(DEV), samples.to(DEV), 0.05)
        check_score(poses, counts, xyz, tgt, samples, 0.05, "N = %d, H = %d, n = %d" % (N, H, n))
        splits.add(lib.tp3d_ransac_splits(N, H))
        again = tp.ransac_score(xyz.to(DEV), tgt.to(DEV), samples.to(DEV), 0.05)
        assert torch.equal(again[0], poses) and torch.equal(again[1], counts)
    assert {1, 2, 3} <= splits
    # rows 1.. of a larger buffer: 12 bytes past an aligned address
    xyz, tgt, _ = ref.case_b(2 * tp.RANSAC_TILE + 2, 9)
    samples = ref.draw(len(xyz) - 1, 257, n, 5)
    dx, dt = xyz.to(DEV), tgt.to(DEV)
    assert dx[1:].data_ptr() % 16 != 0 and dx[1:].is_contiguous()
    poses, counts = tp.ransac_score(dx[1:], dt[1:], samples.to(DEV), 0.05)
    check_score(poses, counts, xyz[1:], tgt[1:], samples, 0.05, "unaligned clouds, n = %d" % n)
    aligned = tp.ransac_score(dx[1:].clone(), dt[1:].clone(), samples.to(DEV), 0.05)
    assert torch.equal(aligned[0], poses) and torch.equal(aligned[1], counts)


def test_score_refuses_rows_outside_the_cloud(tp):
    """a sampled row outside [0, N) is never dereferenced: NaNs and the count 0; the other hypotheses are untouched"""
    s = scored(tp, "b", 4)
    samples = s["samples"][:300].clone()
    samples[7, 2] = len(s["xyz"])
    samples[299, 0] = -1
    poses, counts = tp.ransac_score(s["xyz"].to(DEV), s["tgt"].to(DEV), samples.to(DEV), s["thr"])
    bad = torch.zeros(300, dtype=torch.bool)
    bad[[7, 299]] = True
    assert bool(torch.isnan(poses.cpu()[bad]).all()) and bool((counts.cpu()[bad] == 0).all())
    assert torch.equal(poses.cpu()[~bad], s["poses"].cpu()[:300][~bad]) and torch.equal(counts.cpu()[~bad], s["counts"].cpu()[:300][~bad])
    T, stats = tp.ransac_pose(s["xyz"].to(DEV), s["tgt"].to(DEV), s["thr"], samples=samples[[7, 299]].to(DEV))
    assert torch.equal(T.cpu(), torch.eye(4)) and int(stats["best"]) == 0 and int(stats["best_count"]) == 0
    assert int(stats["inliers"]) == 0 and float(stats["inlier_rmse"]) == 0.0


def test_select_takes_the_lowest_index_of_the_best(tp):
    """a samples table whose only good hypotheses sit where they are put: at index 0, at H - 1, on both sides of the
    seam between two blocks of hypotheses and of the select kernel's stride"""
    gen = torch.Generator().manual_seed(4)
    xyz = torch.rand(100, 3, generator=gen) * 2 - 1
    T = ref.case_a()[2]
    tgt = xyz.mm(T[:3, :3].T) + T[:3, 3]
    tgt[60:] = torch.rand(40, 3, generator=gen) * 40 + 10  # rows 60.. match nothing
    H, b = 1300, tp.RANSAC_HYP_BLOCK
    junk = torch.randint(60, 100, (H, 4), generator=gen)
    good = torch.tensor([0, 1, 2, 3])
    dx, dt = xyz.to(DEV), tgt.to(DEV)
    for places in ([0], [H - 1], [b - 1], [b], [b - 1, b], [1023], [1024], [1024, 1023, H - 1], [0, H - 1]):
        samples = junk.clone()
        samples[places] = good
        _, counts = tp.ransac_score(dx, dt, samples.to(DEV), 0.01)
        c = counts.cpu()
        assert int(c.max()) == 60 and sorted(torch.nonzero(c == 60).view(-1).tolist()) == sorted(places)
        T_got, stats = tp.ransac_pose(dx, dt, 0.01, samples=samples.to(DEV))
        assert int(stats["best"]) == min(places) and int(stats["best_count"]) == 60 and int(stats["inliers"]) == 60
        assert stats["best"].dtype == torch.int64 and stats["best"].device.type == "cuda"
        npt.assert_allclose(T_got.cpu().numpy(), T.numpy(), rtol=1e-3)


@pytest.mark.parametrize("name,n", [("a", 4), ("b", 4), ("b", 3)])
def test_whole_solve_against_float64(tp, reg, name, n):
    s = scored(tp, name, n)
    xyz, tgt, thr, samples = s["xyz"], s["tgt"], s["thr"], s["samples"]
    dx, dt, ds = xyz.to(DEV), tgt.to(DEV), samples.to(DEV)
    T, stats = tp.ransac_pose(dx, dt, thr, samples=ds)
    assert T.dtype == torch.float32 and tuple(T.shape) == (4, 4) and T.device.type == "cuda"
    c = s["counts"].cpu().long()
    best = int(stats["best"])
    assert best == int(torch.nonzero(c == c.max())[0]) and int(stats["best_count"]) == int(c.max())
    lo, _, hi = ref.counts_banded(s["poses"].cpu(), xyz, tgt, thr, BAND)
    assert int(hi[best]) >= int(lo.max())  # a maximiser up to the band
    assert bool(s["keep"][best])
    want, inliers, sum_d2, margin = ref.refit(xyz, tgt, thr, s["poses64"][best])
    print("case %s, n = %d: best %d with %d, %d inliers after the refit, least | |d| - threshold | %.3g" % (name, n, best, int(c.max()),
                                                                                                        inliers, margin))
    assert margin > BAND
    d = ref.distances(s["poses64"][best][None], xyz, tgt)[0]
    want32 = rr.estimate_transfo(xyz[d < thr], tgt[d < thr])  # the reference's fp32 arithmetic on the same inliers
    _close64(T.cpu()[:3], want32[:3], want, 1e-4, 0.0, what="refined pose, case %s" % name)
    assert torch.equal(T.cpu()[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
    assert int(stats["inliers"]) == inliers and float(stats["fitness"]) == inliers / len(xyz)
    npt.assert_allclose(float(stats["inlier_rmse"]), (sum_d2 / inliers) ** 0.5, rtol=1e-3, atol=1e-9)
    assert all(v.device.type == "cuda" and v.dim() == 0 for v in stats.values())
    if name == "a":
        npt.assert_allclose(T.cpu().numpy(), s["T"].numpy(), rtol=1e-3)  # the reference test's own bar
        assert int(stats["inliers"]) == 90 and float(stats["fitness"]) == 0.9 and float(stats["inlier_rmse"]) < 1e-5
    # bit-equal repeats, the public function, more rounds of refit
    T2, stats2 = tp.ransac_pose(dx, dt, thr, samples=ds)
    assert torch.equal(T, T2) and all(torch.equal(stats[k], stats2[k]) for k in stats)
    if n == 4:
        assert torch.equal(reg.ransac_registration(dx, dt, thr, samples=ds), T)
    want2, inliers2, _, margin2 = ref.refit(xyz, tgt, thr, s["poses64"][best], refine=2)
    assert margin2 > BAND
    T3, stats3 = tp.ransac_pose(dx, dt, thr, samples=ds, refine=2)
    d = ref.distances(want[None], xyz, tgt)[0]
    _close64(T3.cpu()[:3], rr.estimate_transfo(xyz[d < thr], tgt[d < thr])[:3], want2, 1e-4, 0.0, what="two rounds of refit")
    assert int(stats3["inliers"]) == inliers2
    T0, stats0 = tp.ransac_pose(dx, dt, thr, samples=ds, refine=0)  # no refit: the hypothesis' own pose
    assert torch.equal(T0[:3], s["poses"][best]) and int(stats0["best"]) == best


def test_default_samples_follow_the_generator(tp, reg):
    xyz, tgt, T = ref.case_a()
    dx, dt = xyz.to(DEV), tgt.to(DEV)
    gen = torch.Generator(device=DEV)
    out = []
    for _ in range(2):
        gen.manual_seed(3)
        out.append(tp.ransac_pose(dx, dt, 0.01, num_iterations=2048, generator=gen))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1]["best"], out[1][1]["best"])
    npt.assert_allclose(out[0][0].cpu().numpy(), T.numpy(), rtol=1e-3)
    gen.manual_seed(3)
    got = reg.ransac_registration(dx, dt, distance_threshold=0.01, num_iterations=2048, generator=gen)
    assert got.device.type == "cuda" and torch.equal(got, out[0][0])
    gen.manual_seed(3)
    three = tp.ransac_pose(dx, dt, 0.01, num_iterations=2048, ransac_n=3, generator=gen)
    npt.assert_allclose(three[0].cpu().numpy(), T.numpy(), rtol=1e-3)


def _kabsch_case(N, seed):
    xyz, tgt, _ = ref.case_b(max(N, 4), seed)
    return xyz[:N], tgt[:N]


@pytest.mark.parametrize("N", [3, 64, 257, 5000])
def test_kabsch_against_float64(tp, reg, N):
    xyz, tgt = _kabsch_case(N, N)
    dx, dt = xyz.to(DEV), tgt.to(DEV)
    got = tp.kabsch(dx, dt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 4)
    _close64(got.cpu(), rr.estimate_transfo(xyz, tgt), ref.to4x4(ref.estimate_transfo(xyz, tgt)), 1e-4, 0.0, what="kabsch N = %d" % N)
    assert torch.equal(got, tp.kabsch(dx, dt))
    gen = torch.Generator().manual_seed(N)
    w = torch.rand(N, generator=gen) + 0.1
    got_w = tp.kabsch(dx, dt, w.to(DEV))
    want_w = ref.to4x4(ref.estimate_transfo(xyz, tgt, w))
    want_w32 = ref.to4x4(ref.estimate_transfo(xyz, tgt, w)).float()
    _close64(got_w.cpu(), want_w32, want_w, 1e-4, 0.0, what="weighted kabsch N = %d" % N)
    assert torch.equal(got_w, tp.kabsch(dx, dt, w.to(DEV)))
    if N >= 64:  # a zero-weight tail is as good as absent
        head = (2 * N) // 3
        w0 = torch.ones(N)
        w0[head:] = 0
        got_0 = tp.kabsch(dx, dt, w0.to(DEV))
        _close64(got_0.cpu(), rr.estimate_transfo(xyz[:head], tgt[:head]), ref.to4x4(ref.estimate_transfo(xyz[:head], tgt[:head])),
                 1e-4, 0.0, what="zero-weight tail N = %d" % N)
    assert torch.equal(tp.kabsch(dx, dt, torch.zeros(N, device=DEV)), torch.eye(4, device=DEV))  # no weight at all


def test_kabsch_planar_mirrored(tp):
    """a planar cloud against its mirror image: the SVD's V U^T is a reflection and the determinant correction turns it
    into the rotation by pi about an axis in the plane; Horn's quaternion form can only give a rotation"""
    gen = torch.Generator().manual_seed(8)
    p = torch.rand(257, 3, generator=gen) * 2 - 1
    p[:, 2] = 0.25
    R = rr.rotation([0.3, -0.5, 0.4], 0.8).float()
    q = (p * torch.tensor([-1.0, 1.0, 1.0])).mm(R.T) + torch.tensor([0.3, -0.2, 0.5])
    want = ref.estimate_transfo(p, q)
    S = torch.linalg.svdvals((p - p.mean(0)).double().T @ (q - q.mean(0)).double())
    assert float(S[2]) < 1e-6 * float(S[1])  # the third direction is free: uncorrected, V U^T may come out a reflection
    plane = (p[:, :2] - p[:, :2].mean(0)).double()
    image = ((q - q.mean(0)).double() @ R.double())[:, :2]  # the in-plane map is a reflection: only the correction
    assert float(torch.det(torch.linalg.lstsq(plane, image).solution)) < -0.99  # (or Horn) makes the pose a rotation
    got = tp.kabsch(p.to(DEV), q.to(DEV)).cpu()
    assert abs(float(torch.det(got[:3, :3].double())) - 1) < 1e-5
    _close64(got, rr.estimate_transfo(p, q), ref.to4x4(want), 1e-4, 0.0, what="planar, mirrored")
    # the plane is fitted exactly: the mirror image IS reachable by a proper rotation
    assert float((p.double() @ got[:3, :3].double().T + got[:3, 3].double() - q.double()).norm(dim=1).max()) < 1e-5


def test_all_outliers_keep_the_hypothesis_pose(tp):
    gen = torch.Generator().manual_seed(0)
    xyz, tgt = torch.rand(200, 3, generator=gen), torch.rand(200, 3, generator=gen) * 7
    samples = ref.draw(200, 512, 4, 1)
    poses64 = ref.hypotheses(xyz, tgt, samples)
    assert int(ref.counts_banded(poses64, xyz, tgt, 1e-3, BAND)[2].max()) < 3
    poses, counts = tp.ransac_score(xyz.to(DEV), tgt.to(DEV), samples.to(DEV), 1e-3)
    T, stats = tp.ransac_pose(xyz.to(DEV), tgt.to(DEV), 1e-3, samples=samples.to(DEV), refine=2)
    best = int(stats["best"])
    c = counts.cpu()
    assert int(c.max()) < 3 and best == int(torch.nonzero(c == c.max())[0])
    assert bool(torch.isfinite(T).all()) and torch.equal(T[:3], poses[best])
    _, inliers, _, margin = ref.refit(xyz, tgt, 1e-3, poses64[best], refine=2)
    assert margin > BAND and inliers < 3
    assert int(stats["inliers"]) == inliers and float(stats["fitness"]) == inliers / 200


def test_small_call_after_a_large_one(tp):
    """the workspace is grow-only and shared: a small problem after a large one must not see the large one's leftovers"""
    s = scored(tp, "a", 4)
    dx, dt, ds = s["xyz"].to(DEV), s["tgt"].to(DEV), s["samples"][:64].to(DEV)
    first = tp.ransac_pose(dx, dt, s["thr"], samples=ds)
    first_k = tp.kabsch(dx, dt)
    xyz, tgt, _ = ref.case_b(5000, 3)
    big = tp.ransac_pose(xyz.to(DEV), tgt.to(DEV), 0.05, samples=ref.draw(5000, 8192, 4, 2).to(DEV))
    assert float(big[1]["fitness"]) > 0.6
    again = tp.ransac_pose(dx, dt, s["thr"], samples=ds)
    assert torch.equal(first[0], again[0]) and all(torch.equal(first[1][k], again[1][k]) for k in first[1])
    assert torch.equal(first_k, tp.kabsch(dx, dt))
    assert torch.equal(tp.ransac_score(dx, dt, ds, s["thr"])[1], s["counts"][:64])


def test_argument_errors(tp, reg):
    xyz = torch.rand(10, 3, device=DEV)
    samples = torch.zeros(4, 4, dtype=torch.long, device=DEV)
    for bad in (lambda: tp.ransac_score(xyz[:2], xyz[:2], samples, 0.1), lambda: tp.ransac_pose(xyz[:2], xyz[:2], 0.1),
                lambda: tp.kabsch(xyz[:2], xyz[:2]), lambda: tp.ransac_pose(xyz, xyz, 0.1, num_iterations=0),
                lambda: tp.ransac_score(xyz, xyz, samples[:0], 0.1), lambda: tp.ransac_score(xyz, xyz, samples[:, :2], 0.1),
                lambda: tp.ransac_score(xyz, xyz, samples.view(-1), 0.1), lambda: tp.ransac_score(xyz, xyz[:9], samples, 0.1),
                lambda: tp.ransac_score(xyz, xyz, torch.zeros(4, 9, dtype=torch.long, device=DEV), 0.1),
                lambda: tp.ransac_pose(xyz, xyz, 0.1, ransac_n=2), lambda: tp.kabsch(xyz, xyz, torch.ones(9, device=DEV)),
                lambda: tp.kabsch(xyz.view(-1), xyz.view(-1)), lambda: tp.ransac_score(xyz.cpu(), xyz.cpu(), samples.cpu(), 0.1),
                lambda: tp.ransac_score(xyz, xyz, samples.cpu(), 0.1), lambda: tp.kabsch(xyz.cpu(), xyz.cpu()),
                lambda: tp.kabsch(xyz, xyz, torch.ones(10)), lambda: tp.ransac_pose(xyz.cpu(), xyz.cpu(), 0.1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        reg.ransac_registration(xyz, xyz, num_iterations=0)


def _metrics_inputs():
    xyz, tgt, T = ref.case_b(600, 6)
    gen = torch.Generator().manual_seed(2)
    feat = torch.randn(600, 32, generator=gen)
    feat = feat / feat.norm(dim=1, keepdim=True)
    perm = torch.randperm(600, generator=gen)
    feat_t = (feat + 0.02 * torch.randn(600, 32, generator=gen))[perm]
    return [t.to(DEV) for t in (xyz, tgt[perm], feat, feat_t, T.float(), ref.draw(600, 1024, 4, 9))]


def test_compute_metrics_is_the_composition(reg):
    xyz, tgt, feat, feat_t, T, samples = _metrics_inputs()
    clean = xyz @ T[:3, :3].T + T[:3, 3]
    res = reg.compute_metrics(xyz, tgt, feat, feat_t, T, use_ransac=True, ransac_thresh=0.05, xyz_gt=xyz, xyz_target_gt=clean,
                              samples=samples)
    matches = reg.get_matches(feat, feat_t)
    src, dst = xyz[matches[:, 0]], tgt[matches[:, 1]]
    hit = reg.compute_hit_ratio(src, dst, T, 0.1)
    want = {"hit_ratio": hit, "feat_match_ratio": (hit > 0.05).float()}
    for tag, T_est in (("fgr", reg.fast_global_registration(src, dst)), ("ransac", reg.ransac_registration(src, dst, 0.05, samples=samples))):
        te, re = reg.compute_transfo_error(T_est, T)
        want.update({"trans_error_" + tag: te, "rot_error_" + tag: re, "rre_" + tag: (re < 5).float(), "rte_" + tag: (te < 5).float(),
                     "sr_" + tag: reg.compute_scaled_registration_error(xyz, T, T_est),
                     "registration_recall_" + tag: reg.compute_registration_recall(xyz, clean, T_est, 0.2)})
    assert sorted(res) == sorted(want)
    for k in want:
        assert res[k].device.type == "cuda" and res[k].dim() == 0 and torch.equal(res[k], want[k]), k
    assert bool(res["registration_recall_ransac"]) and float(res["hit_ratio"]) > 0.6 and float(res["rre_ransac"]) == 1.0 and float(res["trans_error_ransac"]) < 0.01
    plain = reg.compute_metrics(xyz, tgt, feat, feat_t, T)
    assert sorted(plain) == sorted(k for k in want if "ransac" not in k and "recall" not in k)


def test_ransac_reads_nothing_back(tp, reg):
    xyz, tgt, feat, feat_t, T, samples = _metrics_inputs()
    gen = torch.Generator(device=DEV)

    def run():
        tp.ransac_pose(xyz, tgt, 0.05, samples=samples)
        tp.ransac_pose(xyz, tgt, 0.05, num_iterations=512, generator=gen)
        reg.compute_metrics(xyz, tgt, feat, feat_t, T, use_ransac=True, ransac_thresh=0.05, samples=samples)

    run()  # warm-up: library load, workspaces
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enforced = False
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            enforced = True
        if enforced:
            run()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not enforced:
        pytest.skip("this ROCm build of torch does not enforce set_sync_debug_mode('error'): a deliberate .item() did not raise")
