"""Registration on the GPU (csrc/registration.hip, torch_points3d_amd.registration) against the float64 brute force of
tests/registration_ref.py on the device and against the reference's own results (tests/golden/registration.npz).

feature_nn.  idx must equal the float64 argmin on every row whose float64 gap between the best and the second best d^2 is
at least g = 16 * max|ref32 - ref64| over the restatement's own fp32 d^2 matrix (two correct fp32 evaluations may order a
closer pair either way); at most 1 % of the rows may fall below g.  On these inputs, evaluated on the CPU: the restatement's
fp32 error is <= 7e-7, so g ~ 1e-5; the smallest gaps are 4.7e-5 at (1024, 256, 32), 3.7e-4 at (65, 255, 3), 5.0e-4 at
(63, 257, 16) and 6.9e-6 at (257, 1025, 33), where one row of 257 falls below g -- for such a row the candidate taken
must be within g of the best in float64.  dist2 is held to test_gpu_ppnet._close64 at rtol 1e-5 without an absolute term.
Losses, poses and metrics: _close64 against the float64 results, rtol 1e-5 for values, 1e-4 for gradients and poses."""
import copy
import types

import numpy as np
import pytest
import torch

import registration_ref as rr
from conftest import load_golden
from test_gpu_ppnet import _close64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1), (63, 257, 16), (65, 255, 3), (64, 64, 1), (257, 1025, 33), (1024, 256, 32), (130, 4097, 96), (70, 300, 130)]


@pytest.fixture(scope="module")
def g():
    return load_golden("registration")


@pytest.fixture(scope="module")
def tp():
    from torch_points3d_amd import torchpoints
    return torchpoints


@pytest.fixture(scope="module")
def reg():
    from torch_points3d_amd import registration
    return registration


def cfg(g, name):
    return g["config/" + name].reshape(-1)[0].item()


def f64(g, key):
    return torch.from_numpy(np.asarray(g["f64/" + key]))


def unit(t):
    return t / t.norm(dim=1, keepdim=True)


def nn_inputs(P, S, C):
    torch.manual_seed(0)
    if C == 1:  # integers and quarters: the nearest is 0.0625 away in d^2, the second nearest 0.5625
        b = torch.randperm(S).float().view(S, 1)
        a = b[torch.randint(0, S, (P,))] + 0.25
        return a.to(DEV), b.to(DEV)
    return unit(torch.randn(P, C)).to(DEV), unit(torch.randn(S, C)).to(DEV)


def check_nn(got_d, got_i, a, b, pos_a=None, pos_b=None, min_dist=None, what=""):
    """the conditions of the module docstring; returns the number of rows whose gap is below g"""
    ref64_d, ref64_i, D64 = rr.feature_nn(a.double(), b.double(), pos_a, pos_b, min_dist)
    ref32_d, _, D32 = rr.feature_nn(a, b, pos_a, pos_b, min_dist)
    finite = torch.isfinite(D64)
    assert torch.equal(finite, torch.isfinite(D32))
    own = float((D32.double() - D64)[finite].abs().max()) if bool(finite.any()) else 0.0
    gth = 16.0 * own
    gap = rr.nn_gap(D64)
    sure = gap >= gth
    below = int((~sure).sum())
    print("%s: |ref32 - ref64|max %.3g, g %.3g, least gap %.3g, rows below g %d of %d" % (what, own, gth, float(gap.min()), below,
                                                                                        len(a)))
    assert below <= len(a) // 100
    assert got_i.dtype == torch.int64 and got_d.dtype == torch.float32
    assert torch.equal(got_i[sure], ref64_i[sure])
    none = ref64_i < 0
    assert torch.equal(got_i < 0, none)
    assert bool(torch.isinf(got_d[none]).all()) and bool((got_d[none] > 0).all())
    # rows below g: whichever candidate was taken, its float64 distance is within g of the best
    if below:
        taken = D64[~sure].gather(1, got_i[~sure].clamp(min=0).view(-1, 1)).view(-1)
        assert bool((taken - ref64_d[~sure] <= gth).all())
    _close64(got_d[~none], ref32_d[~none], ref64_d[~none], 1e-5, 0.0, what=what + " dist2")
    return below


@pytest.mark.parametrize("P,S,C", SHAPES)
def test_feature_nn_against_float64(tp, P, S, C):
    a, b = nn_inputs(P, S, C)
    d, i = tp.feature_nn(a, b)
    check_nn(d, i, a, b, what="feature_nn (%d, %d, %d)" % (P, S, C))
    if C == 1:
        assert bool((d == 0.0625).all())
    d2, i2 = tp.feature_nn(a, b)
    assert torch.equal(d, d2) and torch.equal(i, i2)


def test_feature_nn_ties_take_the_lowest_index(tp):
    a, b = nn_inputs(70, 1025, 32)
    for row in (3, 700, 1024):
        b[row] = a[5]
    d, i = tp.feature_nn(a, b)
    assert int(i[5]) == 3 and float(d[5]) == 0.0
    rest = torch.arange(len(a), device=DEV) != 5  # (row 5 has a gap of 0 on purpose)
    check_nn(d[rest], i[rest], a[rest], b, what="ties, the other rows")
    b[3] = float("nan")  # a NaN distance never wins: the next tie takes over
    d, i = tp.feature_nn(a, b)
    assert int(i[5]) == 700 and float(d[5]) == 0.0 and bool((i != 3).all()) and bool(torch.isfinite(d).all())
    d, i = tp.feature_nn(a, torch.full_like(b, float("nan")))
    assert bool((i == -1).all()) and bool(torch.isinf(d).all())
    d, i = tp.feature_nn(a, b[:0])
    assert bool((i == -1).all()) and bool(torch.isinf(d).all())
    assert tp.feature_nn(a[:0], b)[1].shape == (0,)


def test_feature_nn_spatial_exclusion(tp):
    """positions on the 5 x 5 x 5 lattice of pitch 0.1 (every distance is 0.1 sqrt(k), k an integer: nowhere near the
    thresholds).  At min_dist 0.15 a row loses itself and its 18 closest neighbours; at 0.35 (k >= 13 is kept) the six
    neighbours of the centre keep 16 candidates each and the centre, within 0.1 sqrt(12) of every node, keeps none."""
    torch.manual_seed(0)
    nodes = torch.tensor([[x, y, z] for x in range(5) for y in range(5) for z in range(5)], dtype=torch.float32) * 0.1
    pos = nodes[torch.randperm(len(nodes))].to(DEV)
    feats = unit(torch.randn(len(pos), 24)).to(DEV)
    others = unit(torch.randn(len(pos), 24)).to(DEV)
    for min_dist in (0.15, 0.35):
        d, i = tp.feature_nn(feats, others, pos, pos, min_dist)
        check_nn(d, i, feats, others, pos, pos, min_dist, what="exclusion %.2f" % min_dist)
        kept = rr.allowed_pairs(pos, pos, min_dist).sum(1)
        print("candidates kept per row: least %d, most %d" % (int(kept.min()), int(kept.max())))
        d2, i2 = tp.feature_nn(feats, others, pos, pos, min_dist)
        assert torch.equal(d, d2) and torch.equal(i, i2)
        if min_dist == 0.15:
            assert int(kept.max()) < len(pos) and bool((i >= 0).all())
    centre = int((pos - 0.2).abs().sum(1).argmin())
    assert int(kept[centre]) == 0 and sorted(kept.tolist())[1] == 16
    assert int(i[centre]) == -1 and float(d[centre]) == float("inf") and int((i < 0).sum()) == 1
    # different query and candidate positions, and more candidates than one chunk holds
    pos_b = torch.cat([pos, pos + 0.1, pos - 0.1])
    many = unit(torch.randn(len(pos_b), 24)).to(DEV)
    d, i = tp.feature_nn(feats, many, pos, pos_b, 0.35)
    check_nn(d, i, feats, many, pos, pos_b, 0.35, what="exclusion, 375 candidates")


def test_gather_rows_forward_and_ordered_gradient(tp):
    torch.manual_seed(0)
    x = torch.randn(300, 33).to(DEV)
    idx = torch.randint(0, 150, (4000,)).to(DEV)  # repeats (long runs included), rows 150.. unused
    idx[:600] = 7
    cot = torch.randn(4000, 33).to(DEV)
    grads = []
    for _ in range(2):
        xin = x.clone().requires_grad_(True)
        out = tp.gather_rows(xin, idx)
        assert torch.equal(out, x[idx])
        (out * cot).sum().backward()
        grads.append(xin.grad)
    assert torch.equal(grads[0], grads[1])
    x64 = x.double().requires_grad_(True)
    (x64[idx] * cot.double()).sum().backward()
    x32 = x.clone().requires_grad_(True)
    (x32[idx] * cot).sum().backward()
    _close64(grads[0], x32.grad, x64.grad, 1e-5, 0.0, what="gather_rows gradient")
    assert bool((grads[0][150:] == 0).all()) and bool((grads[0][:150].abs().sum(1) > 0).all())


def _hn_inputs(g):
    return (g["F0"].to(DEV), g["F1"].to(DEV), g["matches"].to(DEV), g["sel0"].to(DEV), g["sel1"].to(DEV), g["pos_sel"].to(DEV))


def _run_hn(reg, g, F0, F1, matches, sel0, sel1, pos_sel):
    loss_fn = reg.ContrastiveHardestNegativeLoss(cfg(g, "pos_thresh"), cfg(g, "neg_thresh"), cfg(g, "num_pos"),
                                                 cfg(g, "num_hn_samples"))
    a, b = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
    loss = loss_fn(a, b, matches, sel0=sel0, sel1=sel1, pos_sel=pos_sel)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def test_hardest_negative_loss_against_the_reference(reg, g):
    first = _run_hn(reg, g, *_hn_inputs(g))
    for got, key, rtol in zip(first, ("hn/loss", "hn/dF0", "hn/dF1"), (1e-5, 1e-4, 1e-4)):
        _close64(got, g[key], f64(g, key), rtol, 0.0, what=key)
    again = _run_hn(reg, g, *_hn_inputs(g))
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_hardest_negative_loss_default_selections_and_empty_negatives(reg, g):
    F0, F1, matches = g["F0"].to(DEV), g["F1"].to(DEV), g["matches"].to(DEV)
    gen = torch.Generator(device=DEV)
    loss_fn = reg.ContrastiveHardestNegativeLoss(0.1, 1.4, 64, 128, generator=gen)
    gen.manual_seed(5)
    one = loss_fn(F0, F1, matches)
    gen.manual_seed(5)
    two = loss_fn(F0, F1, matches)
    assert bool(torch.isfinite(one)) and torch.equal(one, two)
    # every mined pair is a positive pair: fragments that are copies of each other, every row matched to itself and mined
    # among all rows -- the nearest row of F0[i] in F1 is F1[i], distance 0; the mean over no negatives is NaN
    n = 40
    same = F0[:n].clone()
    pairs = torch.arange(n, device=DEV).view(-1, 1).repeat(1, 2)
    full = torch.arange(n, device=DEV)
    loss = reg.ContrastiveHardestNegativeLoss(0.1, 1.4, 64, 128)(same, same.clone(), pairs, sel0=full, sel1=full)
    assert bool(torch.isnan(loss))


def test_hardest_negative_step_reads_nothing_back(reg, g):
    args = _hn_inputs(g)
    _run_hn(reg, g, *args)  # warm-up: library load, workspaces
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
            _run_hn(reg, g, *args)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not enforced:
        pytest.skip("this ROCm build of torch does not enforce set_sync_debug_mode('error'): a deliberate .item() did not raise")


def test_batch_hard_loss_against_the_reference(reg, g):
    F0, F1, matches, xyz0 = g["F0"].to(DEV), g["F1"].to(DEV), g["matches"].to(DEV), g["xyz0"].to(DEV)
    loss_fn = reg.BatchHardContrastiveLoss(cfg(g, "bh_pos_thresh"), cfg(g, "bh_neg_thresh"), cfg(g, "bh_min_dist"))
    runs = []
    for _ in range(2):
        a, b = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
        loss = loss_fn(a, b, matches, xyz0, g["xyz1"].to(DEV))
        loss.backward()
        runs.append((loss.detach(), a.grad, b.grad))
    for got, key, rtol in zip(runs[0], ("bh/loss", "bh/dF0", "bh/dF1"), (1e-5, 1e-4, 1e-4)):
        _close64(got, g[key], f64(g, key), rtol, 0.0, what=key)
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    # a pair with no allowed negative contributes 0: all positions within min_dist of each other
    loss = loss_fn(F0, F1, matches[:5], torch.zeros_like(xyz0))
    furthest = (F0[matches[:5, 0]] - F1[matches[:5, 1]]).pow(2).max(1)[0]
    want = torch.relu(furthest - cfg(g, "bh_pos_thresh")).pow(2).mean()
    torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-8)


def _fgr_case(n, outliers, seed):
    gen = torch.Generator().manual_seed(seed)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = rr.rotation([0.5, 0.2, -0.7], 0.5)
    T[:3, 3] = torch.tensor([0.2, 0.3, -0.15], dtype=torch.float64)
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    tgt = (xyz.double() @ T[:3, :3].T + T[:3, 3]).float() + 0.003 * torch.randn(n, 3, generator=gen)
    if outliers:
        bad = torch.randperm(n, generator=gen)[: (3 * n) // 10]
        tgt[bad] = torch.rand(len(bad), 3, generator=gen) * 3 - 1.5
    return xyz, tgt, T


@pytest.mark.parametrize("n,outliers", [(4, False), (64, False), (257, True), (5000, True)])
def test_fgr_against_float64(tp, reg, n, outliers):
    xyz, tgt, T_true = _fgr_case(n, outliers, n)
    ref32 = rr.fast_global_registration(xyz, tgt)
    ref64 = rr.fast_global_registration(xyz.double(), tgt.double())
    got = tp.fgr(xyz.to(DEV), tgt.to(DEV))
    assert got.dtype == torch.float32 and got.shape == (4, 4)
    _close64(got, ref32, ref64, 1e-4, 0.0, what="fgr N = %d" % n)
    assert torch.equal(got, reg.fast_global_registration(xyz.to(DEV), tgt.to(DEV)))
    # errors against the truth: below the float64 restatement's own plus 1e-4.  The rotation error is the chordal distance
    # |R - R_true|_F (sqrt(2) x the angle in radians for small angles), not compute_transfo_error's acos of the trace: at
    # an angle of 6e-4 rad the acos turns one fp32 ulp of T's entries (6e-8) into 1e-4 rad = 5e-3 degrees, more than the
    # allowance, for ANY pose stored in fp32
    def errors(T):
        return float((T[:3, 3] - T_true[:3, 3]).norm()), float((T[:3, :3] - T_true[:3, :3]).norm())

    (rte, rot), (rte64, rot64) = errors(got.cpu().double()), errors(ref64)
    print("N = %d: translation error %.3g (float64 restatement %.3g), |R - R_true|_F %.3g (%.3g), %.3g degrees"
          % (n, rte, rte64, rot, rot64, float(rr.compute_transfo_error(T_true, got.cpu().double())[1])))
    assert rte <= rte64 + 1e-4 and rot <= rot64 + 1e-4


def test_fgr_two_points_and_iteration_count(tp):
    xyz, tgt, _ = _fgr_case(2, False, 2)
    T = tp.fgr(xyz.to(DEV), tgt.to(DEV))
    assert bool(torch.isfinite(T).all())
    assert bool(torch.isfinite(tp.fgr(xyz[:0].to(DEV), tgt[:0].to(DEV))).all())
    xyz, tgt, _ = _fgr_case(64, False, 64)
    one = tp.fgr(xyz.to(DEV), tgt.to(DEV), num_iter=7, mu_init=0.5)
    ref32 = rr.fast_global_registration(xyz, tgt, mu_init=0.5, num_iter=7)
    ref64 = rr.fast_global_registration(xyz.double(), tgt.double(), mu_init=0.5, num_iter=7)
    _close64(one, ref32, ref64, 1e-4, 0.0, what="fgr 7 iterations")


def test_matches_kabsch_and_metrics_against_the_reference(reg, g):
    F0, F1 = g["F0"].to(DEV), g["F1"].to(DEV)
    assert torch.equal(reg.get_matches(F0, F1).cpu(), g["matches/plain"])
    assert torch.equal(reg.get_matches(F0, F1, sym=True).cpu(), g["matches/sym"])
    xyz, tgt, clean, T_true = (g[k].to(DEV) for k in ("fgr_xyz", "fgr_target", "fgr_clean", "T_true"))
    T_kabsch = reg.estimate_transfo(xyz, tgt)
    _close64(T_kabsch, g["kabsch/T"], f64(g, "kabsch/T"), 1e-4, 0.0, what="Kabsch")
    T_fgr = reg.fast_global_registration(xyz, tgt)
    _close64(T_fgr, g["fgr/T"], f64(g, "fgr/T"), 1e-4, 0.0, what="FGR")
    hit = reg.compute_hit_ratio(xyz, tgt, T_true, cfg(g, "tau_1"))
    assert float(hit) == float(g["metrics/hit_ratio"])
    # the metrics of the fixture's own fp32 pose: the formulas alone
    T_ref = g["fgr/T"].to(DEV)
    rte, rre = reg.compute_transfo_error(T_true, T_ref)
    _close64(rte, g["metrics/rte"], f64(g, "metrics/rte"), 1e-4, 0.0, what="rte")
    _close64(rre, g["metrics/rre"], f64(g, "metrics/rre"), 1e-4, 0.0, what="rre")
    sr = reg.compute_scaled_registration_error(xyz, T_true, T_ref)
    _close64(sr, g["metrics/sr_err"], f64(g, "metrics/sr_err"), 1e-4, 0.0, what="sr_err")
    assert bool(reg.compute_registration_recall(xyz, clean, T_fgr)) == bool(g["metrics/recall_fgr"])
    assert bool(reg.compute_registration_recall(xyz, clean, T_kabsch, thresh=0.02)) == bool(g["metrics/recall_kabsch"])


def test_evaluate_pair_against_the_reference(reg, g):
    got = reg.evaluate_pair(g["F0"].to(DEV), g["F1"].to(DEV), g["xyz0"].to(DEV), g["xyz1"].to(DEV), g["matches"].to(DEV),
                            num_points=cfg(g, "num_points"), tau_1=cfg(g, "tau_1"), tau_2=cfg(g, "tau_2"), rand=g["rand"].to(DEV),
                            rand_target=g["rand_target"].to(DEV))
    assert sorted(got) == ["feat_match_ratio", "hit_ratio", "rot_error", "sr_err", "trans_error"]
    assert all(v.device.type == "cuda" and v.dim() == 0 for v in got.values())
    assert float(got["hit_ratio"]) == float(g["pair/hit_ratio"]) and float(got["feat_match_ratio"]) == 1.0
    for k in ("trans_error", "rot_error", "sr_err"):
        _close64(got[k], g["pair/" + k], f64(g, "pair/" + k), 1e-4, 0.0, what=k)
    # default draws: all rows (num_points above the fragment sizes), the figures stay finite
    again = reg.evaluate_pair(g["F0"].to(DEV), g["F1"].to(DEV), g["xyz0"].to(DEV), g["xyz1"].to(DEV), g["matches"].to(DEV))
    assert all(bool(torch.isfinite(v)) for v in again.values())


def _fragment(rng, n_feat):
    """about 700 voxels of a 40 x 20 x 2 slab (six cells of the coarsest stride-16 level)"""
    cells = np.array([[x, y, z] for x in range(40) for y in range(20) for z in range(2)])
    coords = cells[rng.permutation(len(cells))[:700]]
    return types.SimpleNamespace(x=torch.from_numpy(rng.randn(len(coords), n_feat).astype(np.float32)).to(DEV),
                                 coords=torch.from_numpy(coords).int().to(DEV),
                                 batch=torch.zeros(len(coords), dtype=torch.long, device=DEV),
                                 pos=torch.from_numpy(coords.astype(np.float32) * 0.05).to(DEV))


def test_fragment_descriptor_sparse_training_step(reg):
    rng = np.random.RandomState(3)
    data, target = _fragment(rng, 3), _fragment(rng, 3)
    match = torch.from_numpy(np.stack([rng.permutation(700)[:100], rng.permutation(700)[:100]], 1)).long().to(DEV)
    torch.manual_seed(0)
    gen = torch.Generator(device=DEV)
    net = reg.FragmentDescriptor.sparse(3, in_feat=8, out_channels=16).to(DEV).train()
    twin = copy.deepcopy(net)  # the same state: parameters and running statistics
    net.metric_loss_module = twin.metric_loss_module = reg.ContrastiveHardestNegativeLoss(0.1, 1.4, num_pos=64, num_hn_samples=256,
                                                                                          generator=gen)
    losses = []
    for model in (net, twin):
        gen.manual_seed(7)
        out = model(data, target, match)
        assert out is model.output and model.output.shape == (700, 16) and model.output_target.shape == (700, 16)
        for rows in (model.output, model.output_target):
            torch.testing.assert_close(rows.norm(dim=1), torch.ones(700, device=DEV), rtol=1e-5, atol=1e-5)
        assert model.loss.dim() == 0 and bool(torch.isfinite(model.loss))
        model.loss.backward()
        losses.append(model.loss.detach().clone())
    assert torch.equal(losses[0], losses[1])
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert float(p.grad.abs().max()) > 0, name
    # inference: one fragment, no loss
    net.eval()
    with torch.no_grad():
        alone = net(data)
    assert alone.shape == (700, 16) and net.loss is None and net.output_target is None
