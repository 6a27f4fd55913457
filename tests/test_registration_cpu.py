"""Registration without a GPU: the plain-torch restatement (tests/registration_ref.py) is held to the fixture the reference's
own code produced (tests/golden/registration.npz), in fp32 and in float64; the fixture's safety conditions are checked
again; the product refuses CPU tensors; the head carries FragmentKPConv's parameter names."""
import numpy as np
import pytest
import torch

import registration_ref as rr
from conftest import load_golden

RELU_MARGIN = 5e-5
GAP_MARGIN = 1e-4
TOL = {torch.float32: dict(rtol=1e-5, atol=1e-6), torch.float64: dict(rtol=1e-9, atol=1e-11)}


@pytest.fixture(scope="module")
def g():
    return load_golden("registration")


def cfg(g, name):
    return g["config/" + name].reshape(-1)[0].item()


def want(g, key, dtype):
    """the fixture's entry for the dtype of the pass, as a tensor"""
    v = g[key] if dtype == torch.float32 else g["f64/" + key]
    return v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))


def cast(g, key, dtype):
    return g[key].to(dtype).detach().clone()


def close(got, ref, dtype, what):
    torch.testing.assert_close(got.detach().to(dtype), ref.to(dtype).reshape(got.shape), msg=lambda m: what + ": " + m, **TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hardest_negative_restatement_matches_reference(g, dtype):
    F0, F1 = cast(g, "F0", dtype).requires_grad_(True), cast(g, "F1", dtype).requires_grad_(True)
    loss = rr.hardest_negative_loss(F0, F1, g["matches"], g["sel0"], g["sel1"], g["pos_sel"], cfg(g, "pos_thresh"),
                                    cfg(g, "neg_thresh"), cfg(g, "num_pos"))
    loss.backward()
    close(loss, want(g, "hn/loss", dtype), dtype, "loss")
    close(F0.grad, want(g, "hn/dF0", dtype), dtype, "dF0")
    close(F1.grad, want(g, "hn/dF1", dtype), dtype, "dF1")
    assert float(F0.grad.abs().max()) > 0 and float(F1.grad.abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_hard_restatement_matches_reference(g, dtype):
    F0, F1 = cast(g, "F0", dtype).requires_grad_(True), cast(g, "F1", dtype).requires_grad_(True)
    loss = rr.batch_hard_loss(F0, F1, g["matches"], cast(g, "xyz0", dtype), cfg(g, "bh_pos_thresh"), cfg(g, "bh_neg_thresh"),
                              cfg(g, "bh_min_dist"))
    loss.backward()
    close(loss, want(g, "bh/loss", dtype), dtype, "loss")
    close(F0.grad, want(g, "bh/dF0", dtype), dtype, "dF0")
    close(F1.grad, want(g, "bh/dF1", dtype), dtype, "dF1")


def test_safety_conditions_hold(g):
    F0, F1, xyz0 = g["F0"].double(), g["F1"].double(), g["xyz0"].double()
    hn = rr.hardest_negative_parts(F0, F1, g["matches"], g["sel0"], g["sel1"], g["pos_sel"], cfg(g, "pos_thresh"),
                                   cfg(g, "neg_thresh"), cfg(g, "num_pos"))
    bh = rr.batch_hard_parts(F0, F1, g["matches"], xyz0, cfg(g, "bh_pos_thresh"), cfg(g, "bh_neg_thresh"), cfg(g, "bh_min_dist"))
    assert float(hn["relu_args"].abs().min()) >= RELU_MARGIN and float(bh["relu_args"].abs().min()) >= RELU_MARGIN
    assert min(float(hn["gap01"].min()), float(hn["gap10"].min()), float(bh["gap"].min())) >= GAP_MARGIN
    # both sides of every relu and of every mask are exercised
    for parts in (hn, bh):
        assert bool((parts["relu_args"] > 0).any()) and bool((parts["relu_args"] < 0).any())
    for m in (hn["mask0"], hn["mask1"]):
        assert 0 < int(m.sum()) < m.numel()
    assert len(g["pos_sel"]) == cfg(g, "num_pos") < len(g["matches"])
    assert bool((bh["idx"] >= 0).all())
    # the exclusion is nowhere near its threshold: the fp32 and float64 masks are the same pairs
    sub = g["xyz0"][g["matches"][:, 0]]
    d = rr.pdist(sub.double(), sub.double())
    assert float((d - cfg(g, "bh_min_dist")).abs().min()) > 5e-3
    assert bool((d <= cfg(g, "bh_min_dist")).sum() > len(sub))  # pairs other than (i, i) are excluded too


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_matching_pose_and_metrics_match_reference(g, dtype):
    F0, F1 = cast(g, "F0", dtype), cast(g, "F1", dtype)
    for key, sym in (("matches/plain", False), ("matches/sym", True)):
        assert torch.equal(rr.get_matches(F0, F1, sym=sym), want(g, key, dtype).long())
    assert 0 < len(g["matches/sym"]) < len(g["matches/plain"]) == len(F0)
    xyz, tgt, clean = cast(g, "fgr_xyz", dtype), cast(g, "fgr_target", dtype), cast(g, "fgr_clean", dtype)
    T_true = cast(g, "T_true", dtype)
    T_kabsch, T_fgr = rr.estimate_transfo(xyz, tgt), rr.fast_global_registration(xyz, tgt)
    close(T_kabsch, want(g, "kabsch/T", dtype), dtype, "Kabsch")
    close(T_fgr, want(g, "fgr/T", dtype), dtype, "FGR")
    close(rr.compute_hit_ratio(xyz, tgt, T_true, cfg(g, "tau_1")), want(g, "metrics/hit_ratio", dtype), dtype, "hit ratio")
    rte, rre = rr.compute_transfo_error(T_true, T_fgr)
    close(rte, want(g, "metrics/rte", dtype), dtype, "rte")
    close(rre, want(g, "metrics/rre", dtype), dtype, "rre")
    close(rr.compute_scaled_registration_error(xyz, T_true, T_fgr), want(g, "metrics/sr_err", dtype), dtype, "sr_err")
    assert rr.compute_registration_recall(xyz, clean, T_fgr) == bool(want(g, "metrics/recall_fgr", dtype))
    assert rr.compute_registration_recall(xyz, clean, T_kabsch, thresh=0.02) == bool(want(g, "metrics/recall_kabsch", dtype))


def test_fixture_case_is_what_it_claims(g):
    """30 % outliers: FGR recovers the pose, Kabsch does not"""
    T_true = g["T_true"].double()
    rte_f, rre_f = rr.compute_transfo_error(T_true, torch.from_numpy(g["f64/fgr/T"]))
    rte_k, rre_k = rr.compute_transfo_error(T_true, torch.from_numpy(g["f64/kabsch/T"]))
    assert float(rte_f) < 0.01 and float(rre_f) < 0.5
    assert float(rte_k) > 5 * float(rte_f) and float(rre_k) > 5 * float(rre_f)
    assert abs(float(g["metrics/hit_ratio"]) - 0.7) < 0.02
    assert bool(g["metrics/recall_fgr"]) and not bool(g["metrics/recall_kabsch"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pair_evaluation_matches_reference(g, dtype):
    got = rr.evaluate_pair(cast(g, "F0", dtype), cast(g, "F1", dtype), cast(g, "xyz0", dtype), cast(g, "xyz1", dtype),
                           g["matches"], g["rand"], g["rand_target"], cfg(g, "tau_1"), cfg(g, "tau_2"))
    for k, v in got.items():
        close(v, want(g, "pair/" + k, dtype), dtype, k)
    assert float(got["hit_ratio"]) > 0.2 and float(got["feat_match_ratio"]) == 1.0


def test_product_refuses_cpu_tensors():
    from torch_points3d_amd import registration as reg
    from torch_points3d_amd import torchpoints as tp
    a, b = torch.rand(5, 8), torch.rand(7, 8)
    pairs = torch.tensor([[0, 1], [2, 3], [4, 5]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.feature_nn(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.gather_rows(a, torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.fgr(torch.rand(6, 3), torch.rand(6, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.ContrastiveHardestNegativeLoss(0.1, 1.4)(a, b, pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.BatchHardContrastiveLoss(0.1, 1.4)(a, b, pairs, torch.rand(5, 3), torch.rand(7, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.get_matches(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.fast_global_registration(torch.rand(6, 3), torch.rand(6, 3))


def test_argument_errors():
    from torch_points3d_amd import torchpoints as tp
    a = torch.rand(5, 8)
    with pytest.raises(ValueError):
        tp.feature_nn(a, a, pos_a=torch.rand(5, 3))  # positions without min_dist
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.feature_nn(a, a, torch.rand(5, 3), torch.rand(5, 3), 0.1)


def test_pdist_is_the_reference_formula():
    from torch_points3d_amd.registration import pdist
    A, B = torch.rand(6, 5, dtype=torch.float64), torch.rand(4, 5, dtype=torch.float64)
    D2 = ((A[:, None] - B[None]) ** 2).sum(2)
    assert torch.equal(pdist(A, B, "SquareL2"), D2) and torch.equal(pdist(A, B), torch.sqrt(D2 + 1e-7))
    with pytest.raises(NotImplementedError):
        pdist(A, B, "L1")


def test_head_carries_the_reference_names():
    from torch_points3d_amd.registration import FragmentDescriptor

    class Backbone(torch.nn.Module):
        output_nc = 12

    net = FragmentDescriptor(Backbone(), [12, 16, 20], out_channels=32, dropout=0.5)
    keys = [k for k in net.state_dict() if k.startswith("FC_layer")]
    expect = ["FC_layer.1.0.weight", "FC_layer.2.0.weight", "FC_layer.Last.weight"]
    for i in (1, 2):
        expect += ["FC_layer.%d.1.batch_norm.%s" % (i, n) for n in ("weight", "bias", "running_mean", "running_var",
                                                                    "num_batches_tracked")]
    assert sorted(keys) == sorted(expect)
    assert tuple(net.FC_layer.Last.weight.shape) == (32, 20) and tuple(net.FC_layer[0][0].weight.shape) == (16, 12)
    assert [type(m).__name__ for m in net.FC_layer] == ["Sequential", "Sequential", "Dropout", "Linear"]
    assert isinstance(net.FC_layer[0][2], torch.nn.LeakyReLU) and net.FC_layer[0][2].negative_slope == 0.2
    assert net.FC_layer[0][1].batch_norm.momentum == 0.02
    with pytest.raises(ValueError):
        FragmentDescriptor(Backbone(), [13, 16])
    sparse = FragmentDescriptor.sparse(3)
    assert sparse.eps == 1e-20 and sparse.out_channels == 32
    assert "FC_layer.1.0.weight" in sparse.state_dict() and any(k.startswith("backbone.down_modules") for k in sparse.state_dict())
