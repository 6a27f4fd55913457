"""PosPool / PPNet on the GPU (csrc/pospool.hip, torch_points3d_amd.ppnet) against the reference's own tensors
(tests/golden/ppnet.npz) and, past the first tile, against the plain-torch restatement tests/ppnet_ref.py evaluated in
float64 on the device (pinned to the reference by tests/test_ppnet_cpu.py).

Bars.  xyz outputs: the KPConv tests' rtol 1e-5 / atol 1e-5 * max(1, |ref|max); gradients rtol 1e-4 / atol 1e-5 * |ref|max.
sin_cos feeds arguments of up to ~100 rad and more to the sine: one fp32 ulp of the argument is ~8e-6 of the result, so
two correct fp32 evaluations differ by more than the bar above.  There the distance is measured against float64:
    |hip - ref64|max <= max(the bar above, 2 * |ref32 - ref64|max)
with ref32 / ref64 the reference's own two evaluations (fixture) or the restatement's (larger shapes); the factor 2 lets
two independent fp32 roundings of an argument fall on opposite sides.  Every comparison prints both distances."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from ppnet_ref import pospool_ref
from test_ppnet_cpu import OP_CASES, _sub, build_stage, build_strided, op_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(v):
    return torch.from_numpy(v) if isinstance(v, np.ndarray) else v


def _close(got, ref, rtol, atol_scale, floor=0.0, what=""):
    ref = _t(ref).to(got.device)
    atol = atol_scale * max(floor, float(ref.abs().max()))
    print("%s: max |diff| %.3g, |ref|max %.3g" % (what, float((got.detach() - ref).abs().max()), float(ref.abs().max())))
    torch.testing.assert_close(got.detach(), ref, rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


def _close64(got, ref32, ref64, rtol, atol_scale, floor=0.0, what=""):
    """|got - ref64| <= max(atol + rtol |ref64|, 2 |ref32 - ref64|max), element-wise"""
    ref64 = _t(ref64).to(got.device).double()
    ref32 = _t(ref32).to(got.device).double()
    if ref64.numel() == 0:
        return
    err = (got.detach().double() - ref64).abs()
    own = float((ref32 - ref64).abs().max())
    bar = atol_scale * max(floor, float(ref64.abs().max())) + rtol * ref64.abs()
    print("%s: |hip - ref64|max %.3g, |ref32 - ref64|max %.3g, |ref|max %.3g" % (what, float(err.max()), own,
                                                                                float(ref64.abs().max())))
    worst = float((err - torch.clamp(bar, min=2.0 * own)).max())
    assert worst <= 0.0, "%s: |hip - ref64| exceeds max(bar, 2 |ref32 - ref64|max = %.3g) by %.3g" % (what, 2.0 * own, worst)


def _hip(q, s, nbr, x, cot, radius, embedding, reduction):
    from torch_points3d_amd.ppnet import pospool
    f = x.clone().requires_grad_(True)
    before = nbr.clone()
    out = pospool(q, s, nbr, f, radius, embedding, reduction)
    (out * cot).sum().backward()
    assert torch.equal(nbr, before)  # the caller's table keeps its -1 entries
    return out.detach(), f.grad


def _check_fixture(g, tag, embedding, out, grad):
    if embedding == "xyz":
        _close(out, g[tag + "out"], 1e-5, 1e-5, 1.0, "out")
        _close(grad, g[tag + "grad_features"], 1e-4, 1e-5, what="grad_features")
    else:
        _close64(out, g[tag + "out"], g[tag + "out64"], 1e-5, 1e-5, 1.0, "out")
        _close64(grad, g[tag + "grad_features"], g[tag + "grad_features64"], 1e-4, 1e-5, what="grad_features")


@pytest.mark.parametrize("reduction", ["sum", "avg"])
@pytest.mark.parametrize("embedding,C", OP_CASES)
def test_operator_matches_reference_fixture(embedding, C, reduction):
    g = load_golden("ppnet")
    q, s, nbr, x, cot, radius = (v.to(DEV) if torch.is_tensor(v) else v for v in op_inputs(g, "op/neighbors", embedding, C))
    out, grad = _hip(q, s, nbr, x, cot, radius, embedding, reduction)
    _check_fixture(g, "op/%s%d_%s/" % (embedding, C, reduction), embedding, out, grad)


@pytest.mark.parametrize("embedding", ["xyz", "sin_cos"])
def test_count_rule_without_shadows_matches_reference_fixture(embedding):
    g = load_golden("ppnet")
    q, s, nbr, x, cot, radius = (v.to(DEV) if torch.is_tensor(v) else v for v in op_inputs(g, "full/neighbors", "sin_cos", 12))
    out, grad = _hip(q, s, nbr, x, cot, radius, embedding, "avg")
    _check_fixture(g, "full/%s12_avg/" % embedding, embedding, out, grad)


def _check_module(g, tag, module, out, x):
    """sin_cos blocks: every compared tensor against the reference's float64 pass, the bar of the module docstring"""
    M = g[tag + "pos"].shape[0]
    ref_idx = g[tag + "idx"]
    ref_idx = torch.where(ref_idx >= M, torch.full_like(ref_idx, -1), ref_idx)
    assert torch.equal(out.idx_neighboors.cpu(), ref_idx)
    _close64(out.x, g[tag + "out_x"], g[tag + "f64/out_x"], 1e-5, 1e-5, 1.0, "out_x")
    (out.x * g[tag + "cot"].to(DEV)).sum().backward()
    _close64(x.grad, g[tag + "grad_x"], g[tag + "f64/grad_x"], 1e-4, 1e-5, what="grad_x")
    params = dict(module.named_parameters())
    grads = _sub(g, tag + "grad.")
    assert set(grads) == set(params)
    failures = []
    for k, ref in grads.items():
        try:
            _close64(params[k].grad, ref, g[tag + "f64/grad." + k], 1e-4, 1e-5, what="grad." + k)
        except AssertionError as e:
            failures.append(str(e))
    state = module.state_dict()
    for k, ref in _sub(g, tag + "after.").items():
        _close64(state[k], ref, g[tag + "f64/after." + k], 1e-5, 1e-5, 1.0, "after." + k)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("fused", [True, False])
def test_stage_block_matches_reference_fixture(fused):
    from torch_points3d_amd.kpconv_blocks import PDData
    g = load_golden("ppnet")
    stage = build_stage(g, fused=fused).to(DEV).train()
    x = g["stage/x"].to(DEV).requires_grad_(True)
    out = stage(PDData(pos=g["stage/pos"].to(DEV), batch=g["stage/batch"].to(DEV), x=x))
    _check_module(g, "stage/", stage, out, x)


def test_strided_block_on_precomputed_query_data_matches_reference_fixture():
    from torch_points3d_amd.kpconv_blocks import PDData
    g = load_golden("ppnet")
    block = build_strided(g).to(DEV).train()
    x = g["strided/x"].to(DEV).requires_grad_(True)
    table = g["strided/neighbors"].to(DEV)
    pre = [PDData(pos=g["strided/q_pos"].to(DEV), batch=g["strided/q_batch"].to(DEV), idx_neighboors=table)]
    out = block(PDData(pos=g["strided/pos"].to(DEV), batch=g["strided/batch"].to(DEV), x=x, block_idx=0), precomputed=pre)
    assert out.x.shape[0] == table.shape[0] and torch.equal(table.cpu(), g["strided/neighbors"])
    _check_module(g, "strided/", block, out, x)


# ------------------------------------------------------------------------------------------- beyond the first tile
def _problem(hip, Nq, M, Mn, C, seed, shadows=True):
    gen = torch.Generator().manual_seed(seed)
    support = torch.rand(M, 3, generator=gen).to(DEV)
    query = support[torch.randperm(M, generator=gen)[:Nq].to(DEV)].contiguous()
    batch = torch.zeros(M, dtype=torch.long, device=DEV)
    r = 0.3 * (40.0 / M) ** (1 / 3)
    if shadows:
        nbr, _ = hip.ball_query(r, Mn, support, query, mode="partial_dense", batch_x=batch, batch_y=batch[:Nq])
        if Mn > 1:
            nbr[:, 1] = 7  # one support point in every row: a long list of the inverted table
        if Nq > 1:
            nbr[Nq // 2, :] = -1  # a query whose slots are all shadows
    else:
        nbr = torch.randint(0, M, (Nq, Mn), generator=gen).to(DEV)
        nbr[0, 0] = M - 1
    return dict(q=query, s=support, nbr=nbr, radius=r, x=torch.randn(M, C, generator=gen).to(DEV),
                cot=torch.randn(Nq, C, generator=gen).to(DEV))


def _ref(p, embedding, reduction, dtype):
    f = p["x"].to(dtype).clone().requires_grad_(True)
    out = pospool_ref(p["q"].to(dtype), p["s"].to(dtype), p["nbr"], f, p["radius"], embedding, reduction)
    (out * p["cot"].to(dtype)).sum().backward()
    return out.detach(), f.grad


# every Nq in {1, 257, 5003}, C in {9, 36, 390 (F = 65: crosses a wave), 1152}, Mn in {1, 26, 41}; 16-, 64-lane groups,
# channel loops, channel passes spread over the grid's y (few rows, C > 64) and not (C = 36; 5003 rows of xyz at C = 390
# backward, 9000 support rows); C = 9 stays at 257 queries: torch's restatement needs 12 s per case at 5003 x 26 x 9
SHAPES = [(1, 40, 1, 9), (257, 300, 26, 36), (5003, 5200, 41, 390), (257, 300, 41, 1152), (257, 5200, 26, 9),
          (5003, 6000, 1, 36), (1, 50, 26, 1152), (257, 9000, 26, 390)]


@pytest.mark.parametrize("embedding,reduction", [("sin_cos", "avg"), ("sin_cos", "sum"), ("xyz", "avg"), ("xyz", "sum")])
@pytest.mark.parametrize("Nq,M,Mn,C", SHAPES)
def test_operator_distance_to_float64(hip, Nq, M, Mn, C, embedding, reduction):
    p = _problem(hip, Nq, M, Mn, C, seed=Nq + Mn + C)
    out, grad = _hip(p["q"], p["s"], p["nbr"], p["x"], p["cot"], p["radius"], embedding, reduction)
    out32, grad32 = _ref(p, embedding, reduction, torch.float32)
    out64, grad64 = _ref(p, embedding, reduction, torch.float64)
    if Nq > 1:
        assert float(out[Nq // 2].abs().max()) == 0.0  # the all-shadow query
    _close64(out, out32, out64, 1e-5, 1e-5, 1.0, "out")
    _close64(grad, grad32, grad64, 1e-4, 1e-5, what="grad_features")


@pytest.mark.parametrize("embedding", ["sin_cos", "xyz"])
def test_count_rule_without_shadows_distance_to_float64(hip, embedding):
    p = _problem(hip, 257, 300, 26, 36, seed=5, shadows=False)
    assert int(p["nbr"].min()) >= 0
    out, grad = _hip(p["q"], p["s"], p["nbr"], p["x"], p["cot"], p["radius"], embedding, "avg")
    out32, grad32 = _ref(p, embedding, "avg", torch.float32)
    out64, grad64 = _ref(p, embedding, "avg", torch.float64)
    _close64(out, out32, out64, 1e-5, 1e-5, 1.0, "out")
    _close64(grad, grad32, grad64, 1e-4, 1e-5, what="grad_features")


@pytest.mark.parametrize("Nq,M,Mn,C,embedding", [(5003, 5200, 26, 36, "sin_cos"), (257, 300, 41, 1152, "sin_cos"),
                                                 (5003, 5200, 26, 9, "xyz")])  # (16-lane groups at 5003 rows)
def test_forward_and_backward_are_bitwise_reproducible(hip, Nq, M, Mn, C, embedding):
    p = _problem(hip, Nq, M, Mn, C, seed=3)
    a = _hip(p["q"], p["s"], p["nbr"], p["x"], p["cot"], p["radius"], embedding, "avg")
    b = _hip(p["q"], p["s"], p["nbr"].clone(), p["x"], p["cot"], p["radius"], embedding, "avg")  # (a new inverted table)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_reduced_width_net_trains_and_fused_paths_agree():
    """PPNet at in_feat = 12 on two clouds of ~2k points: finite forward, loss and backward, a non-zero gradient on every
    parameter, and the module graph (fused=False) agreeing with the fused kernels to 1e-5 (rtol and plain atol)"""
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.ppnet import PPNet
    gen = torch.Generator().manual_seed(21)
    N, classes = 4000, 5
    pos = torch.rand(N, 3, generator=gen).to(DEV)
    batch = torch.sort(torch.randint(0, 2, (N,), generator=gen))[0].to(DEV)
    x = torch.randn(N, 4, generator=gen).to(DEV)
    y = torch.randint(0, classes, (N,), generator=gen).to(DEV)
    torch.manual_seed(2)
    nets = [PPNet(4, classes, 0.03, in_feat=12, fused=fused) for fused in (True, False)]
    nets[1].load_state_dict(nets[0].state_dict(), strict=True)
    outs = []
    for net in nets:
        net.to(DEV).train()
        out = net(PDData(pos=pos, batch=batch, x=x))
        assert out.shape == (N, classes) and bool(torch.isfinite(out).all())
        loss = torch.nn.functional.nll_loss(out, y)
        loss.backward()
        assert bool(torch.isfinite(loss))
        for k, prm in net.named_parameters():
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
            assert float(prm.grad.abs().max()) > 0.0, k
        outs.append(out.detach())
    print("fused vs module graph: max |diff| %.3g, |ref|max %.3g" % (float((outs[0] - outs[1]).abs().max()),
                                                                     float(outs[1].abs().max())))
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-5, atol=1e-5)
