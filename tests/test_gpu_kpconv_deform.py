"""Deformable KPConv on the GPU (csrc/kpconv_deform.hip, torch_points3d_amd.kpconv.KPConv_deform_ops /
KPConvDeformableLayer) against the reference's own tensors (tests/golden/kpconv_deform.npz) and, at larger shapes,
against the plain-torch restatement tests/kpconv_deform_ref.py evaluated on the device (pinned to the reference by
tests/test_kpconv_deform_cpu.py).  Tolerances are the ones of the rigid tests (tests/test_gpu_kpconv.py): fixture
outputs rtol 1e-5 / atol 1e-5 * max(1, |ref|max), gradients rtol 1e-4 / atol 1e-5 * max|ref|; larger shapes rtol 1e-4.

Rows (queries) with a (neighbour, kernel point) pair within 4 fp32 ulp of d2 == extent^2 are left out of the
large-shape comparisons -- the weight, the mask or the derivative jumps there -- by zeroing their cotangents on both
sides; the tests assert that this is at most 1 % of the rows.  The fixture has no such pair (its generator asserts it)."""
import pytest
import torch

from conftest import load_golden
from kpconv_deform_ref import boundary_rows, deform_d2, torch_kpconv_deform
from test_kpconv_deform_cpu import _sub, build_dual

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INFLUENCES = ["constant", "linear", "gaussian"]


def _close(got, ref, rtol, atol_scale, floor=0.0, what=""):
    ref = torch.as_tensor(ref).to(got.device)
    atol = atol_scale * max(floor, float(ref.abs().max()))
    print("%s: max |diff| %.3g, |ref|max %.3g" % (what, float((got.detach() - ref).abs().max()), float(ref.abs().max())))
    torch.testing.assert_close(got.detach(), ref, rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


@pytest.mark.parametrize("use_mod", [False, True])
@pytest.mark.parametrize("influence", INFLUENCES)
def test_deform_ops_match_reference_fixture(influence, use_mod):
    from torch_points3d_amd.kpconv import KPConv_deform_ops
    from torch_points3d_amd.kpconv_losses import fitting_loss, repulsion_loss
    g = load_golden("kpconv_deform")
    tag = "op/%s_%s/" % (influence, "mod" if use_mod else "plain")
    infl, lam = float(g["op/extent"][0]), float(g["op/lambda"][0])
    dev = lambda k: g[k].to(DEV)  # noqa: E731
    f, w, o = (dev(k).requires_grad_(True) for k in ("op/features", "op/K_values", "op/offsets"))
    m = dev("op/modulations").requires_grad_(True) if use_mod else None
    out, kp_min, dk = KPConv_deform_ops(dev("op/query"), dev("op/support"), dev("op/neighbors"), f, dev("op/K_points"), o, m,
                                        w, infl, influence, "sum")
    _close(out, g[tag + "out"], 1e-5, 1e-5, 1.0, "out")
    _close(kp_min, g[tag + "kp_min_d2"], 1e-5, 1e-5, 1.0, "kp_min_d2")
    fit, rep = fitting_loss(kp_min, 1.5 * infl), repulsion_loss(dk, infl)
    _close(fit.reshape(1), g[tag + "fitting"], 1e-5, 1e-5, 1.0, "fitting")
    _close(rep.reshape(1), g[tag + "repulsion"], 1e-5, 1e-5, 1.0, "repulsion")
    ((out * dev("op/cot")).sum() + lam * (fit + rep)).backward()
    for name, t in (("features", f), ("K_values", w), ("offsets", o), ("modulations", m)):
        if t is not None:
            _close(t.grad, g[tag + "grad_" + name], 1e-4, 1e-5, what="grad_" + name)


@pytest.mark.parametrize("tag,modulated,loss_mode", [("layer_plain/", False, "fitting"), ("layer_mod/", True, "permissive")])
def test_deformable_layer_matches_reference_fixture(tag, modulated, loss_mode):
    from torch_points3d_amd.kpconv import KPConvDeformableLayer
    from torch_points3d_amd.kpconv_losses import internal_loss
    g = load_golden("kpconv_deform")
    sd = _sub(g, tag + "sd.")
    cin, cout = sd["weight"].shape[1:]
    layer = KPConvDeformableLayer(cin, cout, float(g[tag + "influence"][0]), sd["K_points"], modulated=modulated,
                                  loss_mode=loss_mode)
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(DEV)
    f = g[tag + "features"].to(DEV).requires_grad_(True)
    out = layer(g[tag + "query"].to(DEV), g[tag + "support"].to(DEV), g[tag + "neighbors"].to(DEV), f)
    _close(out, g[tag + "out"], 1e-5, 1e-5, 1.0, "out")
    for k, v in layer.get_internal_losses().items():
        _close(torch.as_tensor(float(v.detach() if torch.is_tensor(v) else v), device=DEV).reshape(1), g[tag + "loss." + k], 1e-5, 1e-5, 1.0, k)
    ((out * g[tag + "cot"].to(DEV)).sum() + 0.1 * internal_loss(layer)).backward()
    _close(f.grad, g[tag + "grad_features"], 1e-4, 1e-5, what="grad_features")
    grads = _sub(g, tag + "grad.")
    assert sorted(grads) == ["offset_bias", "offset_weights", "weight"]
    for k, ref in grads.items():
        _close(getattr(layer, k).grad, ref, 1e-4, 1e-5, what="grad." + k)


def test_dual_block_rigid_then_deformable_matches_reference_fixture():
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.kpconv_losses import internal_loss
    g = load_golden("kpconv_deform")
    dual = build_dual(g).to(DEV).train()
    x = g["dual/x"].to(DEV).requires_grad_(True)
    out = dual(PDData(pos=g["dual/pos"].to(DEV), batch=g["dual/batch"].to(DEV), x=x))
    ref_idx = g["dual/idx"]
    ref_idx = torch.where(ref_idx >= g["dual/pos"].shape[0], torch.full_like(ref_idx, -1), ref_idx)
    assert torch.equal(out.idx_neighboors.cpu(), ref_idx)
    _close(out.x, g["dual/out_x"], 1e-5, 1e-5, 1.0, "out_x")
    losses = dual.blocks[1].kp_conv.kp_conv.get_internal_losses()
    for k, v in losses.items():
        _close(torch.as_tensor(float(v.detach() if torch.is_tensor(v) else v), device=DEV).reshape(1), g["dual/loss." + k], 1e-5, 1e-5, 1.0, k)
    ((out.x * g["dual/cot"].to(DEV)).sum() + 0.1 * internal_loss(dual)).backward()
    _close(x.grad, g["dual/grad_x"], 1e-4, 1e-5, what="grad_x")
    params = dict(dual.named_parameters())
    grads = _sub(g, "dual/grad.")
    assert any(k.endswith("offset_weights") for k in grads) and any(k.endswith("offset_bias") for k in grads)
    for k, ref in grads.items():
        _close(params[k].grad, ref, 1e-4, 1e-5, what="grad." + k)
    state = dual.state_dict()
    for k, ref in _sub(g, "dual/after.").items():
        _close(state[k], ref, 1e-5, 1e-5, 1.0, "after." + k)


def _problem(hip, Nq, M, Mn, Cin, Cout, seed, all_shadow_row=True):
    gen = torch.Generator().manual_seed(seed)
    support = torch.rand(M, 3, generator=gen).to(DEV)
    query = support[torch.randperm(M, generator=gen)[:Nq].to(DEV)].contiguous()
    batch = torch.zeros(M, dtype=torch.long, device=DEV)
    r = 0.3 * (40.0 / M) ** (1 / 3)
    nbr, _ = hip.ball_query(r, Mn, support, query, mode="partial_dense", batch_x=batch, batch_y=batch[:Nq])
    if all_shadow_row and Nq > 1:
        nbr[Nq // 2, :] = -1  # a query whose slots are all shadows (its kp_min_d2 is 3e12: compared on its own)
    extent = r / 2.5
    kpts = ((torch.rand(15, 3, generator=gen) - 0.5) * r).to(DEV)
    return dict(query=query, support=support, nbr=nbr, extent=extent, kpts=kpts,
                feats=torch.randn(M, Cin, generator=gen).to(DEV),
                W=(torch.randn(15, Cin, Cout, generator=gen) * 0.2).to(DEV),
                offsets=(torch.randn(Nq, 15, 3, generator=gen) * (0.3 * extent)).to(DEV),
                mods=(2 * torch.sigmoid(torch.randn(Nq, 15, generator=gen))).to(DEV),
                cot=torch.randn(Nq, Cout, generator=gen).to(DEV),
                cot_min=(torch.randn(Nq, 15, generator=gen) / extent ** 2).to(DEV))


def _masked_cotangents(p, limit=0.01):
    d2, _, _ = deform_d2(p["query"], p["support"], p["nbr"], p["kpts"], p["offsets"])
    bad = boundary_rows(d2, p["extent"])
    nq = bad.numel()
    print("rows left out: %d of %d" % (int(bad.sum()), nq))
    assert int(bad.sum()) <= max(limit * nq, 0), "more than 1 %% of the rows sit on the extent boundary"
    keep = (~bad).float()[:, None]
    return p["cot"] * keep, p["cot_min"] * keep, ~bad, d2


def _run(fn, p, influence, use_mod, cot, cot_min, dtype=torch.float32, **kw):
    c = lambda t: t.to(dtype)  # noqa: E731
    f, w, o = (c(p[k]).clone().requires_grad_(True) for k in ("feats", "W", "offsets"))
    m = c(p["mods"]).clone().requires_grad_(True) if use_mod else None
    res = fn(c(p["query"]), c(p["support"]), p["nbr"], f, c(p["kpts"]), o, m, w, p["extent"], influence, **kw)
    out, kp_min = res[0], res[1]
    ((out * c(cot)).sum() + (kp_min * c(cot_min)).sum()).backward()
    rec = {"out": out.detach(), "kp_min_d2": kp_min.detach(), "grad_features": f.grad, "grad_K_values": w.grad,
           "grad_offsets": o.grad}
    if use_mod:
        rec["grad_modulations"] = m.grad
    return rec


def _hip_op(q, s, nbr, f, kp, o, m, w, extent, influence):
    from torch_points3d_amd.kpconv import KPConv_deform_ops
    return KPConv_deform_ops(q, s, nbr, f, kp, o, m, w, extent, influence, "sum")


SHAPES = [(5000, 6000, 25, 64, 128), (3000, 3000, 38, 1, 64), (700, 900, 60, 130, 70), (1, 4, 3, 5, 2),
          (65536, 65536, 25, 16, 32), (300, 400, 70, 8, 4), (900, 1000, 20, 64, 24), (900, 1000, 35, 130, 16),
          (900, 1000, 45, 1, 8), (600, 800, 70, 64, 8), (900, 1000, 30, 2, 2), (4200, 4300, 25, 130, 8)]


@pytest.mark.parametrize("influence,use_mod", [("linear", True), ("gaussian", False), ("constant", True)])
@pytest.mark.parametrize("Nq,M,Mn,Cin,Cout", SHAPES)
def test_deform_ops_match_torch_restatement(hip, Nq, M, Mn, Cin, Cout, influence, use_mod):
    """forward and all four gradients at the rigid tests' shapes plus Mn in {20, 35, 45, 70}, Cin in {1, 64, 130}, Nq = 1
    and an all-shadow query"""
    p = _problem(hip, Nq, M, Mn, Cin, Cout, seed=Nq + Mn + Cin)
    cot, cot_min, keep, _ = _masked_cotangents(p, limit=0.01 if Nq > 1 else 1.0)
    got = _run(_hip_op, p, influence, use_mod, cot, cot_min)
    ref = _run(torch_kpconv_deform, p, influence, use_mod, cot, cot_min)
    shadow = (p["nbr"] < 0).all(1)
    for k in ref:
        a, b = got[k], ref[k]
        if k in ("out", "kp_min_d2", "grad_offsets", "grad_modulations"):  # per-query quantities
            if bool(shadow.any()):
                _close(a[shadow], b[shadow], 1e-4, 1e-5, 1.0, k + " (all-shadow query)")
            a, b = a[keep & ~shadow], b[keep & ~shadow]
        if b.numel():
            _close(a, b, 1e-4, 1e-5, 1.0, k)


@pytest.mark.parametrize("influence,use_mod", [("linear", True), ("gaussian", True), ("constant", False)])
@pytest.mark.parametrize("Nq,M,Mn,Cin,Cout", [(5000, 6000, 25, 64, 128), (700, 900, 60, 130, 70), (300, 400, 70, 8, 4)])
def test_deform_ops_distance_to_float64(hip, Nq, M, Mn, Cin, Cout, influence, use_mod):
    """outputs and every gradient: rms <= 2x and max <= 4x the distance of the fp32 TORCH evaluation to the float64
    evaluation of the same restatement (the rule of tests/test_gpu_headline_fp64.py; the float64 pass takes the
    discrete in-range decisions from the fp32 distances, so it is the exact value of the same smooth pieces)"""
    p = _problem(hip, Nq, M, Mn, Cin, Cout, seed=7 + Nq)
    cot, cot_min, keep, d2 = _masked_cotangents(p)
    got = _run(_hip_op, p, influence, use_mod, cot, cot_min)
    ref32 = _run(torch_kpconv_deform, p, influence, use_mod, cot, cot_min)
    ref64 = _run(torch_kpconv_deform, p, influence, use_mod, cot, cot_min, dtype=torch.float64, decide_d2=d2)
    failures = []
    for k, want in ref64.items():
        a, b = got[k].double(), ref32[k].double()
        if k in ("out", "kp_min_d2", "grad_offsets", "grad_modulations"):
            rows = keep & ~(p["nbr"] < 0).all(1)  # (the all-shadow query's 3e12 distances would set the scale)
            a, b, want = a[rows], b[rows], want[rows]
        eps = max(1.0, float(want.abs().max()))
        rms_g, max_g = float((a - want).pow(2).mean().sqrt()), float((a - want).abs().max())
        rms_c, max_c = float((b - want).pow(2).mean().sqrt()), float((b - want).abs().max())
        print("%s: HIP rms %.3g max %.3g | torch fp32 rms %.3g max %.3g" % (k, rms_g, max_g, rms_c, max_c))
        if rms_g > 2.0 * rms_c + 1e-8 * eps:
            failures.append("%s: rms |HIP-f64| %.3g vs |torch32-f64| %.3g" % (k, rms_g, rms_c))
        if max_g > 4.0 * max_c + 1e-7 * eps:
            failures.append("%s: max |HIP-f64| %.3g vs |torch32-f64| %.3g" % (k, max_g, max_c))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("Mn", [25, 70])
def test_backward_is_bitwise_reproducible(hip, Mn):
    p = _problem(hip, 2000, 2500, Mn, 70, 40, seed=3)
    a = _run(_hip_op, p, "linear", True, p["cot"], p["cot_min"])
    b = _run(_hip_op, p, "linear", True, p["cot"], p["cot_min"])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_rigid_block_is_the_rigid_kernel(hip):
    """deformable=False builds the layer and runs the kernel it always did: same bits as a direct KPConv_ops call"""
    from torch_points3d_amd.kpconv import KPConv_ops, KPConvLayer
    from torch_points3d_amd.kpconv_blocks import PDData, SimpleBlock
    gen = torch.Generator().manual_seed(1)
    N = 3000
    pos = torch.rand(N, 3, generator=gen).to(DEV)
    batch = torch.zeros(N, dtype=torch.long, device=DEV)
    x = torch.randn(N, 8, generator=gen).to(DEV)
    blk = SimpleBlock(down_conv_nn=[8, 16], grid_size=0.05, prev_grid_size=0.05, max_num_neighbors=20, deformable=False,
                      bn=None, activation=torch.nn.Identity()).to(DEV)
    assert type(blk.kp_conv) is KPConvLayer
    out = blk(PDData(pos=pos, batch=batch, x=x))
    nbr = hip.ball_query(2.5 * 0.05, 20, pos, pos, mode="partial_dense", batch_x=batch, batch_y=batch)[0]
    ref = KPConv_ops(pos, pos, nbr, x, blk.kp_conv.K_points, blk.kp_conv.weight, 0.05, "linear", "sum")
    assert torch.equal(out.x, ref)


def test_hub_support_point_backward_deformable(hip):
    """a support point referenced by 12 000 slots (as tests/test_gpu_kpconv.py::test_hub_support_point_backward)"""
    gen = torch.Generator().manual_seed(12)
    M, Nq, Mn, Cin, Cout = 400, 3000, 12, 8, 6
    nbr = torch.randint(0, M, (Nq, Mn), generator=gen)
    nbr[:, 3:7] = 17
    nbr[::5, 9:] = -1
    p = dict(query=torch.rand(Nq, 3, generator=gen).to(DEV), support=torch.rand(M, 3, generator=gen).to(DEV),
             nbr=nbr.to(DEV), extent=0.2, kpts=((torch.rand(15, 3, generator=gen) - 0.5) * 0.3).to(DEV),
             feats=torch.randn(M, Cin, generator=gen).to(DEV), W=(torch.randn(15, Cin, Cout, generator=gen) * 0.2).to(DEV),
             offsets=(torch.randn(Nq, 15, 3, generator=gen) * 0.05).to(DEV),
             mods=(2 * torch.sigmoid(torch.randn(Nq, 15, generator=gen))).to(DEV),
             cot=torch.randn(Nq, Cout, generator=gen).to(DEV), cot_min=torch.zeros(Nq, 15, device=DEV))
    cot, cot_min, _, _ = _masked_cotangents(p)
    got = _run(_hip_op, p, "linear", True, cot, cot_min)
    ref = _run(torch_kpconv_deform, p, "linear", True, cot, cot_min)
    _close(got["grad_features"], ref["grad_features"], 1e-4, 1e-5, 1.0, "grad_features")
    again = _run(_hip_op, p, "linear", True, cot, cot_min)
    assert torch.equal(got["grad_features"], again["grad_features"])
