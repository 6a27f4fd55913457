"""The shipped training step at the size bench.py measures, against float64.

unet_3_ss at B=32, N=16384 (FEAT=3, 10 classes; bench.make_inputs seed 1234, bench.build_model weights seed 0): the first
set-abstraction MLP has 32 * 512 * 64 = 1 048 576 rows, so every form of the fused layer chain runs (bf16-pipe forward and
weight-gradient kernels, split-role input-gradient kernels with dY formed in their loader waves, pooled and dense, the
narrow first-layer pair, alternating row directions).  And config 3 (PointNet2_D, charlesmsg, B=32, N=2048), whose 132 /
196 / 260-wide layers and nsample-32 / 128 pooled layers take the library-GEMM fallbacks.

Two host references per network, built once per module on the same weights and cloud, train mode, one backward pass each:
`ref64` is the reference graph (fused=False) evaluated in double through tests/fp64_kernels.py (the oracle's indices on
the fp32 coordinates, every feature operation in double); `ref32` is the same graph in fp32 on the CPU oracle, an
independent fp32 implementation.  The bar for the HIP step is "no further from float64 than the independent fp32 pass":
LeakyReLU kinks and max-pool arg-max switches make element-wise gradient checks impossible at this size, and two fp32
evaluations legitimately differ there.  Measured distances and ratios go to the parity report (section headline_fp64)."""
import gc
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import fp64_kernels
from golden_util import report
from oracle import tpk_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, N, NCLS = 32, 16384, 10
C3_B, C3_N, C3_CLS, C3_CATS = 32, 2048, 50, 16
# relative-L2 floor of the gradient rule (||g - g64|| <= 2 * ||g32 - g64|| + FLOOR * ||g64||): well below what a dropped
# 32-row block of a layer's rows does to its gradient (sqrt(32 / rows): 5.5e-3 at the 1 M-row layers, 1.1e-2 at 262 144)
GRAD_FLOOR = 1e-3
SECTION = "headline_fp64"
STAT_RTOL = 1e-5


# ---------------------------------------------------------------------------------------------------- host references

def _unet(kernels=None, fused=True):
    from torch_points3d_amd.pointnet2 import PointNet2Unet
    return PointNet2Unet(3, output_nc=NCLS, config="unet_3_ss", kernels=kernels, fused=fused)


def _c3(kernels=None, fused=True):
    from torch_points3d_amd.pointnet2 import PointNet2_D
    net = PointNet2_D(3, C3_CLS, config="pointnet2_charlesmsg", num_categories=C3_CATS, kernels=kernels, fused=fused)
    return net


def _train(net):
    """train mode with the classifier's Dropout (config 3) off: host and device would draw different masks"""
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return net


def _stage_modules(net):
    from torch_points3d_amd.pointnet2 import PointNet2_D
    if isinstance(net, PointNet2_D):
        return net.stages()
    return list(net.down_modules), net.inner_modules[0], list(net.up_modules)


def _forward(net, pos, x, category=None, geometry=None):
    """whole forward pass with the stage outputs captured (keys of golden_util.run_stages); out_x = the class scores"""
    from torch_points3d_amd.dense import Data
    rec, hooks = {}, []
    downs, inner, ups = _stage_modules(net)
    for i, m in enumerate(downs):
        hooks.append(m.register_forward_hook(
            lambda mod, inp, out, i=i: rec.update({"down%d_x" % i: out.x, "down%d_pos" % i: out.pos})))
    hooks.append(inner.register_forward_hook(lambda mod, inp, out: rec.update({"inner_x": out.x})))
    for i, m in enumerate(ups):
        hooks.append(m.register_forward_hook(lambda mod, inp, out, i=i: rec.update({"up%d_x" % i: out.x})))
    try:
        if category is None:
            rec["out_x"] = net(Data(pos=pos, x=x), geometry=geometry).x
        else:
            rec["out_x"] = net(Data(pos=pos, x=x), category, geometry=geometry)
    finally:
        for h in hooks:
            h.remove()
    return rec


def _loss(out, y):
    """bench.seg_loss: cross entropy over every point (scores (B, classes, N), or (B*N, classes) for config 3)"""
    return F.cross_entropy(out, y if out.dim() == 3 else y.reshape(-1))


def _buffers(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items() if "running_" in k}


def _reference_pass(make, kernels, dtype, sd, pos, x, y, category, after=None):
    """one train step (forward, loss, backward) of the reference graph in `dtype`, then -- with the running statistics
    `after` loaded -- one eval pass.  Returns stage outputs, gradients, buffers after the step, eval stage outputs."""
    net = make(kernels=kernels, fused=False)
    net.load_state_dict(sd)
    net = _train(net.to(dtype))
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    p = pos.to(dtype)
    rec = _forward(net, p, xi, category)
    _loss(rec["out_x"], y).backward()
    out = {"train": {k: v.detach() for k, v in rec.items()},
           "grad": dict([("x", xi.grad)] + [(k, q.grad) for k, q in net.named_parameters() if q.grad is not None]),
           "after": _buffers(net)}
    del rec, xi
    gc.collect()
    if after is None:
        after = {k: v.float() for k, v in out["after"].items()}
    sd2 = net.state_dict()
    for k, v in after.items():
        sd2[k].copy_(v.to(sd2[k].dtype))
    net.eval()
    with torch.no_grad():
        out["eval"] = {k: v.detach() for k, v in _forward(net, p, x.to(dtype), category).items()}
    return out, after


def _errors(a, b):
    e = a.double() - b
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())


def _grad_ref_norm(k, grads):
    """norm a gradient's error is measured against: its own, and for a BatchNorm bias (a sum with cancellation, the two
    in front of a max-pool especially) at least its layer's BatchNorm weight gradient (as test_gpu_fused.py does)"""
    ref = float(grads[k].norm())
    if k.endswith(".bias") and k[:-4] + "weight" in grads:
        ref = max(ref, float(grads[k[:-4] + "weight"].norm()))
    return ref


def _build_references(make, sd, pos, x, y, category):
    fp64_kernels.limit_threads()
    r64, after = _reference_pass(make, fp64_kernels, torch.float64, sd, pos, x, y, category)
    gc.collect()
    r32, _ = _reference_pass(make, tpk_ref, torch.float32, sd, pos, x, y, category, after=after)
    gc.collect()
    todev = lambda d: {k: v.to(DEV) for k, v in d.items()}  # noqa: E731
    ref = {"r64": {m: todev(r64[m]) for m in ("train", "grad", "after", "eval")},
           "r32": {m: todev(r32[m]) for m in ("train", "grad", "after", "eval")},
           "after": todev(after), "pos": pos, "x": x, "y": y, "category": category, "sd": sd}
    # the bars: the independent fp32 pass's own distance to float64
    ref["bar"] = {
        "train": {k: _errors(v, ref["r64"]["train"][k]) for k, v in ref["r32"]["train"].items() if k.endswith("_x")},
        "eval": {k: _errors(v, ref["r64"]["eval"][k]) for k, v in ref["r32"]["eval"].items() if k.endswith("_x")},
        "grad": {k: float((v.double() - ref["r64"]["grad"][k]).norm()) / _grad_ref_norm(k, ref["r64"]["grad"])
                 for k, v in ref["r32"]["grad"].items()}}
    return ref


@pytest.fixture(scope="module")
def headline():
    """ref64 / ref32 of the BASELINE step: bench.make_inputs(32, 16384, seed 1234), bench.build_model weights (seed 0)"""
    import bench
    pos, x, y = bench.make_inputs(B, N, 1234, "cpu")
    sd = {k: v.clone() for k, v in bench.build_model(None, "cpu").net.state_dict().items()}
    ref = _build_references(_unet, sd, pos, x, y, None)
    oracle = {}
    cur = pos
    from torch_points3d_amd.pointnet2 import unet_config
    cfg = unet_config("unet_3_ss", 3)
    positions = [pos]
    for i in range(len(cfg["npoint"])):
        fps = tpk_ref.furthest_point_sample(cur, cfg["npoint"][i])
        new = cur.gather(1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        oracle["down%d_fps" % i] = fps
        oracle["down%d_ball" % i] = tpk_ref.ball_query(cfg["radii"][i][0], cfg["nsample"][i][0], cur, new)[0]
        cur = new
        positions.append(cur)
    for j in range(1, len(cfg["up_conv_nn"])):  # up0 sits below the global module (no 3-NN table)
        oracle["up%d_nn" % j] = tpk_ref.three_nn(positions[-j - 1], positions[-j])[1]
    ref["oracle"] = oracle
    return ref


@pytest.fixture(scope="module")
def config3():
    """ref64 / ref32 of config 3: PointNet2_D(3, 50, num_categories=16), B=32, N=2048, seed-0 weights, bench's synthetic
    per-cloud category"""
    import bench
    pos, x, y = bench.make_inputs(C3_B, C3_N, 1234, "cpu")
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in _c3().state_dict().items()}
    cat = (torch.arange(C3_B) % C3_CATS).view(C3_B, 1).expand(C3_B, C3_N).contiguous()
    return _build_references(_c3, sd, pos, x, y, cat)


# ----------------------------------------------------------------------------------------------------- the HIP side

class _Spy(object):
    """records the C-ABI entry points the product path calls (the pattern of test_gpu_fused.py's headline test)"""

    def __enter__(self):
        from torch_points3d_amd import fused
        self.seen, self.fused, self.real = set(), fused, fused._lib.call
        fused._lib.call = lambda name, *a: (self.seen.add(name), self.real(name, *a))[1]
        return self

    def __exit__(self, *exc):
        self.fused._lib.call = self.real
        return False


def _hip_net(make, ref):
    torch.manual_seed(0)
    net = make()
    net.load_state_dict(ref["sd"])
    return _train(net.to(DEV))


def _hip_step(make, ref, x_grad=False, geometry=False):
    """one eager training step of the product path: (stage outputs, gradients, entry points called, running statistics and
    BatchNorm momenta right after the step), and the net"""
    net = _hip_net(make, ref)
    pos, y = ref["pos"].to(DEV), ref["y"].to(DEV)
    cat = None if ref["category"] is None else ref["category"].to(DEV)
    x = ref["x"].to(DEV).clone().requires_grad_(x_grad)
    with _Spy() as spy:
        geom = net.precompute_geometry(pos, backward_tables=True) if geometry else None
        rec = _forward(net, pos, x, cat, geom)
        _loss(rec["out_x"], y).backward()
    grads = dict(((k, q.grad) for k, q in net.named_parameters() if q.grad is not None))
    if x_grad:
        grads["x"] = x.grad
    torch.cuda.synchronize()
    momenta = {k: m.momentum for k, m in net.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    run = {"rec": {k: v.detach() for k, v in rec.items()}, "grads": grads, "seen": spy.seen, "bufs": _buffers(net),
           "momenta": momenta}
    return run, net


def _hip_eval(net, ref):
    """eval pass under no_grad with the running statistics the float64 step left (the same values in every net)"""
    sd = net.state_dict()
    for k, v in ref["after"].items():
        sd[k].copy_(v)
    net.eval()
    cat = None if ref["category"] is None else ref["category"].to(DEV)
    with _Spy() as spy, torch.no_grad():
        rec = _forward(net, ref["pos"].to(DEV), ref["x"].to(DEV), cat)
    torch.cuda.synchronize()
    return rec, spy.seen


def _stat_distances(bufs, want, momenta):
    """per running statistic, max over channels of |value - float64| on the statistic's own scale: running_var on |var|;
    running_mean (= momentum * batch mean after one step from zero) on |mean| + momentum * batch std -- a channel whose
    batch mean is ~0 has no scale of its own.  The batch variance is read back from the float64 running_var (initial 1)."""
    out = {}
    for k, v in bufs.items():
        w = want[k].double()
        if k.endswith("running_mean"):
            m = momenta[k[:-len(".running_mean")]]
            std = ((want[k[:-4] + "var"].double() - (1 - m)) / m).clamp(min=0).sqrt()
            den = w.abs() + m * std
        else:
            den = w.abs()
        out[k] = float(((v.double() - w).abs() / den).max())
    return out


def _check_train(tag, ref, run, stats=True):
    """checks 3-5: per stage rms <= 2x and max <= 4x the fp32 reference's distance to float64; every gradient's relative
    L2 distance to float64 <= 2x the fp32 reference's + GRAD_FLOOR; running statistics within STAT_RTOL of float64"""
    r64, bar, failures = ref["r64"], ref["bar"], []
    rec, grads = run["rec"], run["grads"]
    feats = {}
    for k, (rms_c, max_c) in bar["train"].items():
        want = r64["train"][k]
        rms_g, max_g = _errors(rec[k], want)
        eps = max(1.0, float(want.abs().max()))
        feats[k] = {"rms": [rms_g, rms_c], "max": [max_g, max_c]}
        if rms_g > 2.0 * rms_c + 1e-8 * eps:
            failures.append("%s: rms |HIP-f64| %.3g vs |ref32-f64| %.3g" % (k, rms_g, rms_c))
        if max_g > 4.0 * max_c + 1e-7 * eps:
            failures.append("%s: max |HIP-f64| %.3g vs |ref32-f64| %.3g" % (k, max_g, max_c))
    gr = {}
    for k, g in grads.items():
        want = r64["grad"][k]
        r = float((g.double() - want).norm()) / _grad_ref_norm(k, r64["grad"])
        gr[k] = [r, bar["grad"][k]]
        if r > 2.0 * bar["grad"][k] + GRAD_FLOOR:
            failures.append("grad %s: %.3g vs ref32 %.3g" % (k, r, bar["grad"][k]))
    report(SECTION, tag + "/train_stages_[hip,ref32]", feats)
    report(SECTION, tag + "/grad_rel_l2_[hip,ref32]", gr)
    if stats:
        d_hip = _stat_distances(run["bufs"], r64["after"], run["momenta"])
        d_32 = _stat_distances(ref["r32"]["after"], r64["after"], run["momenta"])
        report(SECTION, tag + "/running_stats_max_rel_[hip,ref32]", [max(d_hip.values()), max(d_32.values())])
        for k, d in d_hip.items():
            if d > STAT_RTOL:
                failures.append("%s: relative distance to float64 %.3g (ref32 %.3g)" % (k, d, d_32[k]))
    worst_feat = max((max(v["rms"][0] / max(v["rms"][1], 1e-30), v["max"][0] / max(v["max"][1], 1e-30) / 2)
                      for v in feats.values()), default=0.0)
    worst_grad = max((r / max(c, 1e-30) for r, c in gr.values()), default=0.0)
    report(SECTION, tag + "/worst_ratio_[features_rms_or_half_max,grad]_vs_ref32", [worst_feat, worst_grad])
    return failures


def _check_eval(tag, ref, rec):
    """check 6: every stage within 1e-5 * scale of the fp32 reference's eval pass, and the fp64 rule"""
    failures, rows = [], {}
    for k, (rms_c, max_c) in ref["bar"]["eval"].items():
        want64, want32 = ref["r64"]["eval"][k], ref["r32"]["eval"][k]
        scale = float(want32.abs().max())
        d32 = float((rec[k].double() - want32.double()).abs().max())
        rms_g, max_g = _errors(rec[k], want64)
        eps = max(1.0, float(want64.abs().max()))
        rows[k] = {"max_vs_ref32_over_scale": d32 / scale, "rms": [rms_g, rms_c], "max": [max_g, max_c]}
        if d32 > 1e-5 * scale:
            failures.append("eval %s: max |HIP-ref32| = %.3g of the scale" % (k, d32 / scale))
        if rms_g > 2.0 * rms_c + 1e-8 * eps or max_g > 4.0 * max_c + 1e-7 * eps:
            failures.append("eval %s: |HIP-f64| rms %.3g max %.3g vs ref32 %.3g %.3g" % (k, rms_g, max_g, rms_c, max_c))
    report(SECTION, tag + "/eval_stages", rows)
    return failures


# ------------------------------------------------------------------------------------------------------- the tests

REQUIRED = {"tp3d_gemm_rows_narrow_f32", "tp3d_gemm_tn_bn_narrow_f32", "tp3d_gemm_rows_bnact_x3_f32",
            "tp3d_gemm_rows_bnact_sp_f32", "tp3d_gemm_rows_bnbwd_sp_f32", "tp3d_gemm_tn_x3_act_red_f32"}

_DEFAULT = {}


def _default_run(ref):
    """the default train step and eval pass (computed once, shared with the switch matrix)"""
    if not _DEFAULT:
        run, net = _hip_step(_unet, ref)
        erec, eseen = _hip_eval(net, ref)
        _DEFAULT.update(run=run, erec=erec, eseen=eseen)
    return _DEFAULT


def test_headline_step_is_as_close_to_float64_as_an_fp32_evaluation(headline):
    """The BASELINE training step (default switches, eagerly) against ref64 / ref32, in this order: geometry, coverage of
    the production entry points, train-mode stages, gradients, running statistics, eval mode, the bench's geometry path."""
    ref = headline
    d = _default_run(ref)
    run = d["run"]
    rec, seen = run["rec"], run["seen"]
    # 1. geometry: sampled positions of every level, and the ball-query / 3-NN tables of precompute_geometry
    for i in range(2):
        assert torch.equal(rec["down%d_pos" % i].cpu(), ref["r32"]["train"]["down%d_pos" % i].cpu()), i
        assert torch.equal(rec["down%d_pos" % i].cpu(), ref["r64"]["train"]["down%d_pos" % i].float().cpu()), i
    with torch.no_grad():
        geom = _hip_net(_unet, ref).precompute_geometry(ref["pos"].to(DEV))
    for i, lvl in enumerate(geom.down):
        assert torch.equal(lvl.idx.long().cpu(), ref["oracle"]["down%d_fps" % i].long()), i
        assert torch.equal(lvl.radius_idx[0].long().cpu(), ref["oracle"]["down%d_ball" % i].long()), i
    for j, up in enumerate(geom.up):
        if j == 0:
            assert up is None
            continue
        assert torch.equal(up.idx.long().cpu(), ref["oracle"]["up%d_nn" % j].long()), j
    # 2. coverage of the production entry points
    report(SECTION, "default/entry_points_train", sorted(seen))
    assert REQUIRED <= seen, sorted(REQUIRED - seen)
    # 3.-5. train-mode stages, gradients, running statistics
    failures = _check_train("default", ref, run)
    # 6. eval mode with the statistics the step left
    report(SECTION, "default/entry_points_eval", sorted(d["eseen"]))
    assert "tp3d_gemm_rows_epi_f32" in d["eseen"]
    failures += _check_eval("default", ref, d["erec"])
    # the input gradient: requested, it changes the first layer's path (no narrow dW kernel), so a run of its own
    run_x, _ = _hip_step(_unet, ref, x_grad=True)
    assert "x" in run_x["grads"]
    failures += _check_train("input_grad", ref, run_x)
    # 7. the bench's geometry path: precomputed tables with their inverted scatter forms (dp.PipelinedStep)
    run_g, _ = _hip_step(_unet, ref, geometry=True)
    for k, v in rec.items():
        assert torch.equal(run_g["rec"][k], v), k
    failures += _check_train("geometry_tables", ref, run_g)
    assert not failures, "\n".join(failures)


# (switch, non-default value, mode): one at a time against the same references
SWITCHES = [("USE_ROWS_GEMM", False, "train"), ("FWD_X3", False, "train"), ("WGRAD_X3_ACT", False, "train"),
            ("WGRAD_X3", 0, "train"), ("WGRAD_X3", 9, "train"), ("ROWS_GEMM_WITHOUT_STATS", False, "train"),
            ("ROWS_GEMM_EPILOGUE", False, "eval"), ("ROWS_GEMM_NARROW", False, "train"), ("USE_MLP_CHAIN", False, "train"),
            ("CHAIN_BWD_LOADER", False, "train"), ("CHAIN_BWD_POOLED", False, "train"),
            ("ROW_ORDER_ALTERNATE", False, "train"), ("WGRAD_NARROW", False, "train"), ("FWD_NARROW", False, "train"),
            ("WGRAD_RED", False, "train"), ("CHAIN_MIN_ROWS", 1 << 30, "train")]
# Switches that change nothing at this shape: the same entry points and a bit-identical step (pinned, so that a change
# in coverage is noticed).  ROWS_GEMM_NARROW: every 64-wide layer of this network sits in a fused chain or is served
# without the rows kernel's 128 x 64 tiles.
INERT = {"ROWS_GEMM_NARROW=False"}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("name,value,mode", SWITCHES, ids=["%s=%s" % (n, v) for n, v, _ in SWITCHES])
def test_switch_matrix_against_float64(headline, name, value, mode):
    """Each fused.py switch at its non-default value, one at a time: the step differs from the default run's (other entry
    points, or -- ROW_ORDER_ALTERNATE, which only changes the row direction argument -- other bits), and obeys the float64
    rules of the default run (train stages, gradients, running statistics, eval mode)."""
    from torch_points3d_amd import fused
    ref = headline
    d = _default_run(ref)
    old = getattr(fused, name)
    tag = "switch/%s=%s" % (name, value)
    try:
        setattr(fused, name, value)
        failures = []
        if mode == "train":
            run, net = _hip_step(_unet, ref)
            failures += _check_train(tag, ref, run)
            seen = run["seen"]
            same = _same(run["rec"], d["run"]["rec"]) and _same(run["grads"], d["run"]["grads"])
            erec, eseen = _hip_eval(net, ref)
        else:
            seen = d["run"]["seen"]
            erec, eseen = _hip_eval(_hip_net(_unet, ref), ref)
            same = True
        same = same and _same(erec, d["erec"])
        failures += _check_eval(tag, ref, erec)
    finally:
        setattr(fused, name, old)
    base = d["run"]["seen"] | d["eseen"]
    changed_calls = (seen != d["run"]["seen"]) or (eseen != d["eseen"])
    report(SECTION, tag + "/entry_points_[added,dropped]", [sorted((seen | eseen) - base), sorted(base - (seen | eseen))])
    report(SECTION, tag + "/bit_identical_to_default", same)
    if "%s=%s" % (name, value) in INERT:
        assert same and not changed_calls, "switch is no longer inert at this shape: take it out of INERT"
    else:
        assert changed_calls or not same, "%s=%s changes nothing at this shape" % (name, value)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("switch", [None, ("USE_MLP_CHAIN", False), ("ROWS_GEMM_WITHOUT_STATS", False)],
                         ids=["default", "USE_MLP_CHAIN=False", "ROWS_GEMM_WITHOUT_STATS=False"])
def test_config3_full_batch_against_float64(config3, switch):
    """Config 3 (PointNet2_D charlesmsg, B=32, N=2048) by the same rules: train stages, class scores (Dropout off on every
    side), gradients, running statistics, eval mode."""
    from torch_points3d_amd import fused
    ref = config3
    old = None if switch is None else getattr(fused, switch[0])
    tag = "config3/" + ("default" if switch is None else "%s=%s" % switch)
    try:
        if switch is not None:
            setattr(fused, switch[0], switch[1])
        run, net = _hip_step(_c3, ref)
        failures = _check_train(tag, ref, run)
        erec, _ = _hip_eval(net, ref)
        failures += _check_eval(tag, ref, erec)
    finally:
        if switch is not None:
            setattr(fused, switch[0], old)
    report(SECTION, tag + "/entry_points_train", sorted(run["seen"]))
    for k in [k for k in run["rec"] if k.endswith("_pos")]:
        assert torch.equal(run["rec"][k].cpu(), ref["r32"]["train"][k].cpu()), k
    assert not failures, "\n".join(failures)
