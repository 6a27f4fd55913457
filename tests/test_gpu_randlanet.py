"""RandLA-Net on the device: the one-kernel eval-mode edge pass (csrc/randla_lfa.hip) against float64 and against the
row kernels it replaces, its routes, its memory, and RandLANetSeg (both configs) against the fixtures the REFERENCE's
own classes produced (tests/golden/make_golden_randlanet.py).

Bars.  Kernel: |fused - fp64| <= max(1e-5 * scale, 2 * |rows - fp64|), fp64 = the module's rows arithmetic in double on
the CPU (randlanet_util.lfa_fp64 + global_nn), rows = the existing path on the same inputs, scale = max |fp64|.
Networks: eval output within 1e-5 * scale of the fixture with lfa="rows" and within randla_golden_util.bound (1e-5, or
twice the reference pass's own distance to float64) with lfa="auto"; train-mode output within that bound of the float64
pass; gradients by relative L2 against the float64 ones at max(1e-4, 4 * the fixture's own float32-to-float64 distance),
the rule of tests/test_gpu_pointnet2_mp.py.  With TP3D_PARITY_OUT set, the kernel distances are written there as JSON
(profiles/randla_lfa_parity.json is such a run)."""
import json
import os

import pytest
import torch

import randlanet_util as ru
from randla_golden_util import bound

pytestmark = pytest.mark.gpu
DEV = "cuda"

NQS = (1, 63, 64, 65, 257)
M = 40
# (Cx or None for x = None, P1, P2, A1)
WIDTHS = {"pos": (None, 8, 3, 8), "c12": (6, 8, 6, 8), "c32": (16, 8, 16, 64), "c64": (32, 16, 32, 128),
          "odd": (5, 7, 6, 7)}
PARITY = []


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("TP3D_PARITY_OUT")
    if path and PARITY:
        with open(path, "w") as f:
            json.dump({"bar": "max(1e-5 * scale, 2 * rows_vs_fp64)", "M": M, "cases": PARITY}, f, indent=1)
            f.write("\n")


def _kernels(widths, seed, global_out=16):
    """three RandlaKernels on the same weights -- lfa "rows", "fused", "auto" -- with BatchNorm buffers and affine
    parameters moved off their defaults so that the folding is exercised; eval mode"""
    from torch_points3d_amd.randla import RandlaKernel
    Cx, P1, P2, A1 = widths
    C = (3 if Cx is None else Cx) + P2
    kw = dict(point_pos_nn=[10, P1, P2], attention_nn=[C, A1, C], global_nn=[C, global_out])
    torch.manual_seed(seed)
    rows = RandlaKernel(lfa="rows", **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in rows.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
    out = {"rows": rows.to(DEV).eval()}
    for lfa in ("fused", "auto"):
        k = RandlaKernel(lfa=lfa, **kw)
        k.load_state_dict(rows.state_dict())
        out[lfa] = k.to(DEV).eval()
    return out


def _inputs(widths, Nq, seed, m=M):
    Cx = widths[0]
    g = torch.Generator().manual_seed(seed)
    pos_s = torch.rand(m, 3, generator=g) * 2 - 1
    pos_q = torch.rand(Nq, 3, generator=g) * 2 - 1
    nbr = torch.randint(0, m, (Nq, 16), generator=g)
    x = None if Cx is None else torch.randn(m, Cx, generator=g)
    return pos_q.to(DEV), pos_s.to(DEV), (None if x is None else x.to(DEV)), nbr.to(DEV)


def _fp64(ker, pos_q, pos_s, x, nbr):
    import copy
    pooled = ru.lfa_fp64(pos_q, pos_s, x, nbr, ker.point_pos_nn, ker.attention_nn)
    with torch.no_grad():
        return copy.deepcopy(ker.global_nn).cpu().double().eval()(pooled)


def _one_kernel(ker, x, pos_q, pos_s, nbr):
    """what RandlaKernel does on the "fused" route, whatever the route function's table of measured wins says of the
    width class: the kernel's arithmetic is tested for every width it accepts"""
    from torch_points3d_amd import fused, randla
    return fused.rows_mlp(ker.global_nn, randla.randla_lfa_eval(pos_q, pos_s, x, nbr, ker.point_pos_nn, ker.attention_nn))


def _route(ker, x, nbr):
    from torch_points3d_amd.randla import lfa_route
    return lfa_route(nbr.shape[1], 3 if x is None else x.shape[1], ker.point_pos_nn, ker.attention_nn, False, False, DEV)


def _check(got, rows, ref64, what):
    scale = float(ref64.abs().max())
    d_fused = float((got.double().cpu() - ref64).abs().max())
    d_rows = float((rows.double().cpu() - ref64).abs().max())
    bar = max(1e-5 * scale, 2.0 * d_rows)
    print("%s: fused vs fp64 %.3e, rows vs fp64 %.3e, scale %.3e, bar %.3e" % (what, d_fused, d_rows, scale, bar))
    assert d_fused <= bar, (what, d_fused, d_rows, bar)
    return d_fused, d_rows, scale


@pytest.mark.parametrize("Nq", NQS)
@pytest.mark.parametrize("tag", sorted(WIDTHS))
def test_kernel_against_float64(hip, tag, Nq):
    widths = WIDTHS[tag]
    kers = _kernels(widths, 100 + len(tag))
    pos_q, pos_s, x, nbr = _inputs(widths, Nq, 7 * Nq + len(tag))
    with torch.no_grad():
        rows = kers["rows"](x, (pos_q, pos_s), nbr)
        auto = kers["auto"](x, (pos_q, pos_s), nbr)
        route = _route(kers["rows"], x, nbr)
        assert route in ("fused", "rows")
        got = _one_kernel(kers["rows"], x, pos_q, pos_s, nbr)
        if route == "rows":  # a width class the route function does not serve: "auto" is the existing path
            assert torch.equal(auto, rows)
            with pytest.raises(ValueError, match="lfa='fused'"):
                kers["fused"](x, (pos_q, pos_s), nbr)
        else:
            assert torch.equal(auto, got) and torch.equal(kers["fused"](x, (pos_q, pos_s), nbr), got)
    assert tuple(got.shape) == tuple(rows.shape) and bool(torch.isfinite(got).all())
    d_fused, d_rows, scale = _check(got, rows, _fp64(kers["rows"], pos_q, pos_s, x, nbr), "%s Nq=%d" % (tag, Nq))
    PARITY.append(dict(widths=tag, route=route, Cx=widths[0], P1=widths[1], P2=widths[2], A1=widths[3], Nq=Nq, fused_vs_fp64=d_fused,
                       rows_vs_fp64=d_rows, scale=scale))


@pytest.mark.parametrize("tag", ["pos", "c32", "c64"])
def test_kernel_edge_cases(hip, tag):
    """a query that is one of its own neighbours (dij = 0), two identical query rows, and a second run"""
    widths = WIDTHS[tag]
    kers = _kernels(widths, 300)
    pos_q, pos_s, x, nbr = _inputs(widths, 70, 11)
    pos_q = pos_s[nbr[:, 3]].clone()  # every query coincides with its neighbour in slot 3
    pos_q[69], nbr[69] = pos_q[5], nbr[5]  # rows 5 and 69: the same query drawn twice
    pos_q[64], nbr[64] = pos_q[63], nbr[63]  # a pair that straddles two workgroups
    with torch.no_grad():
        got = _one_kernel(kers["rows"], x, pos_q, pos_s, nbr)
        again = _one_kernel(kers["rows"], x, pos_q, pos_s, nbr)
        rows = kers["rows"](x, (pos_q, pos_s), nbr)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[5], got[69]) and torch.equal(got[63], got[64])
    assert torch.equal(got, again)
    _check(got, rows, _fp64(kers["rows"], pos_q, pos_s, x, nbr), "edge cases " + tag)


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def test_memory_of_the_two_routes(hip):
    """Nq = 4096, C = 64: the fused forward holds its (Nq, 64) result (1 MiB), the folded constants (< 0.1 MiB) and the
    narrow global_nn rows; the rows route holds fij_hat alone at 65 536 x 64 x 4 B = 16 MiB"""
    widths = WIDTHS["c64"]
    kers = _kernels(widths, 500, global_out=8)
    pos_q, pos_s, x, nbr = _inputs(widths, 4096, 13, m=4096)
    MiB = float(1 << 20)
    with torch.no_grad():
        _one_kernel(kers["rows"], x, pos_q, pos_s, nbr), kers["rows"](x, (pos_q, pos_s), nbr)  # plans, workspaces, caches
        fused = _peak_rise(lambda: _one_kernel(kers["rows"], x, pos_q, pos_s, nbr))
        rows = _peak_rise(lambda: kers["rows"](x, (pos_q, pos_s), nbr))
    print("allocator peak above the inputs: fused %.3f MiB, rows %.3f MiB" % (fused / MiB, rows / MiB))
    assert fused < 2 * MiB, fused / MiB
    assert rows >= 16 * MiB, rows / MiB


def test_routes_refuse_and_fall_back(hip):
    from torch_points3d_amd.randla import RandlaKernel
    widths = WIDTHS["c32"]
    kers = _kernels(widths, 700)
    pos_q, pos_s, x, nbr = _inputs(widths, 65, 17)
    holes = nbr.clone()
    holes[7, 12:] = -1
    with torch.no_grad():
        with pytest.raises(ValueError, match="lfa='fused'"):
            kers["fused"](x, (pos_q, pos_s), holes)
        assert torch.equal(kers["auto"](x, (pos_q, pos_s), holes), kers["rows"](x, (pos_q, pos_s), holes))
    # training mode: the statistics are the batch's; all three modules hold the same buffers before the step
    for k in kers.values():
        k.train()
    with pytest.raises(ValueError, match="lfa='fused'"):
        kers["fused"](x, (pos_q, pos_s), nbr)
    a, r = kers["auto"](x, (pos_q, pos_s), nbr), kers["rows"](x, (pos_q, pos_s), nbr)
    assert torch.equal(a, r) and a.requires_grad
    # eval mode with a gradient wanted: the one-kernel pass has no backward
    for k in kers.values():
        k.eval()
    xg = x.clone().requires_grad_(True)
    assert kers["auto"](xg, (pos_q, pos_s), nbr).requires_grad
    with pytest.raises(ValueError, match="lfa='fused'"):
        kers["fused"](xg, (pos_q, pos_s), nbr)
    # the last convolution of Randlanet_Res does not fit
    kw = dict(point_pos_nn=[10, 32, 64], attention_nn=[128, 256, 128], global_nn=[128, 16])
    torch.manual_seed(3)
    wide = {lfa: RandlaKernel(lfa=lfa, **kw) for lfa in ("rows", "auto", "fused")}
    for k in wide.values():
        k.load_state_dict(wide["rows"].state_dict())
        k.to(DEV).eval()
    x64 = torch.randn(M, 64, device=DEV)
    with torch.no_grad():
        with pytest.raises(ValueError, match="lfa='fused'"):
            wide["fused"](x64, (pos_q, pos_s), nbr)
        assert torch.equal(wide["auto"](x64, (pos_q, pos_s), nbr), wide["rows"](x64, (pos_q, pos_s), nbr))


# ---------------------------------------------------------------- the networks

@pytest.fixture(scope="module", params=ru.CONFIGS)
def case(request):
    return request.param, ru.load_fixture(request.param)


def _count_fused(monkeypatch):
    from torch_points3d_amd import randla
    calls = []
    real = randla.randla_lfa_eval

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(randla, "randla_lfa_eval", counted)
    return calls


def test_network_against_the_reference_fixture(hip, case, monkeypatch):
    """One cloud of 1024 points.  The pooled row of the innermost module is copied to all 16 rows of the last level, so
    the train-mode BatchNorm of the first FPModule removes it: the gradients of `inner.nn` are analytically zero here
    (1e-13 in the fixture's float64 pass) and are checked as such, like a Linear bias under a train-mode BatchNorm."""
    name, gold = case
    draws = ru.draws_of(gold)
    net = ru.build_net(name, gold, DEV, "rows").train()
    ru.replay(net, draws, DEV)
    data = ru.bag(gold, DEV)
    x = data.x.clone().requires_grad_(True)
    data.x = x
    out = net(data)
    f64 = torch.as_tensor(gold["f64/out"])
    tol = bound(gold["out"], gold["f64/out"])
    dist = float((out.detach().double().cpu() - f64).abs().max())
    print("%s train-mode output vs float64: %.3e (bar %.1e)" % (name, dist, tol))
    assert dist <= tol, (dist, tol)
    (out * gold["cot"].to(DEV)).sum().backward()
    checked = 0
    for pname, p in list(net.named_parameters()) + [("x", x)]:
        want = gold["grad64/x"] if p is x else gold.get("pgrad64/" + pname)
        if p is not x and p.grad is None:  # features_downsample_nn of a residual block: evaluated, not consumed
            assert want is None, pname
            continue
        assert want is not None, pname
        if p is not x and pname.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
            wn = float(gold["pgrad64/" + pname[:-4] + "weight"].norm())
            assert float(p.grad.norm()) < 1e-4 * wn + 1e-6, pname
            continue
        if p is not x and ".inner.nn." in pname:
            # analytically zero (see the docstring): the bias rule above, against the gradient of the FPModule weight
            # whose BatchNorm does the cancelling
            wn = float(gold["pgrad64/" + pname[:pname.index("inner.nn.")] + "up.nn.0.0.weight"].norm())
            assert float(p.grad.norm()) < 1e-4 * wn + 1e-6 and float(want.norm()) < 1e-4 * wn + 1e-6, pname
            continue
        tolg = max(1e-4, 4.0 * float(gold["grel/" + pname][0]))
        rel = float((p.grad.cpu() - want).norm() / (want.norm() + 1e-30))
        print("gradient %s: relative L2 %.3e (bar %.1e)" % (pname, rel, tolg))
        assert rel <= tolg, (pname, rel, tolg)
        checked += 1
    assert checked > 60
    sd = net.state_dict()
    after = {k[len("after/"):]: v for k, v in gold.items() if k.startswith("after/")}
    assert len(after) > 60
    for k, v in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v), k
        else:
            torch.testing.assert_close(sd[k].cpu(), v, rtol=1e-4, atol=1e-5, msg=k)
    # eval mode on the statistics this step left: rows, then the routed network on the same state
    want = gold["eval/out"]
    scale = float(want.abs().max())
    net.eval()
    with torch.no_grad():
        ev = net(ru.bag(gold, DEV))
    d_rows = float((ev.cpu() - want).abs().max())
    auto = ru.build_net(name, gold, DEV, "auto")
    auto.load_state_dict(net.state_dict(), strict=True)
    auto.eval()
    ru.replay(auto, draws, DEV)
    calls = _count_fused(monkeypatch)
    with torch.no_grad():
        ev_auto = auto(ru.bag(gold, DEV))
    d_auto = float((ev_auto.cpu() - want).abs().max())
    print("%s eval output vs the fixture: rows %.3e (bar %.1e), auto %.3e (bar %.1e), %d fused edge passes" % (
        name, d_rows, 1e-5 * scale, d_auto, tol, len(calls)))
    assert d_rows <= 1e-5 * scale, (d_rows, scale)
    assert d_auto <= tol, (d_auto, tol)
    from torch_points3d_amd.randla import lfa_route
    convs = ru.samplers(auto)
    served = sum(lfa_route(16, c._conv.attention_nn[0][0].in_features - c._conv.point_pos_nn[1][0].out_features,
                           c._conv.point_pos_nn, c._conv.attention_nn, False, False, DEV) == "fused" for c in convs)
    assert len(calls) == served and len(convs) == (3 if name == "Randlanet_Conv" else 4)
    assert served <= 3  # the [128, 256, 128] attention MLP of Randlanet_Res never fits


def test_two_clouds_in_one_batch(hip, monkeypatch):
    """Clouds of 300 and 724 points, Randlanet_Conv, eval mode, the samplers' own sort: each cloud's rows equal the same
    network run on that cloud alone with that cloud's share of the draws; every level's batch vector is sorted."""
    from torch_points3d_amd.kpconv_blocks import PDData
    gold = ru.load_fixture("Randlanet_Conv")
    sizes, quota = (300, 724), ((80, 24, 6), (176, 40, 10))
    g = torch.Generator().manual_seed(91)
    pos = torch.rand(1024, 3, generator=g) * 2 - 1
    x = torch.randn(1024, ru.FEAT, generator=g)
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes))
    # per level and cloud an unsorted draw with replacement among the cloud's rows of the level below
    below, share = list(sizes), [[], []]
    joint = []
    for level in range(3):
        parts, base = [], 0
        for c in range(2):
            d = torch.randint(0, below[c], (quota[c][level],), generator=g)
            share[c].append(d)
            parts.append(d + base)
            base += below[c]
            below[c] = quota[c][level]
        both = torch.cat(parts)
        joint.append(both[torch.randperm(both.numel(), generator=g)])
    state = dict(ru.state_of(gold), **{k[len("after/"):]: v for k, v in gold.items() if k.startswith("after/")})

    def run(pos_, x_, batch_, draws):
        net = ru.build_net("Randlanet_Conv", gold, DEV, "auto")
        net.load_state_dict(state, strict=True)
        net.eval()
        pending = [d.to(DEV) for d in draws]
        monkeypatch.setattr(torch, "randint", lambda *a, **kw: pending.pop(0))  # RandomSampler(sort=True) sorts it
        levels = []
        hooks = [c.register_forward_hook(lambda m, i, o: levels.append(o.batch)) for c in ru.samplers(net)]
        try:
            with torch.no_grad():
                out = net(PDData(pos=pos_.to(DEV), x=x_.to(DEV), batch=batch_.to(DEV)))
        finally:
            monkeypatch.undo()
            for h in hooks:
                h.remove()
        assert not pending and len(levels) == 3
        return out.cpu(), [b.cpu() for b in levels]

    out, levels = run(pos, x, batch, joint)
    for level, b in enumerate(levels):
        assert bool((b[1:] >= b[:-1]).all()), level
        assert [int((b == c).sum()) for c in range(2)] == [quota[0][level], quota[1][level]]
    scale = float(out.abs().max())
    lo = 0
    for c, n in enumerate(sizes):
        alone, _ = run(pos[lo:lo + n], x[lo:lo + n], torch.zeros(n, dtype=torch.long), share[c])
        d = float((out[lo:lo + n] - alone).abs().max())
        print("cloud %d: batch vs alone %.3e (bar %.1e)" % (c, d, 1e-5 * scale))
        assert d <= 1e-5 * scale, (c, d)
        lo += n
