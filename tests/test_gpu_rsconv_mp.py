"""Message-passing RSConv on the HIP kernels (csrc/rsconv_mp.hip, torch_points3d_amd/rsconv_mp.py) against the plain-torch
restatement tests/rsconv_mp_ref.py and the fixture the REFERENCE's own Convolution / RSConvDown produced
(tests/golden/rsconv_mp.npz, written by tests/golden/make_golden_rsconv_mp.py; see its docstring for what stands in for
torch_geometric and for the two places where the reference cannot be followed literally).

Bars.  Kernel level: everything torch.equal -- indices, the relation rows' columns 1-9 (one subtraction or a copy), and
the fused max and its d_w (one multiplication: the composition segment_max(w * x[col]) has to be met to the bit) --
except the relation rows' column 0, rtol 1e-6 / atol 0 against the float64 norm of the same float32 differences (three
squares, two adds and a square root are a few roundings in whatever order, 1e-6 ~ 8 ulp), and dx where a support row
wins in hundreds of queries (a sum in another order than float64's: rtol 1e-5, atol 1e-5 * |ref|max).  Module and network
level: exactly the bars at the head of tests/test_gpu_pointnet2_mp.py -- stages teacher-forced rtol 1e-5 /
atol bound(out, out64); the chained network <= 4x max and <= 2x RMS of the reference pass's own distance to float64;
BatchNorm buffers 1e-4 / 1e-5; eval mode 1e-5 * max(1, scale); gradients in relative L2 <= max(1e-4, 4 * grel) with grel
stored in the fixture.  None of these figures comes from the code under test."""
import pytest
import torch

from conftest import load_golden
import pointnet2_mp_ref as mp
import rsconv_mp_ref as ref
from randla_golden_util import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STAGES = ("rs1", "rs2", "glob", "fp0", "fp1", "fp2", "out")


@pytest.fixture(scope="module")
def gold():
    return load_golden("rsconv_mp")


def _sub(gold, prefix):
    return {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _csr(lengths):
    es = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    es[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return es


# any CSR, not the finder's cap.  3: runs cut into 5 pieces of 140 / 1 / 26 rows (four of the middle run's five are empty)
RUNS = {1: [200], 3: [700, 1, 130], 5: [1, 0, 64, 65, 3], 257: ([0, 1, 63, 64, 65, 200, 2, 7] * 33)[:257]}


def _parts(E, nq):
    """pieces per run of the element-walking kernels (csrc/edge_run.h run_parts): about 64 rows each, from the MEAN run"""
    return max(1, min(1024, (E // nq + 63) // 64))


def _case(C, nq, ldw, seed):
    """w and x in eighths: the products are exact and tie often (the first edge has to win); support rows repeat inside
    a run; the padding columns of w hold garbage; the last query with two edges or more sees negative products only"""
    g = torch.Generator().manual_seed(seed)
    es = _csr(RUNS[nq])
    E, M = int(es[-1]), 23
    col = torch.randint(0, M - 2, (E,), generator=g)
    w = torch.randint(-8, 9, (E, ldw), generator=g).float() / 8
    w[:, C:] = 1e30
    x = torch.randint(-8, 9, (M, C), generator=g).float() / 8
    x[M - 2:] = -x[M - 2:].abs() - 0.125
    deg = es[1:] - es[:-1]
    neg = int(torch.nonzero(deg >= 2)[-1]) if bool((deg >= 2).any()) else None
    if neg is not None:
        a, b = int(es[neg]), int(es[neg + 1])
        col[a:b] = torch.randint(M - 2, M, (b - a,), generator=g)
        w[a:b, :C] = w[a:b, :C].abs() + 0.125
    return es, col, w, x, neg


# ---------------------------------------------------------------------------------------------------- relation rows
@pytest.mark.parametrize("ld", [10, 12, 17])
def test_relation_rows(hip, ld):
    _relation_rows_case(hip, ld, 257, 50, 40)
    assert _parts(sum(RUNS[3]), 3) == 5
    _relation_rows_case(hip, ld, 3, 3, 3)


def _relation_rows_case(hip, ld, nq, head, least_zero):
    g = torch.Generator().manual_seed(ld)
    es = _csr(RUNS[nq])
    E, M = int(es[-1]), 300
    pos_s = torch.rand(M, 3, generator=g) * 2 - 1
    col = torch.randint(0, M, (E,), generator=g)
    pos_q = torch.rand(nq, 3, generator=g) * 2 - 1
    pos_q[:head] = pos_s[col[es[:head].clamp(max=E - 1)]]  # the first edge of these queries: a query that IS its support point
    got = hip.rsconv_relation_rows(pos_s.to(DEV), pos_q.to(DEV), es.to(DEV), col.to(DEV), ld=ld).cpu()
    want = ref.relation_rows(pos_s, pos_q, es, col, ld=ld)
    assert got.shape == want.shape == (E, ld)
    assert torch.equal(got[:, 1:10], want[:, 1:10])
    assert not bool(got[:, 10:].any())
    norm64 = want[:, 1:4].double().norm(dim=1)
    torch.testing.assert_close(got[:, 0].double(), norm64, rtol=1e-6, atol=0.0)
    zero = torch.nonzero(norm64 == 0).reshape(-1)
    assert zero.numel() >= least_zero and bool((got[zero, 0] == 0).all())
    if ld == 12:
        assert torch.equal(hip.rsconv_relation_rows(pos_s.to(DEV), pos_q.to(DEV), es.to(DEV), col.to(DEV)).cpu(), got)
        none = hip.rsconv_relation_rows(pos_s.to(DEV), pos_q.to(DEV), torch.zeros(nq + 1, dtype=torch.long, device=DEV),
                                        torch.zeros(0, dtype=torch.long, device=DEV))
        assert tuple(none.shape) == (0, 12)
    with pytest.raises(ValueError):
        hip.rsconv_relation_rows(pos_s.to(DEV), pos_q.to(DEV), es.to(DEV), col.to(DEV), ld=9)


# ---------------------------------------------------------------------------------------------------- msgmax
@pytest.mark.parametrize("nq", [1, 3, 5, 257])
@pytest.mark.parametrize("C", [3, 16, 64, 130])
def test_msgmax_forward_and_d_w_equal_the_composition(hip, C, nq):
    assert nq != 3 or _parts(sum(RUNS[3]), 3) == 5
    for ldw in (C, C + 5):
        es, col, w, x, neg = _case(C, nq, ldw, 1000 * C + nq)
        wd, wr = w.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        xd, xr = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        out, arg = hip.rsconv_msgmax(wd, xd, es.to(DEV), col.to(DEV), C=C, return_argmax=True)
        want, warg = ref.msgmax(wr, xr, es, col.to(DEV), C=C)
        assert arg.dtype == torch.int64 and torch.equal(arg, warg), (ldw, "argmax")
        assert torch.equal(out, want), (ldw, "out")
        deg = es[1:] - es[:-1]
        empty = deg == 0
        assert not bool(out[empty.to(DEV)].any()) and bool((arg[empty.to(DEV)] == -1).all())
        if neg is not None:
            assert bool((out[neg] < 0).all())  # the negative maximum, not 0
        if int(deg.max()) >= 63:  # ties happened, and the first edge won them (the restatement's rule)
            prod = (w[:, :C] * x[col]).to(DEV)
            ties = 0
            for i in torch.nonzero(deg >= 63).reshape(-1).tolist()[:4]:
                blk = prod[int(es[i]):int(es[i + 1])]
                ties += int(((blk == out[i]).sum(0) > 1).sum())
            assert ties > 0
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(C + nq)).to(DEV)
        (out * cot).sum().backward()
        (want * cot).sum().backward()
        assert torch.equal(wd.grad, wr.grad), (ldw, "d_w")
        assert not bool(wd.grad[:, C:].any())
        torch.testing.assert_close(xd.grad, xr.grad, rtol=1e-5, atol=1e-5 * float(xr.grad.abs().max()))


def test_msgmax_feature_rows_wider_than_c_and_argument_checks(hip):
    es, col, w, x, _ = _case(16, 5, 20, 5)
    xw = torch.cat([x, torch.full((x.shape[0], 3), 1e30)], 1).to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    out, arg = hip.rsconv_msgmax(wd, xw, es.to(DEV), col.to(DEV), C=16, return_argmax=True)
    want, warg = ref.msgmax(w.to(DEV), x.to(DEV), es, col.to(DEV))
    assert torch.equal(out, want) and torch.equal(arg, warg)
    out.sum().backward()
    assert tuple(xw.grad.shape) == (x.shape[0], 19) and not bool(xw.grad[:, 16:].any())
    with pytest.raises(ValueError):
        hip.rsconv_msgmax(wd, xw, es.to(DEV), col.to(DEV), C=21)
    with pytest.raises(ValueError):
        hip.rsconv_msgmax(wd, xw, es.to(DEV), col[:-1].to(DEV), C=16)


def test_msgmax_without_edges(hip):
    w = torch.zeros(0, 8, device=DEV, requires_grad=True)
    x = torch.rand(5, 8, device=DEV, requires_grad=True)
    es = torch.zeros(4, dtype=torch.long, device=DEV)
    out, arg = hip.rsconv_msgmax(w, x, es, torch.zeros(0, dtype=torch.long, device=DEV), return_argmax=True)
    assert tuple(out.shape) == (3, 8) and not bool(out.any()) and bool((arg == -1).all())
    out.sum().backward()
    assert tuple(w.grad.shape) == (0, 8) and not bool(x.grad.any())
    out = hip.rsconv_msgmax(w, x, torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV))
    assert tuple(out.shape) == (0, 8)


def test_msgmax_dx_exact_with_one_winner_per_support(hip):
    """every support row belongs to one edge: at most one term per (support, channel), so dx is a single product"""
    g = torch.Generator().manual_seed(77)
    es = _csr(RUNS[257])
    E, C = int(es[-1]), 37
    col = torch.randperm(E + 9, generator=g)[:E]
    w, x = torch.randn(E, C + 3, generator=g), torch.randn(E + 9, C, generator=g)
    wd, wr = w.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    xd, xr = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    out = hip.rsconv_msgmax(wd, xd, es.to(DEV), col.to(DEV), C=C)
    want, _ = ref.msgmax(wr, xr, es, col.to(DEV), C=C)
    cot = torch.randn(out.shape, generator=g).to(DEV)
    (out * cot).sum().backward()
    (want * cot).sum().backward()
    assert torch.equal(out, want) and torch.equal(wd.grad, wr.grad) and torch.equal(xd.grad, xr.grad)


def test_msgmax_dx_at_a_hub_support_row(hip):
    """support row 0 is an edge of all 300 queries and wins every channel of each: 300 terms per element of dx[0]"""
    g = torch.Generator().manual_seed(78)
    nq, C, M = 300, 16, 40
    es = _csr([3] * nq)
    col = torch.randint(1, M, (3 * nq,), generator=g)
    col[1::3] = 0
    w, x = torch.rand(3 * nq, C, generator=g), torch.rand(M, C, generator=g)
    w[1::3] += 1.0
    x[0] += 5.0
    cot = torch.randn(nq, C, generator=g)
    grads = []
    for _ in range(2):
        wd, xd = w.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        out, arg = hip.rsconv_msgmax(wd, xd, es.to(DEV), col.to(DEV), return_argmax=True)
        (out * cot.to(DEV)).sum().backward()
        grads.append(xd.grad.cpu())
    assert bool((col.to(DEV)[arg] == 0).all())
    assert torch.equal(grads[0], grads[1])  # no floating-point atomics: the same bits every run
    w64, x64 = w.double().requires_grad_(True), x.double().requires_grad_(True)
    (ref.msgmax(w64, x64, es, col)[0] * cot.double()).sum().backward()
    torch.testing.assert_close(grads[0].double(), x64.grad, rtol=1e-5, atol=1e-5 * float(x64.grad.abs().max()))
    torch.testing.assert_close(wd.grad.double().cpu(), w64.grad, rtol=1e-6, atol=0.0)


def test_msgmax_skips_dx_when_the_features_want_no_gradient(hip, monkeypatch):
    from torch_points3d_amd import _lib
    es, col, w, x, _ = _case(16, 5, 16, 9)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    wd, xd = w.to(DEV).requires_grad_(True), x.to(DEV)
    hip.rsconv_msgmax(wd, xd, es.to(DEV), col.to(DEV)).sum().backward()
    assert xd.grad is None and wd.grad is not None
    assert calls == ["tp3d_rsconv_msgmax_fwd_f32", "tp3d_rsconv_msgmax_bwd_f32"]


# ---------------------------------------------------------------------------------------------------- the fixture
def _bag(gold, tag, x=None):
    from torch_points3d_amd.kpconv_blocks import PDData
    if tag == "in":
        pos, batch, xx = gold["pos"], gold["batch"], None
    elif tag == "glob":
        pos, batch, xx = torch.zeros(len(ref.GOLD_SIZES), 3), torch.arange(len(ref.GOLD_SIZES)), gold["glob/x"]
    else:
        pos, batch, xx = gold[tag + "/pos"], gold[tag + "/batch"], gold[tag + "/x"]
    xx = xx if x is None else x
    return PDData(pos=pos.to(DEV), batch=batch.to(DEV), x=None if xx is None else xx.to(DEV))


def _net(gold, fused=True):
    from torch_points3d_amd.rsconv_mp import RSConvMP
    net = RSConvMP(ref.GOLD_CFG, ref.GOLD_CLASSES, fused=fused)
    net.load_state_dict(_sub(gold, "sd/"), strict=True)  # the reference's keys
    return net.to(DEV).train()


def _dist64(t, ref64):
    d = t.detach().double().cpu() - torch.as_tensor(ref64)
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def _close(got, gold, key):
    want = gold[key + "/x"]
    torch.testing.assert_close(got.detach().cpu(), want, rtol=1e-5, atol=bound(want, gold["f64/" + key + "/x"]),
                               msg=lambda m: "stage %s: %s" % (key, m))


def _check_grads(named, gold, prefix):
    checked = 0
    for name, p in named:
        want = gold.get(prefix + "pgrad/" + name)
        assert want is not None, name
        if name.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
            wn = float(gold[prefix + "pgrad/" + name[:-4] + "weight"].norm())
            assert p.grad is None or float(p.grad.norm()) < 1e-4 * wn + 1e-6, name
            continue
        tol = max(1e-4, 4.0 * float(gold[prefix + "grel/" + name][0]))
        rel = float((p.grad.cpu() - want).norm() / (want.norm() + 1e-30))
        print("gradient %s%s: relative L2 %.3e (bar %.1e)" % (prefix, name, rel, tol))
        assert rel <= tol, (name, rel, tol)
        checked += 1
    return checked


def _check_buffers(module, gold, prefix, least):
    sd = module.state_dict()
    after = _sub(gold, prefix)
    assert len(after) >= least
    for name, v in after.items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v), name
        else:
            torch.testing.assert_close(sd[name].cpu(), v, rtol=1e-4, atol=1e-5, msg=name)


@pytest.mark.parametrize("fused", [True, False])
def test_stages_teacher_forced_on_the_fixture(hip, gold, fused):
    from torch_points3d_amd import fused as fz
    net = _net(gold, fused)
    b0 = net.model
    b1 = b0.submodule
    b2 = b1.submodule
    levels = ((b0.down, "in", "rs1"), (b1.down, "rs1", "rs2"))
    for down, src, dst in levels:
        data = _bag(gold, src)
        idx = gold[dst + "/idx"].to(DEV)
        edges = down.neighbour_finder(data.pos, data.pos[idx], batch_x=data.batch, batch_y=data.batch[idx])
        want_es, want_col = gold["edges/%s/edge_start" % dst], gold["edges/%s/col" % dst]
        assert torch.equal(edges.edge_start.cpu(), want_es) and torch.equal(edges[1].cpu(), want_col)
        # the winning edges, on a copy of the layer (a second train-mode pass would move the BatchNorm buffers)
        conv = down._conv
        with torch.no_grad():
            rows = hip.rsconv_relation_rows(data.pos, data.pos[idx], edges.edge_start, edges[1])
            sd = {k: v.clone() for k, v in conv.state_dict().items()}
            wts = fz.rows_mlp(conv.local_nn, rows)
            conv.load_state_dict(sd)
            feats = data.pos if data.x is None else data.x
            _, arg = hip.rsconv_msgmax(wts, feats, edges.edge_start, edges[1], return_argmax=True)
        assert torch.equal(arg.cpu(), gold[dst + "/arg"]), dst
        out = down(data)
        assert torch.equal(out.idx.cpu(), gold[dst + "/idx"]) and torch.equal(out.pos.cpu(), gold[dst + "/pos"])
        assert torch.equal(out.batch.cpu(), gold[dst + "/batch"])
        _close(out.x, gold, dst)
    dg = b2.inner(_bag(gold, "rs2"))
    _close(dg.x, gold, "glob")
    _close(b2.up((_bag(gold, "glob"), _bag(gold, "rs2"))).x, gold, "fp0")
    _close(b1.up((_bag(gold, "rs2", gold["fp0/x"]), _bag(gold, "rs1"))).x, gold, "fp1")
    _close(b0.up((_bag(gold, "rs1", gold["fp1/x"]), _bag(gold, "in"))).x, gold, "fp2")


@pytest.mark.parametrize("fused", [True, False])
def test_chained_network_gradients_buffers_and_eval(hip, gold, fused):
    net = _net(gold, fused)
    out = net(_bag(gold, "in"))
    own_max, own_rms = _dist64(gold["out/x"], gold["f64/out/x"])
    got_max, got_rms = _dist64(out, gold["f64/out/x"])
    print("chained output vs float64: max %.3e (reference pass %.3e), rms %.3e (reference pass %.3e)" % (
        got_max, own_max, got_rms, own_rms))
    assert got_max <= 4 * own_max and got_rms <= 2 * own_rms, (got_max, own_max, got_rms, own_rms)
    (out * gold["cot"].to(DEV)).sum().backward()
    assert _check_grads(list(net.named_parameters()), gold, "") > 40
    _check_buffers(net, gold, "after/", 30)
    net.eval()
    with torch.no_grad():
        ev = net(_bag(gold, "in"))
    want = gold["eval/out/x"]
    torch.testing.assert_close(ev.cpu(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))


@pytest.mark.parametrize("fused", [True, False])
def test_stand_alone_convolution_with_features(hip, gold, fused):
    from torch_points3d_amd.rsconv_mp import Convolution
    conv = Convolution(local_nn=ref.GOLD_CONV["local_nn"], global_nn=ref.GOLD_CONV["global_nn"], fused=fused)
    conv.load_state_dict(_sub(gold, "conv/sd/"), strict=True)
    conv = conv.to(DEV).train()
    pos = gold["pos"].to(DEV)
    pos_q = pos[gold["conv/idx"].to(DEV)]
    row = torch.repeat_interleave(torch.arange(pos_q.shape[0]), gold["conv/edge_start"][1:] - gold["conv/edge_start"][:-1])
    edges = (row.to(DEV), gold["conv/col"].to(DEV))  # a plain (row, col) pair: the offsets are counted
    x = gold["conv/x_in"].to(DEV).requires_grad_(True)
    out = conv(x, (pos, pos_q), edges)
    want = gold["conv/x"]
    torch.testing.assert_close(out.detach().cpu(), want, rtol=1e-5, atol=bound(want, gold["conv/f64/x"]))
    (out * gold["conv/cot"].to(DEV)).sum().backward()
    want = gold["conv/grad_x"]
    rel = float((x.grad.cpu() - want).norm() / want.norm())
    assert rel <= max(1e-4, 4.0 * float(gold["conv/grel/x"][0])), rel
    assert _check_grads(list(conv.named_parameters()), gold, "conv/") >= 6
    _check_buffers(conv, gold, "conv/after/", 9)
    conv.eval()
    with torch.no_grad():
        ev = conv(x.detach(), (pos, pos_q), edges)
    want = gold["conv/eval/x"]
    torch.testing.assert_close(ev.cpu(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))
    # without features x_j = pos_j: positions get no gradient
    conv3 = Convolution(local_nn=[10, 8, 3], fused=fused).to(DEV).train()
    ps = pos.clone().requires_grad_(True)
    conv3(None, (ps, pos_q), edges).sum().backward()
    assert ps.grad is None and conv3.local_nn[0][0].weight.grad is not None


# ---------------------------------------------------------------------------------------------------- past the first tile
def test_rsconv_down_on_a_ragged_batch_past_the_first_tile(hip, oracle):
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.rsconv_mp import RSConvDown
    sizes = [65, 1, 4099, 2, 0, 63]
    g = torch.Generator().manual_seed(31)
    pos = torch.rand(sum(sizes), 3, generator=g) * 2 - 1
    batch = _batch_of(sizes)
    x = torch.randn(pos.shape[0], 5, generator=g)
    torch.manual_seed(3)
    down = RSConvDown(ratio=0.25, radius=0.3, local_nn=[10, 8, 5], down_conv_nn=[5, 16]).to(DEV).train()
    plan = mp.search_plan(oracle, pos, batch, [0.25], [0.3], [64], [])
    idx, (es, col) = plan["idx"][0], plan["edges"][0][0]
    deg = es[1:] - es[:-1]
    assert int(deg.min()) >= 1 and int(deg.max()) == 64 and int((deg < 64).sum()) > 10
    edges = down.neighbour_finder(pos.to(DEV), pos.to(DEV)[idx.to(DEV)], batch_x=batch.to(DEV), batch_y=batch.to(DEV)[idx.to(DEV)])
    assert torch.equal(edges.edge_start.cpu(), es) and torch.equal(edges[1].cpu(), col)
    sd = {k: v.detach().cpu().clone() for k, v in down.state_dict().items()}
    xd = x.to(DEV).requires_grad_(True)
    out = down(PDData(pos=pos.to(DEV), batch=batch.to(DEV), x=xd))
    assert torch.equal(out.idx.cpu(), idx) and torch.equal(out.batch.cpu(), batch[idx])
    cot = torch.randn(out.x.shape, generator=g)
    (out.x * cot.to(DEV)).sum().backward()
    res = {}
    for dtype in (torch.float32, torch.float64):
        m = ref.RSConvDown.from_state_dict(sd, dtype)
        xi = x.to(dtype).clone().requires_grad_(True)
        o = m(xi, pos.to(dtype), idx, (es, col))
        (o * cot.to(dtype)).sum().backward()
        res[dtype] = (o.detach(), xi.grad, m._conv.margin)
    o32, g32, _ = res[torch.float32]
    o64, g64, margin = res[torch.float64]
    print("closest max-pool contest of the float64 pass: %.3e" % margin)
    torch.testing.assert_close(out.x.detach().cpu(), o32, rtol=1e-5, atol=bound(o32, o64))
    grel = float((g32.double() - g64).norm() / g64.norm())
    rel = float((xd.grad.cpu().double() - g64).norm() / g64.norm())
    print("gradient x: relative L2 to float64 %.3e (the restatement's float32 pass: %.3e)" % (rel, grel))
    assert rel <= max(1e-4, 4.0 * grel), (rel, grel)
