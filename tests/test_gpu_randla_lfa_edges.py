"""The one-kernel eval-mode edge pass (csrc/randla_lfa.hip, tp3d_randla_lfa_eval_f32) where tests/test_gpu_randlanet.py
does not reach: the seams of its 16-column blocks, more than one pass of the grid over the queries (a wave's second
query lands on tiles the first one left dirty), a softmax that a naive exp cannot evaluate, degenerate geometry and
input forms, and the folded constants following the module's state through training passes and replayed steps.

The bar is that file's, unchanged: |fused - fp64| <= max(1e-5 * scale, 2 * |rows - fp64|), fp64 = the module's rows
arithmetic in double on the CPU (randlanet_util.lfa_fp64 + global_nn), rows = RandlaKernel(lfa="rows") on the same
inputs, scale = max |fp64|.  The kernel is always run through _one_kernel (randla.randla_lfa_eval called directly), so no
case can fall to the rows route unnoticed.  Every measured pair of distances goes to golden_util.report and, with
TP3D_PARITY_OUT set, to that file as JSON (profiles/randla_lfa_edges_parity.json is such a run)."""
import json
import os

import pytest
import torch

from golden_util import report
from test_gpu_randlanet import WIDTHS, _check, _fp64, _inputs, _kernels, _one_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 40
BIG = (1, 64, 63, 128)  # the largest LDS carve the kernel accepts: 144 624 bytes, one workgroup per CU
PARITY = []


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("TP3D_PARITY_OUT")
    if path and PARITY:
        with open(path, "w") as f:
            json.dump({"bar": "max(1e-5 * scale, 2 * rows_vs_fp64)", "cases": PARITY}, f, indent=1)
            f.write("\n")


def _tag(widths):
    return "x".join("none" if w is None else str(w) for w in widths)


def _held(section, what, widths, got, rows, ref64, **more):
    """the file's bar, with the measured distances on record"""
    d_fused, d_rows, scale = _check(got, rows, ref64, "%s %s" % (section, what))
    PARITY.append(dict(section=section, case=what, Cx=widths[0], P1=widths[1], P2=widths[2], A1=widths[3],
                       fused_vs_fp64=d_fused, rows_vs_fp64=d_rows, scale=scale, **more))
    report("randla_lfa_edges", "%s %s" % (section, what), dict(fused_vs_fp64=d_fused, rows_vs_fp64=d_rows, scale=scale))
    return max(1e-5 * scale, 2.0 * d_rows)


def _three(ker, x, pos_q, pos_s, nbr):
    """the kernel's output, the rows route's, the float64 evaluation"""
    with torch.no_grad():
        got = _one_kernel(ker, x, pos_q, pos_s, nbr)
        rows = ker(x, (pos_q, pos_s), nbr)
    assert ker.lfa == "rows"
    assert tuple(got.shape) == tuple(rows.shape) == (nbr.shape[0], 16)
    assert bool(torch.isfinite(got).all())
    return got, rows, _fp64(ker, pos_q, pos_s, x, nbr)


# ---------------------------------------------------------------- A. block seams

SEAMS = [(10, 16, 6, 16),     # every dimension exactly one block
         (11, 17, 6, 17),     # one column into the second block everywhere
         (1, 33, 32, 65),     # Cx = 1 (the gather's i / Cx, col0 of layer 2 = 1), C = 33
         (45, 1, 3, 48),      # P1 = 1, C = 48
         (60, 64, 3, 127),    # C = 63
         (63, 5, 1, 128),     # P2 = 1, C = 64
         BIG,
         (None, 64, 61, 128)]  # x is None, C = 64


@pytest.mark.parametrize("Nq", [3, 130])
@pytest.mark.parametrize("widths", SEAMS, ids=_tag)
def test_block_seams(hip, widths, Nq):
    ker = _kernels(widths, 900 + sum(w or 0 for w in widths))["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, Nq, 31 * Nq + widths[1])
    got, rows, ref64 = _three(ker, x, pos_q, pos_s, nbr)
    _held("seams", "%s Nq=%d" % (_tag(widths), Nq), widths, got, rows, ref64, Nq=Nq)
    with torch.no_grad():
        assert torch.equal(_one_kernel(ker, x, pos_q, pos_s, nbr), got)


# ---------------------------------------------------------------- B. more than one pass of the grid

@pytest.mark.parametrize("widths", [WIDTHS["pos"], WIDTHS["odd"], WIDTHS["c64"], BIG], ids=_tag)
def test_more_than_one_grid_pass(hip, widths):
    """The launch holds at most 4 workgroups of 4 waves per CU, so with 2 * 16 * CUs + 5 queries every wave serves at
    least two, the last pass is ragged and Nq % 4 = 1.  A query's arithmetic touches its own rows and the weights only:
    its output row must not depend, by a single bit, on which query used the wave's tiles before it."""
    from torch_points3d_amd import randla
    Nq = 2 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    ker = _kernels(widths, 1100 + widths[3])["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, Nq, 41 + widths[1], m=500)
    got, rows, ref64 = _three(ker, x, pos_q, pos_s, nbr)
    _held("passes", "%s Nq=%d" % (_tag(widths), Nq), widths, got, rows, ref64, Nq=Nq)
    g = torch.Generator().manual_seed(Nq)
    with torch.no_grad():
        pooled = randla.randla_lfa_eval(pos_q, pos_s, x, nbr, ker.point_pos_nn, ker.attention_nn)
        for name, perm in (("permuted", torch.randperm(Nq, generator=g)), ("reversed", torch.arange(Nq - 1, -1, -1))):
            perm = perm.to(DEV)
            pq, nb = pos_q[perm].contiguous(), nbr[perm].contiguous()
            again = randla.randla_lfa_eval(pq, pos_s, x, nb, ker.point_pos_nn, ker.attention_nn)
            assert torch.equal(again, pooled[perm]), name  # the edge pass alone
            assert torch.equal(_one_kernel(ker, x, pq, pos_s, nb), got[perm]), name


# ---------------------------------------------------------------- C. saturated softmax

def _spread(C):
    """one channel of each 16-block of the C attention scores, at a different place in each block (the last block may
    be a partial one)"""
    return [16 * b + min(off, C - 1 - 16 * b) for b, off in enumerate((3, 9, 0, 15)) if 16 * b < C]


@pytest.mark.parametrize("mode", ["first", "last", "each_block", "minus"])
@pytest.mark.parametrize("widths", [WIDTHS["c32"], (11, 17, 6, 17), BIG], ids=_tag)
def test_saturated_softmax(hip, widths, mode):
    """300 added to the BatchNorm bias of attention scores: the softmax is one-hot to within e^-300 (the float64 side
    holds exact zeros elsewhere) and the problem stays well conditioned, but exp of a score without the row maximum
    taken off -- or with the maximum of the wrong 16 lanes -- is inf.  300 subtracted: the LeakyReLU branch gives -60,
    whose exp must underflow in the softmax without a trace."""
    C = widths[0] + widths[2]
    ker = _kernels(widths, 1300 + C)["rows"]
    channels = {"first": [0], "last": [C - 1], "each_block": _spread(C), "minus": [C // 2]}[mode]
    assert mode != "each_block" or len(channels) == (C + 15) // 16
    with torch.no_grad():
        ker.attention_nn[1][1].batch_norm.bias[channels] += -300.0 if mode == "minus" else 300.0
    pos_q, pos_s, x, nbr = _inputs(widths, 70, 53 + C)
    got, rows, ref64 = _three(ker, x, pos_q, pos_s, nbr)
    _held("softmax", "%s %s" % (_tag(widths), mode), widths, got, rows, ref64, channels=channels)


# ---------------------------------------------------------------- D. degenerate geometry and input forms

@pytest.mark.parametrize("widths", [WIDTHS["pos"], WIDTHS["c32"], (11, 17, 6, 17)], ids=_tag)
def test_one_support_point(hip, widths):
    """M = 1: every slot is row 0, every query sits on the support point, dij = 0 on all 16 edges"""
    ker = _kernels(widths, 1500)["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, 70, 61, m=1)
    pos_q = pos_s[0].repeat(70, 1)
    assert int(nbr.abs().max()) == 0
    got, rows, ref64 = _three(ker, x, pos_q, pos_s, nbr)
    _held("degenerate", "%s M=1" % _tag(widths), widths, got, rows, ref64)
    assert torch.equal(got, got[:1].expand_as(got))  # 70 times the same query


@pytest.mark.parametrize("widths", [WIDTHS["pos"], WIDTHS["c32"], (11, 17, 6, 17)], ids=_tag)
def test_sixteen_times_the_same_neighbour(hip, widths):
    ker = _kernels(widths, 1600)["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, 70, 67)
    nbr = nbr[:, 5:6].expand(70, 16).contiguous()
    got, rows, ref64 = _three(ker, x, pos_q, pos_s, nbr)
    _held("degenerate", "%s one neighbour" % _tag(widths), widths, got, rows, ref64)


@pytest.mark.parametrize("widths", [WIDTHS["pos"], WIDTHS["c32"]], ids=_tag)
def test_no_queries(hip, widths):
    from torch_points3d_amd import randla
    ker = _kernels(widths, 1700)["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, 4, 71)
    with torch.no_grad():
        out = randla.randla_lfa_eval(pos_q[:0], pos_s, x, nbr[:0], ker.point_pos_nn, ker.attention_nn)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, (3 if widths[0] is None else widths[0]) + widths[2]) and out.dtype == torch.float32


def test_input_forms(hip):
    """int32 table, features as a column slice of a wider tensor or in float64, query positions as a slice of an (N, 4)
    tensor: bit for bit what contiguous float32 / int64 copies give"""
    widths = (11, 17, 6, 17)
    ker = _kernels(widths, 1800)["rows"]
    pos_q, pos_s, x, nbr = _inputs(widths, 70, 73)
    wide = torch.cat([torch.full((M, 2), 7.0, device=DEV), x, torch.full((M, 3), -7.0, device=DEV)], 1)
    x_slice = wide[:, 2:2 + widths[0]]
    pos4 = torch.cat([pos_q, torch.full((70, 1), 9.0, device=DEV)], 1)
    assert not x_slice.is_contiguous() and not pos4[:, :3].is_contiguous()
    with torch.no_grad():
        want = _one_kernel(ker, x, pos_q, pos_s, nbr)
        forms = {"int32 table": (x, pos_q, nbr.int()), "sliced x": (x_slice, pos_q, nbr), "float64 x": (x.double(), pos_q, nbr),
                 "sliced pos_q": (x, pos4[:, :3], nbr), "all": (x_slice.double(), pos4[:, :3], nbr.int())}
        for name, (xf, pq, nb) in forms.items():
            assert torch.equal(_one_kernel(ker, xf, pq, pos_s, nb), want), name


# ---------------------------------------------------------------- E. the constants follow the module's state

def _edge_linears(ker):
    return [layer[0] for mlp in (ker.point_pos_nn, ker.attention_nn) for layer in mlp]


def _auto_kernel(widths, seed, bias):
    """RandlaKernel(lfa="auto") in eval mode with _kernels' state; bias=False: the Linears of the two edge MLPs have none"""
    ker = _kernels(widths, seed)["auto"]
    if not bias:
        for lin in _edge_linears(ker):
            lin.bias = None
    return ker


def _twin(ker, widths, lfa, bias):
    """a fresh module on `ker`'s state_dict: nothing cached on it"""
    from torch_points3d_amd.randla import RandlaKernel
    Cx, P1, P2, A1 = widths
    twin = RandlaKernel(lfa=lfa, point_pos_nn=[10, P1, P2], attention_nn=[Cx + P2, A1, Cx + P2], global_nn=[Cx + P2, 16])
    if not bias:
        for lin in _edge_linears(twin):
            lin.bias = None
    twin.load_state_dict({k: v.clone() for k, v in ker.state_dict().items()}, strict=True)
    return twin.to(DEV).eval()


def _eval_then_change_then_eval(monkeypatch, bias, change, what):
    from torch_points3d_amd import randla
    widths = WIDTHS["c12"]
    monkeypatch.setitem(randla.LFA_MEASURED_WIN, 16, True)  # "auto" takes the kernel at C = 12 whatever was measured
    calls = []
    real = randla.randla_lfa_eval
    monkeypatch.setattr(randla, "randla_lfa_eval", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    ker = _auto_kernel(widths, 1900, bias)
    pos_q, pos_s, x, nbr = _inputs(widths, 257, 79)
    with torch.no_grad():
        first = ker(x, (pos_q, pos_s), nbr)
    change(ker, x, pos_q, pos_s, nbr)
    assert not ker.training
    with torch.no_grad():
        second = ker(x, (pos_q, pos_s), nbr)
        assert len(calls) == 2  # both eval forwards were the one-kernel pass
        fresh = _twin(ker, widths, "auto", bias)(x, (pos_q, pos_s), nbr)
        rows = _twin(ker, widths, "rows", bias)(x, (pos_q, pos_s), nbr)
    assert len(calls) == 3
    bar = _held("state", what, widths, second, rows, _fp64(ker, pos_q, pos_s, x, nbr))
    assert torch.equal(second, fresh)
    moved = float((second - first).abs().max())
    print("%s: second eval output vs the first %.3e (bar %.3e)" % (what, moved, bar))
    assert moved > bar, (moved, bar)  # the statistics did move: the test would see stale ones


def _train_forward(ker, x, pos_q, pos_s, nbr):
    ker.train()
    ker(x, (pos_q, pos_s), nbr)
    ker.eval()


@pytest.mark.parametrize("bias", [True, False], ids=["as_built", "bias_free"])
def test_eval_after_a_training_pass(hip, monkeypatch, bias):
    """eval, a train-mode forward (the BatchNorm kernels move the running statistics through raw pointers), eval: the
    second eval output is that of the module's state now"""
    _eval_then_change_then_eval(monkeypatch, bias, _train_forward, "train pass, " + ("as built" if bias else "bias-free"))


def test_eval_after_a_replayed_step(hip, monkeypatch):
    """what a replayed captured training step leaves: statistics written with no version counter moved and no Python
    run but dp's fused.note_graph_replay()"""
    from torch_points3d_amd import fused

    def change(ker, *inputs):
        g = torch.Generator().manual_seed(83)
        for m in ker.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                versions = m.running_mean._version, m.running_var._version
                m.running_mean.data.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                assert versions == (m.running_mean._version, m.running_var._version)
        fused.note_graph_replay()

    _eval_then_change_then_eval(monkeypatch, True, change, "replayed step")
