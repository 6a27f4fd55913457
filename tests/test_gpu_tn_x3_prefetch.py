"""The loader loop of the bf16-pipe weight-gradient kernel (csrc/gemm_tn_x3.hip) at its edges.

The loader waves run a main loop of three unconditional steps per pass (one per register stage) that fetches the steps
3 .. steps - 2 of a workgroup, and a general loop for the last four to six steps.  What can go wrong is the hand-over
between the two, so the row counts are built from the launch plan (tp3d_gemm_tn_x3_plan: splits, rows per step) to make
the steps per workgroup 0, 1 and 2 mod 3, unequal between the splits of one launch, and the last row block ragged.

Not covered: a workgroup with fewer than three steps.  The kernel serves M >= 131072 only, a launch has at most 256
splits and a step stages at most 64 rows, so every workgroup of a served shape runs at least 131072 / 64 / 256 = 8 steps;
no entry point reaches the case.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 131072
SHAPES = [(128, 128), (128, 64), (64, 64), (256, 128), (128, 132)]  # (N, K); the last one is the strip form
CASES = ["floor", "mod0", "mod1", "mod2"]
SLOPE = 0.01


def _plan(M, N, K):
    from torch_points3d_amd import _lib
    buf = (ctypes.c_int64 * 8)()
    assert _lib.load().tp3d_gemm_tn_x3_plan(M, N, K, ctypes.addressof(buf)) == 0, (M, N, K)
    return list(buf)


def _steps(M, N, K):
    """(splits, rows per step, steps of the shortest workgroup, workgroups with one step more, rows of the last block)"""
    p = _plan(M, N, K)
    splits, br = p[0], p[5]
    q, r = divmod(-(-M // br), splits)  # row blocks are dealt round-robin to the splits
    return splits, br, q, r, M % br


@functools.lru_cache(maxsize=None)
def _rows(N, K, case):
    """The smallest served M of the case: "floor" = 131072 rows; "modR" = the shortest workgroups run q = R (mod 3) steps,
    some run q + 1, and the last row block is short by five rows."""
    if case == "floor":
        return FLOOR
    want = int(case[3:])
    br = _plan(FLOOR, N, K)[5]
    for blocks in range(FLOOR // br + 1, 3 * FLOOR // br):
        M = blocks * br - 5
        splits, _, q, r, _ = _steps(M, N, K)
        if q % 3 == want and 8 <= r <= splits - 8:  # (at least eight workgroups of either length)
            return M
    raise AssertionError((N, K, case))


@functools.lru_cache(maxsize=1)
def _problem(N, K, case):
    """Operands and references of one case, shared by both walking directions."""
    from torch_points3d_amd import _lib, fused
    M = _rows(N, K, case)
    g = torch.Generator(device=DEV).manual_seed(1000 * N + K + len(case) + M)
    dY = torch.randn(M, N, generator=g, device=DEV)
    Yp = torch.randn(M, K, generator=g, device=DEV) * 1.5 + 0.2
    dA = torch.randn(M, K, generator=g, device=DEV)
    gamma, beta = torch.rand(K, generator=g, device=DEV) + 0.5, torch.randn(K, generator=g, device=DEV) * 0.3
    mean = Yp.mean(0)
    invstd = 1.0 / torch.sqrt(Yp.var(0, unbiased=False) + 1e-5)
    scale = gamma * invstd
    st = _lib.stream_ptr(dY.device)
    act = torch.empty_like(Yp)  # the activated rows, in the forward kernels' expression and order
    _lib.call("tp3d_bn_act_f32", _lib.ptr(Yp), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(beta), SLOPE, M, K, _lib.ptr(act), st)
    ref = torch.mm(dY.double().t(), act.double())
    lib = float((torch.mm(dY.t(), act).double() - ref).abs().max())
    err32 = float((fused.gemm_tn(dY, act, x3=0).double() - ref).abs().max())
    # the reductions of the layer below (the side of the activation's kink decided in fp32, in the kernels' order)
    positive = ((Yp - mean) * scale + beta) > 0
    dz = dA.double() * torch.where(positive, 1.0, SLOPE)
    xh = (Yp.double() - mean.double()) * invstd.double()
    want = torch.stack([dz.sum(0), (dz * xh).sum(0)])
    mag = torch.stack([dz.abs().sum(0), (dz * xh).abs().sum(0)])
    sep = torch.empty(4, K, device=DEV)
    bws = _lib.bn_workspace(M, K, dY.device)
    _lib.call("tp3d_bn_bwd_reduce_f32", _lib.ptr(dA), None, _lib.ptr(Yp), _lib.ptr(scale), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(invstd),
              SLOPE, M, 1, K, 1, _lib.ptr(sep[0]), _lib.ptr(sep[1]), _lib.ptr(sep[2]), _lib.ptr(sep[3]), _lib.ptr(bws), 0, st)
    torch.cuda.synchronize()
    return dict(M=M, dY=dY, Yp=Yp, dA=dA, act=act, mean=mean, invstd=invstd, scale=scale, beta=beta, ref=ref, lib=lib,
                err32=err32, want=want, mag=mag, sep=sep)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_row_counts_reach_every_edge_of_the_loader_loop(N, K, case):
    """the M of each case, built from the plan, has the step counts the case is named for"""
    M = _rows(N, K, case)
    splits, br, q, r, last = _steps(M, N, K)
    assert FLOOR <= M < 3 * FLOOR and q > 6  # (the main loop runs: more than six steps)
    if case == "floor":
        return
    assert q % 3 == int(case[3:]) and 0 < r < splits and last == br - 5, (M, splits, br, q, r, last)


def test_the_cases_of_a_shape_cover_all_three_residues():
    for N, K in SHAPES:
        seen = set()
        for case in CASES[1:]:
            splits, br, q, r, last = _steps(_rows(N, K, case), N, K)
            seen.update([q % 3, (q + 1) % 3])
        assert seen == {0, 1, 2}, (N, K)


def _check_dw(got, P):
    """the bars of test_gemm_tn_x3_matches_fp64 (tests/test_gpu_fused.py).  One dropped or doubled 32-row block would move
    dW by about sqrt(32 / M) = 1.5e-2 of its norm."""
    scale = float(P["ref"].abs().max())
    err = float((got.double() - P["ref"]).abs().max())
    print("M=%d err=%.3e lib=%.3e err32=%.3e scale=%.3e" % (P["M"], err, P["lib"], P["err32"], scale))
    assert err <= max(2.0 * P["lib"], 1e-5 * scale), (err, P["lib"], scale)
    assert err <= 3.0 * P["err32"] + 1e-7 * scale, (err, P["err32"])


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_weight_gradient_and_reductions_at_the_loop_edges(N, K, case, reverse):
    from torch_points3d_amd import _lib, fused
    h = _lib.load()
    P = _problem(N, K, case)
    M, dY, Yp = P["M"], P["dY"], P["Yp"]
    st = _lib.stream_ptr(dY.device)
    floats = _plan(M, N, K)[6]
    stats = (P["mean"], P["scale"], P["beta"], SLOPE)
    # the activated-operand form, into a workspace of its own that starts out as NaN
    ws = torch.full((floats,), float("nan"), device=DEV)
    plain = torch.full((N, K), float("nan"), device=DEV)
    _lib.call("tp3d_gemm_tn_x3_act_f32", _lib.ptr(dY), _lib.ptr(Yp), _lib.ptr(P["mean"]), _lib.ptr(P["scale"]), _lib.ptr(P["beta"]),
              SLOPE, M, N, K, 6, _lib.ptr(plain), _lib.ptr(ws), reverse, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all())
    assert torch.equal(plain, fused.gemm_tn(dY, Yp, x3=6, act=stats, reverse=reverse))
    # ... forms the rows tp3d_bn_act_f32 writes: the form without a prologue on those rows gives the same bits
    assert torch.equal(plain, fused.gemm_tn(dY, P["act"], x3=6, reverse=reverse))
    _check_dw(plain, P)
    chunks = h.tp3d_gemm_tn_x3_red_chunks(M, N, K)
    if K > 128:
        assert chunks == 0  # (the strip form carries no reductions)
        return
    assert chunks > 0
    ws.fill_(float("nan"))
    rws = torch.full((chunks * 2 * K,), float("nan"), device=DEV)
    out = torch.full((N, K), float("nan"), device=DEV)
    red = torch.full((4, K), float("nan"), device=DEV)
    _lib.call("tp3d_gemm_tn_x3_act_red_f32", _lib.ptr(dY), _lib.ptr(Yp), _lib.ptr(P["mean"]), _lib.ptr(P["scale"]), _lib.ptr(P["beta"]),
              _lib.ptr(P["invstd"]), SLOPE, _lib.ptr(P["dA"]), 1, M, N, K, 6, _lib.ptr(out), _lib.ptr(ws), _lib.ptr(red), _lib.ptr(rws),
              reverse, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(rws).all())
    assert torch.equal(out, plain)
    _check_dw(out, P)
    # the bars of test_weight_gradient_kernel_also_reduces_the_layer_below
    e64 = float(((red[:2].double() - P["want"]).abs() / P["mag"]).max())
    esep = float(((red[:2] - P["sep"][:2]).double().abs() / P["mag"]).max())
    print("reductions: vs float64 %.3e, vs tp3d_bn_bwd_reduce_f32 %.3e" % (e64, esep))
    assert e64 < 1e-6 and esep < 1e-6
    torch.testing.assert_close(red[2], red[0] / M, rtol=1e-6, atol=0)
    torch.testing.assert_close(red[3], P["invstd"] * (red[1] / M), rtol=1e-6, atol=0)
