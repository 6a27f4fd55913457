"""Loader loops of the split-role rows GEMMs (csrc/gemm_rows_sp.hip, csrc/gemm_rows_x3.hip) on every path through a pair
loop and its tail, and both store paths of the epilogue: one, two, three, four, six and eight K-steps per workgroup, workgroups of one launch with different
step counts, a short last K-step, a ragged last row block, both tile widths, both row orders, with and without the side
output and the statistics, the dense and the pooled backward form.  References and bars are those of test_gpu_fused.py for
the same entry point: the two-kernel composition tp3d_bn_act_f32 + tp3d_gemm_rows_f32, the float64 backward formula for
the dY side output, the fp32 kernel's own distance to float64 for the bf16-pipe form."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.01
# include/tp3d_hip.h: the kernels serve "at least 512 output tiles"; a tile has 128 rows and the row blocks are rounded up
# to groups of 8, so the first served M is one row into the group that completes 512 items
MIN_ITEMS, ROWS, GROUP = 512, 128, 8


def _first_served(serves):
    lo, hi = 1, 1 << 22
    assert not serves(lo) and serves(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if serves(mid) else (mid, hi)
    return hi


def _rows_for(serves, items, short):
    """The row count with `items` work items (one column tile), `short` rows missing from the last row block -- from the
    entry point's own shape rule: its first served M starts the group of row blocks that completes MIN_ITEMS items."""
    first = _first_served(serves)
    assert (first - 1) % (GROUP * ROWS) == 0
    M = first - 1 + (items - MIN_ITEMS + GROUP) * ROWS - short
    assert serves(M) and 0 <= short < ROWS
    return M


def _walks(rows_per_chunk, items, grid, M):
    """Statistics chunks (one per workgroup and wave row, 64 rows of every item the workgroup walked): the launch reached
    `items` items -- every row counted once, and the workgroups of the longer walk are as many as the item count says."""
    assert int(rows_per_chunk.sum()) == M
    lo = items // grid
    if items % grid:
        assert int((rows_per_chunk > 64 * lo).sum()) == 2 * (items - lo * grid)
        assert int(rows_per_chunk.max()) <= 64 * (lo + 1)
    else:
        assert int(rows_per_chunk.max()) == 64 * lo


def _forward_case(M, N, K):
    """Inputs and the references of one forward shape, computed once for all its launches: the activated rows of
    tp3d_bn_act_f32, the product of tp3d_gemm_rows_f32 on them, the float64 product."""
    from torch_points3d_amd import _lib, fused
    g = torch.Generator().manual_seed(M + N + K)
    Y = (torch.randn(M, K, generator=g) * 2 + 0.3).to(DEV)
    Bt = (torch.randn(N, K, generator=g) * 0.2).to(DEV)
    mean, scale, beta = (torch.randn(K, generator=g) * 0.2).to(DEV), (torch.rand(K, generator=g) + 0.5).to(DEV), \
        (torch.randn(K, generator=g) * 0.3).to(DEV)
    st = _lib.stream_ptr(Y.device)
    act_ref = torch.empty_like(Y)
    _lib.call("tp3d_bn_act_f32", _lib.ptr(Y), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(beta), SLOPE, M, K, _lib.ptr(act_ref), st)
    ref32 = fused.gemm_rows(act_ref, Bt)[0]
    act64 = torch.nn.functional.leaky_relu((Y.double() - mean.double()) * scale.double() + beta.double(), SLOPE)
    ref64 = act64 @ Bt.double().t()
    return Y, Bt, mean, scale, beta, act_ref, ref32, ref64


def _forward(entry, chunk_fn, case, M, N, K, stats, side, reverse):
    from torch_points3d_amd import _lib
    Y, Bt, mean, scale, beta = case[:5]
    chunks = chunk_fn(M, N, K, 1 if side else 0)
    assert chunks > 0
    out = torch.full((M, N), float("nan"), device=DEV)
    act = torch.full((M, K), float("nan"), device=DEV) if side else None
    part = torch.full((chunks * 4 * N + 64,), float("nan"), device=DEV) if stats else None
    _lib.call(entry, _lib.ptr(Y), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(beta), SLOPE, _lib.ptr(Bt), M, N, K, _lib.ptr(out),
              _lib.ptr(part), _lib.ptr(act), reverse, _lib.stream_ptr(Y.device))
    return out, act, part, chunks


def _finalized(part, chunks, M, N):
    from torch_points3d_amd import _lib, fused
    assert bool(torch.isnan(part[chunks * 4 * N:]).all()) and not bool(torch.isnan(part[:chunks * 4 * N]).any())
    bn = torch.nn.BatchNorm1d(N).to(DEV)
    return fused._finalize_stats(part.clone(), M, N, bn.weight.detach(), bn.bias.detach(), bn, part.device,
                                 _lib.stream_ptr(part.device), chunks)


def _forward_variants(entry, chunk_fn, case, M, N, K, items, first, stats0):
    """Every other output combination and the reversed walk against the full forward-order launch: the same rows bit for
    bit, statistics that are the same sums in another order."""
    out, act = first
    std = out.double().std(0, unbiased=False)
    for stats, side, reverse in ((True, True, 1), (False, False, 0), (False, False, 1), (True, False, 0), (False, True, 1)):
        o, a, p, chunks = _forward(entry, chunk_fn, case, M, N, K, stats, side, reverse)
        assert torch.equal(o, out), (stats, side, reverse)
        if side:
            assert torch.equal(a, act), (stats, side, reverse)
        if stats:
            if not reverse:
                _walks(p[:chunks * 4 * N].view(chunks, 4, N)[:, 3, 0], items, chunks // 2, M)
            s = _finalized(p, chunks, M, N)
            assert float(((s[0] - stats0[0]).double().abs() / std).max()) < 1e-5, (stats, side, reverse)
            torch.testing.assert_close(s[1], stats0[1], rtol=2e-5, atol=0)


# (items, K, N, rows missing from the last block): K-steps of 32 -- totals 1; 1 and 2; 3 and 6; 4 and 8; 3 and 4; a short
# last step (K = 100: four steps, the last four wide); both tile widths
SP_CASES = [(512, 32, 128, 5), (520, 32, 64, 5), (520, 96, 128, 5), (520, 128, 64, 0), (1544, 32, 128, 5), (512, 100, 128, 5),
            (520, 100, 64, 5)]


@pytest.mark.parametrize("items,K,N,short", SP_CASES)
def test_fp32_forward_on_every_loader_path(items, K, N, short):
    from torch_points3d_amd import _lib
    h = _lib.load()
    M = _rows_for(lambda m: h.tp3d_gemm_rows_sp_chunks(m, N, K, 1) > 0, items, short)
    case = _forward_case(M, N, K)
    act_ref, ref32 = case[5], case[6]
    out, act, part, chunks = _forward("tp3d_gemm_rows_bnact_sp_f32", h.tp3d_gemm_rows_sp_chunks, case, M, N, K, True, True, 0)
    assert torch.equal(act, act_ref)
    torch.testing.assert_close(out, ref32, rtol=1e-5, atol=1e-5 * float(ref32.abs().max()))
    _walks(part[:chunks * 4 * N].view(chunks, 4, N)[:, 3, 0], items, chunks // 2, M)
    stats = _finalized(part, chunks, M, N)
    o64 = out.double()
    std = o64.std(0, unbiased=False)
    assert float(((stats[0].double() - o64.mean(0)).abs() / std).max()) < 1e-5
    torch.testing.assert_close(stats[1].double(), 1.0 / torch.sqrt(o64.var(0, unbiased=False) + 1e-5), rtol=2e-5, atol=0)
    _forward_variants("tp3d_gemm_rows_bnact_sp_f32", h.tp3d_gemm_rows_sp_chunks, case, M, N, K, items, (out, act), stats)


# K-steps of 16 -- totals 1; 1 and 2; 3 and 6; 4 and 8; 3 and 4; a strip width (K = 132: nine steps, the last four wide)
X3_CASES = [(512, 16, 128, 5), (520, 16, 128, 5), (520, 48, 128, 5), (520, 64, 128, 0), (1544, 16, 128, 5), (520, 132, 128, 5)]


@pytest.mark.parametrize("items,K,N,short", X3_CASES)
def test_bf16_pipe_forward_on_every_loader_path(items, K, N, short):
    from torch_points3d_amd import _lib
    h = _lib.load()
    M = _rows_for(lambda m: h.tp3d_gemm_rows_x3_chunks(m, N, K, 1) > 0, items, short)
    case = _forward_case(M, N, K)
    act_ref, ref64 = case[5], case[7]
    o_sp, _, p_sp, c_sp = _forward("tp3d_gemm_rows_bnact_sp_f32", h.tp3d_gemm_rows_sp_chunks, case, M, N, K, True, False, 0)
    out, act, part, chunks = _forward("tp3d_gemm_rows_bnact_x3_f32", h.tp3d_gemm_rows_x3_chunks, case, M, N, K, True, True, 0)
    assert torch.equal(act, act_ref)
    scale_c = float(ref64.abs().max())
    e_sp, e_x3 = float((o_sp.double() - ref64).abs().max()) / scale_c, float((out.double() - ref64).abs().max()) / scale_c
    assert e_x3 < 1e-6 and e_x3 < 1.5 * e_sp + 1e-7, (e_sp, e_x3)
    _walks(part[:chunks * 4 * N].view(chunks, 4, N)[:, 3, 0], items, chunks // 2, M)
    stats, s_sp = _finalized(part, chunks, M, N), _finalized(p_sp, c_sp, M, N)
    std = ref64.std(0, unbiased=False)
    assert float(((stats[0].double() - ref64.mean(0)).abs() / std).max()) < 1e-5
    torch.testing.assert_close(stats[1], s_sp[1], rtol=2e-5, atol=0)
    _forward_variants("tp3d_gemm_rows_bnact_x3_f32", h.tp3d_gemm_rows_x3_chunks, case, M, N, K, items, (out, act), stats)


def _backward(args, M, N, K, dA, arg, ns, side, reverse, pads=None):
    """One launch of the input-gradient form into a NaN-filled (or, with pads, 7-filled wider) C; returns (C, dY)."""
    from torch_points3d_amd import _lib
    Y, Wt, mean, scale, beta, c1, c2 = args
    dY = torch.full((M, K), float("nan"), device=DEV) if side else None
    if pads is None:
        out, ldc, lo, hi = torch.full((M, N), float("nan"), device=DEV), N, 0, 0
        c_ptr = out.data_ptr()
    else:
        lo, hi = pads
        out, ldc = torch.full((M, N + 8), 7.0, device=DEV), N + 8
        c_ptr = out.data_ptr() + 4 * 3  # the product goes to columns 3 .. 3 + N of the wider rows
    _lib.call("tp3d_gemm_rows_bnbwd_sp_f32", _lib.ptr(Y), _lib.ptr(dA), _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(beta), _lib.ptr(c1),
              _lib.ptr(c2), SLOPE, _lib.ptr(Wt), M, N, K, c_ptr, ldc, lo, hi, _lib.ptr(dY), _lib.ptr(arg), ns, reverse,
              _lib.stream_ptr(Y.device))
    return out, dY


def _pads_written(wide, out, N):
    """Three zero columns in front of the product, four of the five behind it, the last one untouched."""
    assert torch.equal(wide[:, 3:3 + N], out)
    assert bool((wide[:, :3] == 0).all()) and bool((wide[:, 3 + N:3 + N + 4] == 0).all()) and bool((wide[:, 3 + N + 4:] == 7).all())


# totals 1; 1 and 2; 3 and 6; 4 and 8; 3 and 4; a short last step; both tile widths
BWD_CASES = [(512, 32, 128, 5), (520, 32, 64, 5), (520, 96, 64, 5), (520, 128, 128, 0), (1544, 32, 128, 5), (520, 100, 128, 5)]


@pytest.mark.parametrize("items,K,N,short", BWD_CASES)
def test_dense_input_gradient_on_every_loader_path(items, K, N, short):
    from torch_points3d_amd import _lib
    h = _lib.load()
    M = _rows_for(lambda m: h.tp3d_gemm_rows_bnbwd_sp_serves(m, N, K) == 1, items, short)
    assert M == _rows_for(lambda m: h.tp3d_gemm_rows_sp_chunks(m, N, K, 1) > 0, items, short)  # (the forward form's item count)
    g = torch.Generator().manual_seed(M + N + K)
    Y = (torch.randn(M, K, generator=g) * 1.5 + 0.2).to(DEV)
    dA = torch.randn(M, K, generator=g).to(DEV)
    Wt = (torch.randn(N, K, generator=g) * 0.2).to(DEV)
    gamma, beta = (torch.rand(K, generator=g) + 0.5).to(DEV), (torch.randn(K, generator=g) * 0.3).to(DEV)
    mean = Y.double().mean(0)
    invstd = 1.0 / torch.sqrt(Y.double().var(0, unbiased=False) + 1e-5)
    mean32, invstd32 = mean.float(), invstd.float()
    scale = (gamma.double() * invstd).float()
    st = _lib.stream_ptr(Y.device)
    red = torch.empty(4, K, device=DEV)
    ws = _lib.bn_workspace(M, K, Y.device)
    _lib.call("tp3d_bn_bwd_reduce_f32", _lib.ptr(dA), None, _lib.ptr(Y), _lib.ptr(scale), _lib.ptr(beta), _lib.ptr(mean32),
              _lib.ptr(invstd32), SLOPE, M, 1, K, 1, _lib.ptr(red[0]), _lib.ptr(red[1]), _lib.ptr(red[2]), _lib.ptr(red[3]), _lib.ptr(ws), 0, st)
    args = (Y, Wt, mean32, scale, beta, red[2], red[3])
    out, dY = _backward(args, M, N, K, dA, None, 1, True, 0)
    yc = Y.double() - mean32.double()
    z = yc * scale.double() + beta.double()
    dz = dA.double() * torch.where(z > 0, 1.0, SLOPE)
    xhat = yc * invstd32.double()
    want = scale.double() * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))
    err = (dY.double() - want).abs()
    err[z.abs() < 1e-5] = 0
    assert float(err.max()) < 2e-5 * float(want.abs().max())
    ref = dY.double() @ Wt.double().t()
    assert float((out.double() - ref).abs().max()) < 1e-5 * float(ref.abs().max()) + 1e-6
    for side, reverse in ((True, 1), (False, 0), (False, 1)):
        o, d = _backward(args, M, N, K, dA, None, 1, side, reverse)
        assert torch.equal(o, out), (side, reverse)
        assert d is None or torch.equal(d, dY)
    for reverse in (0, 1):
        wide, _ = _backward(args, M, N, K, dA, None, 1, False, reverse, pads=(3, 4))
        _pads_written(wide, out, N)


# ns = 64 with M a multiple of 64 but not of 128: the last row block holds one group
@pytest.mark.parametrize("items,K,N,short,ns", [(512, 32, 128, 64, 64), (520, 32, 64, 64, 64), (520, 96, 128, 0, 128), (520, 128, 64, 64, 64),
                                                (1544, 32, 128, 64, 64), (520, 100, 128, 64, 64)])
def test_pooled_input_gradient_on_every_loader_path(items, K, N, short, ns):
    """The pooled form against the dense form of the same kernel on the scattered gradient: dY and the product bit for bit
    (the dense form stands against float64 above), both row orders, the pad columns."""
    from torch_points3d_amd import _lib
    h = _lib.load()
    M = _rows_for(lambda m: h.tp3d_gemm_rows_bnbwd_sp_serves(m, N, K) == 1, items, short)
    assert M % ns == 0 and (short == 0 or M % ROWS)
    g = torch.Generator().manual_seed(M + ns + K)
    G = M // ns
    Y = (torch.randn(M, K, generator=g) * 1.5 + 0.2).to(DEV)
    dP = torch.randn(G, K, generator=g).to(DEV)
    arg = torch.randint(0, ns, (G, K), generator=g, dtype=torch.int32).to(DEV)
    dense = torch.zeros(G, ns, K, device=DEV)
    dense.scatter_(1, arg.long().unsqueeze(1), dP.unsqueeze(1))
    dense = dense.view(M, K).contiguous()
    Wt = (torch.randn(N, K, generator=g) * 0.2).to(DEV)
    mean, scale, beta = (torch.randn(K, generator=g) * 0.2).to(DEV), (torch.rand(K, generator=g) + 0.5).to(DEV), \
        (torch.randn(K, generator=g) * 0.3).to(DEV)
    c1, c2 = (torch.randn(K, generator=g) * 0.01).to(DEV), (torch.randn(K, generator=g) * 0.01).to(DEV)
    args = (Y, Wt, mean, scale, beta, c1, c2)
    out, dY = _backward(args, M, N, K, dense, None, 1, True, 0)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dY).any())
    for side, reverse in ((True, 0), (True, 1), (False, 1)):
        o, d = _backward(args, M, N, K, dP, arg, ns, side, reverse)
        assert torch.equal(o, out), (side, reverse)
        assert d is None or torch.equal(d, dY)
    wide, _ = _backward(args, M, N, K, dP, arg, ns, False, 0, pads=(3, 4))
    _pads_written(wide, out, N)
