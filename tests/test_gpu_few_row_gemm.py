"""The few-row tile rule (fused.FEW_ROW_TILES, csrc/gemm_plans.h) changes which workgroup computes an output element,
never how: every entry point it bears on is run with the switch at 0 and at 1 on the same inputs and every output must
be torch.equal.  No tolerance is involved -- the old route is the reference and has its own float64 tests.

Forward: tp3d_gemm_rows_f32 (C, the raw statistics buffer, mean / invstd after tp3d_bn_finalize_f32) and
tp3d_gemm_rows_epi_f32 on the 64 x 64 form of the plain wide kernel.  That form runs one work item per workgroup (at most
1024 of either), so there is no case with more items than workgroups: it cannot walk several.
Weight gradient: tp3d_gemm_tn_f32 with the tile chosen by fill, the row split untouched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7777.0

ROWS_M = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000]  # ragged last half-block, whole padding items
ROWS_K = [4, 8, 28, 32, 36, 64, 260]  # one step, tail groups of 1 and 4, several steps with a 4-column tail
TN_M = [1, 63, 64, 65, 256, 257, 1000, 4096]
TN_NK = [(64, 64), (128, 128), (256, 256), (256, 260), (128, 256), (512, 256), (10, 128)]


def _plan(name, n, *args):
    from torch_points3d_amd import _lib
    buf = (ctypes.c_int64 * n)()
    assert getattr(_lib.load(), name)(*args, ctypes.addressof(buf)) == 0, (name, args)
    return list(buf)


@pytest.fixture
def few_row():
    from torch_points3d_amd import fused
    saved = fused.FEW_ROW_TILES

    def use(v):
        fused.FEW_ROW_TILES = v
        fused.sync_few_row_tiles()
    yield use
    use(saved)


def _guarded(numel, margin=4096):
    """(whole buffer, the `numel` floats in its middle): sentinel margins on both sides of an output"""
    whole = torch.full((margin + numel + margin,), SENTINEL, device=DEV)
    return whole, whole[margin:margin + numel]


def _margins_intact(whole, numel, margin=4096):
    return bool((whole[:margin] == SENTINEL).all()) and bool((whole[margin + numel:] == SENTINEL).all())


def _rows_operands(M, N, K, const_col):
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    A[:, 0] = 2.5   # with W[const_col] = e_0: column const_col of C is 2.5 in every row
    W[const_col] = 0.0
    W[const_col, 0] = 1.0
    return A.to(DEV), W.to(DEV)


def _rows(A, W, stats, guard=False):
    """tp3d_gemm_rows_f32 -> (C, raw statistics buffer or None, margins intact)"""
    from torch_points3d_amd import _lib
    M, K = A.shape
    N = W.shape[0]
    h = _lib.load()
    cw, C = _guarded(M * N) if guard else (None, torch.full((M * N,), SENTINEL, device=DEV))
    part = pw = None
    if stats:
        floats = h.tp3d_gemm_rows_stat_floats(M, N)
        pw, part = _guarded(floats) if guard else (None, torch.full((floats,), SENTINEL, device=DEV))
    _lib.call("tp3d_gemm_rows_f32", A.data_ptr(), W.data_ptr(), M, N, K, C.data_ptr(), _lib.ptr(part), None, _lib.stream_ptr(A.device))
    ok = True
    if guard:
        ok = _margins_intact(cw, M * N) and (pw is None or _margins_intact(pw, part.numel()))
    return C.view(M, N), part, ok


def _finalize(part, M, N):
    from torch_points3d_amd import _lib
    chunks = _lib.load().tp3d_gemm_rows_stat_chunks(M, N)
    stats = torch.empty(4, N, device=DEV)
    gamma, beta = torch.full((N,), 1.5, device=DEV), torch.full((N,), 0.25, device=DEV)
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    _lib.call("tp3d_bn_finalize_f32", part.data_ptr(), chunks, M, N, 1e-5, 0.1, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), nbt.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(),
              _lib.stream_ptr(part.device))
    return stats, rm, rv


# N = 132 leaves a 4-column remainder tile: rows_plan serves it with 128 x 64 tiles, which the rule leaves alone (both
# settings launch the same kernel); N = 200 is the wide plan with a ragged last column tile
@pytest.mark.parametrize("N", [128, 132, 256, 200])
def test_rows_gemm_small_tiles_bit_identical(N, few_row):
    const_col = 5
    for M in ROWS_M:
        for K in ROWS_K:
            A, W = _rows_operands(M, N, K, const_col)
            out = {}
            for v in (0, 1):
                few_row(v)
                routed = _plan("tp3d_gemm_rows_small_plan", 4, M, N, K)[2]
                assert routed == int(v == 1 and N != 132), (M, N, K, v)
                C0, _, _ = _rows(A, W, stats=False)
                C1, part, _ = _rows(A, W, stats=True)
                out[v] = (C0, C1, part) + tuple(_finalize(part, M, N))
            for a, b in zip(out[0], out[1]):
                assert torch.equal(a, b), (M, N, K)
            C0, C1, part = out[1][:3]
            assert torch.equal(C0, C1) and not bool((C0 == SENTINEL).any()), (M, N, K)
            assert bool((C0[:, const_col] == 2.5).all()), (M, N, K)
            chunks = _plan("tp3d_gemm_rows_plan", 9, M, N, K)[4]
            chunk = part[:chunks * 4 * N].view(chunks, 4, N)
            assert not bool((chunk == SENTINEL).any()), (M, N, K)  # every slot of every chunk written
            # the constant column: the shift equals every value, so both shifted sums are exactly zero in every chunk
            # (a chunk without rows -- the empty lower half of a ragged block -- has shift 0 and sums 0)
            assert bool((chunk[:, 0, const_col] == 0).all()) and bool((chunk[:, 1, const_col] == 0).all()), (M, N, K)
            assert float(chunk[:, 3, 0].sum()) == M, (M, N, K)  # the rows every chunk counted


@pytest.mark.parametrize("M,N,K", [(200, 256, 260), (1000, 128, 36), (65, 200, 64), (4096, 256, 256)])
def test_rows_gemm_eval_epilogue_small_tiles_bit_identical(M, N, K, few_row):
    from torch_points3d_amd import _lib
    A, W = _rows_operands(M, N, K, 5)
    g = torch.Generator().manual_seed(7)
    mean, scale, beta = (torch.randn(N, generator=g).to(DEV), (torch.rand(N, generator=g) + 0.5).to(DEV),
                         torch.randn(N, generator=g).to(DEV))
    out = {}
    for v in (0, 1):
        few_row(v)
        assert _plan("tp3d_gemm_rows_small_plan", 4, M, N, K)[3] == v
        C = torch.full((M, N), SENTINEL, device=DEV)
        _lib.call("tp3d_gemm_rows_epi_f32", A.data_ptr(), W.data_ptr(), M, N, K, mean.data_ptr(), scale.data_ptr(), beta.data_ptr(),
                  0.1, C.data_ptr(), None, _lib.stream_ptr(A.device))
        out[v] = C
    assert torch.equal(out[0], out[1]) and not bool((out[1] == SENTINEL).any())


@pytest.mark.parametrize("M,N,K", [(129, 200, 36), (1000, 256, 260)])
def test_rows_gemm_small_tiles_write_inside_their_outputs(M, N, K, few_row):
    """C and the statistics buffer between sentinel margins: ragged rows, a ragged column tile, padding workgroups"""
    few_row(1)
    assert _plan("tp3d_gemm_rows_small_plan", 4, M, N, K)[2] == 1
    A, W = _rows_operands(M, N, K, 5)
    C, part, intact = _rows(A, W, stats=True, guard=True)
    assert intact
    few_row(0)
    C0, part0, _ = _rows(A, W, stats=True)
    assert torch.equal(C, C0) and torch.equal(part, part0)


def _tn(dY, A, guard=False):
    from torch_points3d_amd import _lib
    M, N = dY.shape
    K = A.shape[1]
    ws = torch.empty(max(1, _lib.load().tp3d_gemm_tn_workspace_floats(M, N, K)), device=DEV)
    whole, out = _guarded(N * K) if guard else (None, torch.full((N * K,), SENTINEL, device=DEV))
    _lib.call("tp3d_gemm_tn_f32", dY.data_ptr(), A.data_ptr(), M, N, K, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dY.device))
    return out.view(N, K), (not guard) or _margins_intact(whole, N * K)


@pytest.mark.parametrize("N,K", TN_NK)
def test_gemm_tn_tile_by_fill_bit_identical(N, K, few_row):
    for M in TN_M:
        g = torch.Generator().manual_seed(M + 7 * N + K)
        dY, A = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV)
        plans, outs = {}, {}
        for v in (0, 1):
            few_row(v)
            plans[v] = _plan("tp3d_gemm_tn_plan", 8, M, N, K)
            outs[v] = _tn(dY, A)[0]
        assert plans[0][:2] == plans[1][:2], (M, N, K)  # splits and rows per split: the summation order
        assert torch.equal(outs[0], outs[1]) and not bool((outs[1] == SENTINEL).any()), (M, N, K)
        if (N, K) == (10, 128):
            assert plans[0] == plans[1] and plans[1][2:4] == [32, 128], (M, N, K)  # the one-wave-row form is untouched
        elif M == 4096 and (N, K) != (64, 64):  # (64 x 64 is the smallest tile there is: nothing to change to)
            assert plans[0][2:4] != plans[1][2:4], (M, N, K, plans)
        elif M == 4096:
            assert plans[0][2:4] == plans[1][2:4] == [64, 64]


def test_gemm_tn_small_tile_writes_inside_its_output(few_row):
    few_row(1)
    M, N, K = 1000, 256, 260
    assert _plan("tp3d_gemm_tn_plan", 8, M, N, K)[2:4] == [64, 64]
    g = torch.Generator().manual_seed(3)
    dY, A = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV)
    out, intact = _tn(dY, A, guard=True)
    assert intact
    few_row(0)
    assert torch.equal(out, _tn(dY, A)[0])
