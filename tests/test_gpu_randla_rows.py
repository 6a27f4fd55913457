"""The RandLA-Net row kernels (csrc/randla.hip, csrc/gemm_skinny.hip, the k = 1 use of knn_interpolate_kernel) against
float64 at every lane layout, width and route, and RandlaKernel on a ragged batch with a cloud smaller than k.

"What is written" is checked through the C-ABI on buffers pre-filled with NaN (or a sentinel where a region must stay
untouched), so no result depends on what the allocator hands back.  Every comparison prints `[rows:<section>] what
err bar ratio`; floating-point bars are stated where they are used."""
import copy
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 0x4B3C614E  # bit pattern of the "must stay untouched" float


def _pad4(c):
    return (c + 3) // 4 * 4


def _report(section, what, err, bar):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    print("[rows:%s] %s: err %.3g bar %.3g ratio %.3g" % (section, what, err, bar, ratio))
    return ratio


def _close64(section, what, got, ref32, ref64, rtol=1e-5, atol=1e-5):
    """|got - ref64| <= max(atol * max(1, |ref64|max) + rtol |ref64|, 2 |ref32 - ref64|max) element-wise (the rule of
    tests/test_gpu_ppnet.py::_close64); ref32 = the plain-torch fp32 evaluation of the same formula, or None"""
    if ref64.numel() == 0:
        return
    ref64 = ref64.double()
    err = (got.detach().double() - ref64).abs()
    own = 0.0 if ref32 is None else float((ref32.double() - ref64).abs().max())
    bar = torch.clamp(atol * max(1.0, float(ref64.abs().max())) + rtol * ref64.abs(), min=2.0 * own)
    ratio = float((err / bar).max())
    print("[rows:%s] %s: |hip - ref64|max %.3g, |torch32 - ref64|max %.3g, |ref|max %.3g, bar>= %.3g, ratio %.3g"
          % (section, what, float(err.max()), own, float(ref64.abs().max()), float(bar.min()), ratio))
    assert ratio <= 1.0, "%s: |hip - ref64| is %.3g x its bar" % (what, ratio)  # (a NaN fails this too)


# ---------------------------------------------------------------------------------------------------------------------
# 1. attentive pooling
# ---------------------------------------------------------------------------------------------------------------------
PAIRS = [(1, 1), (3, 17), (4, 16), (5, 9), (8, 8), (9, 5), (16, 3), (17, 3), (32, 2), (33, 2), (64, 1), (65, 4),
         (128, 16), (129, 3), (192, 2), (193, 3), (256, 16)]  # P = 4..64, R = 1..4, k below / at / past 64 / P
SMALL_NQ = [(1, 1), (5, 9), (17, 3), (65, 4), (256, 16)]  # the 4-waves-per-block tail: Nq = 1..5
LOGITS = ("randn", "shift", "peak", "equal")
MISSING = ("null", "tail", "first", "interior", "allq")


def _lanes(C):
    P = 4
    while P < 64 and P < C:
        P *= 2
    return P


def _ldgs(C):
    return [C, C + 2, _pad4(C) + 4]


def _ldfs(C):
    out = [C, _pad4(C)]
    if C + 4 * _lanes(C) + 3 <= 256:
        out.append(C + 4 * _lanes(C) + 3)
    out.append(256)
    return list(dict.fromkeys(out))


def _logits(kind, E, C, gen):
    if kind == "randn":
        return 3 * torch.randn(E, C, generator=gen)
    if kind == "shift":  # needs the row maximum subtracted
        return 3 * torch.randn(E, C, generator=gen) + 1e4
    if kind == "peak":  # one logit >= 90 above the others: they underflow
        g = torch.randn(E, C, generator=gen).clamp(-5, 5)
        g[torch.arange(E), torch.randint(0, C, (E,), generator=gen)] = 95.0
        return g
    return torch.randn(E, 1, generator=gen).expand(E, C).clone()  # all equal within a row


def _table(kind, Nq, k, gen):
    if kind == "null":
        return None
    nbr = torch.randint(0, 1000, (Nq, k), generator=gen)
    if kind == "tail":
        nbr[::2, k - k // 2:] = -1
    elif kind == "first":
        nbr[::2, 0] = -1
    elif kind == "interior":
        nbr[::2, min(k - 1, max(1, k // 2))] = -1
    else:
        nbr[Nq // 2, :] = -1
    return nbr


def _attn_formula(g, f, keep, cot, Nq, k, C):
    g, f = g.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = (torch.softmax(g, -1) * f * keep.to(g.dtype)).reshape(Nq, k, C).sum(1)
    (out * cot.to(g.dtype)).sum().backward()
    return out.detach(), g.grad, f.grad


def _attn_run(C, k, Nq, ldg, ldf, logit, missing, seed):
    from torch_points3d_amd import _lib
    gen = torch.Generator().manual_seed(seed)
    E = Nq * k
    what = "C%d k%d Nq%d ldg%d ldf%d %s %s" % (C, k, Nq, ldg, ldf, logit, missing)
    g = torch.full((E, ldg), NAN)
    f = torch.full((E, ldf), NAN)  # padding columns hold NaN: they must not reach any output
    g[:, :C] = _logits(logit, E, C, gen)
    f[:, :C] = torch.randn(E, C, generator=gen)
    cot = torch.randn(Nq, C, generator=gen).to(DEV)
    nbr = _table(missing, Nq, k, gen)
    keep = torch.ones(E, 1) if nbr is None else (nbr.reshape(-1, 1) >= 0).float()
    g, f, keep = g.to(DEV), f.to(DEV), keep.to(DEV)
    nbr = None if nbr is None else nbr.to(DEV)
    out = torch.full((Nq, C), NAN, device=DEV)
    dg = torch.full((E, ldg), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    df = torch.full((E, ldf), NAN, device=DEV)
    st = _lib.stream_ptr(out.device)
    _lib.call("tp3d_attn_pool_fwd_f32", _lib.ptr(g), _lib.ptr(f), _lib.ptr(nbr), Nq, k, C, ldg, ldf, _lib.ptr(out), st)
    _lib.call("tp3d_attn_pool_bwd_f32", _lib.ptr(g), _lib.ptr(f), _lib.ptr(cot), _lib.ptr(nbr), Nq, k, C, ldg, ldf,
              _lib.ptr(dg), _lib.ptr(df), st)
    gc, fc = g[:, :C].contiguous(), f[:, :C].contiguous()
    o64, dg64, df64 = _attn_formula(gc.double(), fc.double(), keep, cot, Nq, k, C)
    o32, dg32, df32 = _attn_formula(gc, fc, keep, cot, Nq, k, C)
    _close64("attn", what + " out", out, o32, o64)
    _close64("attn", what + " dg", dg[:, :C], dg32, dg64)
    _close64("attn", what + " df", df[:, :C], df32, df64)
    # every padding column of df is overwritten with 0; dg beyond C keeps the caller's bits
    assert torch.count_nonzero(df[:, C:]) == 0 and not bool(torch.isnan(df[:, C:]).any()), what
    assert bool((dg.view(torch.int32)[:, C:] == SENTINEL).all()), what
    gone = keep.reshape(-1) == 0
    assert torch.count_nonzero(dg[gone, :C]) == 0 and torch.count_nonzero(df[gone]) == 0, what  # exact zeros
    if missing == "allq":
        assert torch.count_nonzero(out[Nq // 2]) == 0, what


def _attn_sweep(C, k, Nq, shift):
    combos = list(itertools.product(LOGITS, MISSING))
    widths = list(itertools.product(_ldgs(C), _ldfs(C)))
    for i, (logit, missing) in enumerate(combos):
        ldg, ldf = widths[(i + shift) % len(widths)]
        _attn_run(C, k, Nq, ldg, ldf, logit, missing, 1000 * C + 10 * k + i)


@pytest.mark.parametrize("C,k", PAIRS)
def test_attentive_pool_layouts(hip, C, k):
    """every lane layout x logit family x missing-slot pattern, the widths rotating through all (ldg, ldf) pairs (20
    runs, at most 12 width pairs: each layout sees every width pair)"""
    _attn_sweep(C, k, 523, PAIRS.index((C, k)))


@pytest.mark.parametrize("C,k", SMALL_NQ)
@pytest.mark.parametrize("Nq", [1, 2, 3, 4, 5])
def test_attentive_pool_block_tail(hip, C, k, Nq):
    """fewer queries than the four waves of a block: the idle waves leave early, the others write everything"""
    _attn_sweep(C, k, Nq, Nq)


@pytest.mark.parametrize("C,ldf", [(3, 20), (5, 40), (20, 256)])
@pytest.mark.parametrize("missing", ["null", "tail"])
def test_attentive_pool_bwd_clears_wide_padding(hip, C, ldf, missing):
    """ldf beyond four times the lanes per edge (C <= 32): the header's "df ... all columns (padding zeroed) are
    overwritten" holds there too.  (Before the tail launch of tp3d_attn_pool_bwd_f32 the columns from 4 * P on kept
    the NaN they are pre-filled with here.)"""
    assert ldf > 4 * _lanes(C)
    _attn_run(C, 7, 37, C + 2, ldf, "randn", missing, C)


def test_attentive_pool_wrapper_wide_scores(hip):
    """through the autograd wrapper with g wider than C: the gradient of the extra columns is exactly 0"""
    from torch_points3d_amd.randla import attentive_pool
    gen = torch.Generator().manual_seed(4)
    Nq, k, C = 37, 5, 9
    g = torch.randn(Nq * k, C + 5, generator=gen).to(DEV).requires_grad_(True)
    f = torch.randn(Nq * k, 40, generator=gen).to(DEV).requires_grad_(True)
    nbr = _table("tail", Nq, k, gen).to(DEV)
    cot = torch.randn(Nq, C, generator=gen).to(DEV)
    out = attentive_pool(g, f, nbr, C)
    (out * cot).sum().backward()
    keep = (nbr.reshape(-1, 1) >= 0).float()
    o64, dg64, df64 = _attn_formula(g.detach()[:, :C].double(), f.detach()[:, :C].double(), keep, cot, Nq, k, C)
    o32, dg32, df32 = _attn_formula(g.detach()[:, :C].contiguous(), f.detach()[:, :C].contiguous(), keep, cot, Nq, k, C)
    _close64("attn", "wrapper out", out, o32, o64)
    _close64("attn", "wrapper dg", g.grad[:, :C], dg32, dg64)
    _close64("attn", "wrapper df", f.grad[:, :C], df32, df64)
    assert torch.count_nonzero(g.grad[:, C:]) == 0 and torch.count_nonzero(f.grad[:, C:]) == 0
    assert not bool(torch.isnan(g.grad).any()) and not bool(torch.isnan(f.grad).any())


@pytest.mark.parametrize("C,ldg,ldf", [(257, 260, 260), (8, 8, 257), (8, 7, 8)])
def test_attentive_pool_argument_checks(hip, C, ldg, ldf):
    from torch_points3d_amd import _lib
    buf = torch.zeros(4 * 300, device=DEV)
    nbr = torch.zeros(4, dtype=torch.long, device=DEV)
    st = _lib.stream_ptr(buf.device)
    with pytest.raises(_lib.Tp3dError):
        _lib.call("tp3d_attn_pool_fwd_f32", _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(nbr), 2, 2, C, ldg, ldf, _lib.ptr(buf), st)
    with pytest.raises(_lib.Tp3dError):
        _lib.call("tp3d_attn_pool_bwd_f32", _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(nbr), 2, 2, C, ldg, ldf,
                  _lib.ptr(buf), _lib.ptr(buf), st)


# ---------------------------------------------------------------------------------------------------------------------
# 2. relative-position rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("special", [-1, "M", "M+5"])
@pytest.mark.parametrize("Nq,k", [(1, 1), (16, 16), (257, 1), (3, 86)])  # (16, 16): exactly one block
def test_relpos_rows_written_and_exact(hip, Nq, k, special, offset):
    from torch_points3d_amd import _lib
    M = 37
    gen = torch.Generator().manual_seed(Nq * 100 + k)
    pos_s = torch.rand(M, 3, generator=gen) * 4 - 2 + offset
    pos_q = torch.rand(Nq, 3, generator=gen) * 4 - 2 + offset
    nbr = torch.randint(0, M, (Nq, k), generator=gen)
    flat = nbr.view(-1)
    flat[1::4] = M - 1  # the last support row is read like any other
    flat[2::4] = 5
    pos_q[(torch.arange(Nq * k)[2::4] // k).unique()[:1]] = pos_s[5]  # a coincident query / support pair
    flat[::4] = {-1: -1, "M": M, "M+5": M + 5}[special]  # no neighbour: zero row
    if special == "M" and Nq * k == 1:
        flat[0] = M - 1  # (the one-edge table also reads a real row once)
    out = torch.full((Nq * k, 12), NAN, device=DEV)
    pq, ps, nb = pos_q.to(DEV), pos_s.to(DEV), nbr.to(DEV)
    _lib.call("tp3d_randla_relpos_f32", _lib.ptr(pq), _lib.ptr(ps), _lib.ptr(nb), Nq, k, M, _lib.ptr(out),
              _lib.stream_ptr(out.device))
    rows = out.cpu()
    assert not bool(torch.isnan(rows).any())  # all 12 columns of every row are written
    ok = (flat >= 0) & (flat < M)
    pos_i, pos_j = pos_q.repeat_interleave(k, 0), pos_s[flat.clamp(0, M - 1)]
    diff = pos_i - pos_j
    assert torch.equal(rows[ok, :9], torch.cat([pos_i, pos_j, diff], 1)[ok])  # copies and one subtraction: exact
    assert torch.count_nonzero(rows[:, 10:]) == 0 and torch.count_nonzero(rows[~ok]) == 0
    # fp32 sqrt of a three-term fp32 sum of squares: a few ulp; rtol 1e-6, atol 0 (tests/test_gpu_rsconv_mp.py)
    want = diff[ok].double().norm(dim=1)
    err = (rows[ok, 9].double() - want).abs()
    if err.numel():
        rel = float((err / want.clamp(min=1e-300)).max()) if bool((want > 0).any()) else 0.0
        _report("relpos", "Nq%d k%d %s +%g |d|" % (Nq, k, special, offset), rel, 1e-6)
        assert bool((err <= 1e-6 * want).all())
    same = ok & (diff == 0).all(1)
    if Nq * k > 2:
        assert bool(same.any())
    assert torch.count_nonzero(rows[same, 6:10]) == 0  # coincident points: exactly 0


def test_relpos_wrapper_takes_any_table(hip):
    """an int32 table and a non-contiguous one go through the Python wrapper"""
    from torch_points3d_amd.randla import relative_position_rows
    gen = torch.Generator().manual_seed(8)
    M, Nq, k = 50, 33, 6
    pos_s, pos_q = torch.rand(M, 3, generator=gen).to(DEV), torch.rand(Nq, 3, generator=gen).to(DEV)
    wide = torch.randint(-1, M, (Nq, 2 * k), generator=gen).to(DEV)
    nbr = wide[:, ::2]
    assert not nbr.is_contiguous()
    base = relative_position_rows(pos_q, pos_s, nbr.contiguous())
    assert torch.equal(relative_position_rows(pos_q, pos_s, nbr), base)
    assert torch.equal(relative_position_rows(pos_q, pos_s, nbr.int()), base)
    j = nbr.reshape(-1)
    want = torch.cat([pos_q.repeat_interleave(k, 0), pos_s[j.clamp(min=0)]], 1) * (j >= 0).unsqueeze(1)
    assert torch.equal(base[:, :6], want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. skinny GEMM
# ---------------------------------------------------------------------------------------------------------------------
SK_M = [1, 255, 256, 257]
SK_N = [1, 3, 4, 6, 31, 32]


def _sk_routes(K):
    """(name, lda, offset in floats of the base pointer) of every load route that exists for this K"""
    out = [("vec", _pad4(K), 0), ("vec+8", _pad4(K) + 8, 0), ("shifted", _pad4(K), 1), ("shifted+8", _pad4(K) + 8, 1)]
    if K % 4:
        out.append(("scalar lda=K", K, 0))  # (K = 4 KV - 2: lda even but no multiple of 4)
    return out


def _sk_rows(A, lda, off):
    """A (M, K) laid out with row stride lda behind `off` floats; columns [K, pad4(K)) -- read by the float4 route,
    where they meet a zero weight -- hold 1e30, everything else outside the rows NaN (never read)"""
    M, K = A.shape
    buf = torch.full((M * lda + 8,), NAN)
    rows = buf[off:off + M * lda].view(M, lda)
    rows[:, :K] = A
    rows[:, K:_pad4(K)] = 1e30
    return buf.to(DEV)


def _sk_call(buf, off, W, M, N, K, lda, epi=None):
    from torch_points3d_amd import _lib
    Y = torch.full((M, N), NAN, device=DEV)
    a = buf.data_ptr() + 4 * off
    st = _lib.stream_ptr(Y.device)
    if epi is None:
        _lib.call("tp3d_gemm_skinny_f32", a, _lib.ptr(W), M, N, K, lda, _lib.ptr(Y), st)
    else:
        mean, scale, beta, slope = epi
        _lib.call("tp3d_gemm_skinny_bnact_f32", a, _lib.ptr(W), M, N, K, lda, _lib.ptr(mean), _lib.ptr(scale),
                  _lib.ptr(beta), slope, _lib.ptr(Y), st)
    return Y


@pytest.mark.parametrize("KV", range(1, 9))
def test_gemm_skinny_routes(hip, KV):
    """every register width KV = ceil(K / 4) at K = 4 KV - 3, 4 KV - 2, 4 KV - 1 and 4 KV, every load route, both store
    routes (N a multiple of 4 or not), M around one block.  vs float64 at rtol 1e-5 / atol 1e-5 (fp32 FMA chains of at
    most 32 terms); small-integer data must be exact."""
    gen = torch.Generator().manual_seed(KV)
    worst = 0.0
    for K in (4 * KV - 3, 4 * KV - 2, 4 * KV - 1, 4 * KV):
        A = torch.randn(257, K, generator=gen)
        Ai = torch.randint(-4, 5, (257, K), generator=gen).float()
        laid = [(name, lda, off, _sk_rows(A, lda, off), _sk_rows(Ai, lda, off)) for name, lda, off in _sk_routes(K)]
        for N in SK_N:
            W = torch.randn(N, K, generator=gen).to(DEV)
            Wi = torch.randint(-4, 5, (N, K), generator=gen).float().to(DEV)
            ref = A.to(DEV).double() @ W.double().t()
            refi = (Ai.to(DEV).double() @ Wi.double().t()).float()
            for name, lda, off, buf, bufi in laid:
                for M in SK_M:
                    got = _sk_call(buf, off, W, M, N, K, lda)
                    err = (got.double() - ref[:M]).abs()
                    bar = 1e-5 + 1e-5 * ref[:M].abs()
                    ratio = float((err / bar).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, ("K%d N%d M%d %s" % (K, N, M, name), ratio)
                    assert torch.equal(_sk_call(bufi, off, Wi, M, N, K, lda), refi[:M]), (K, N, M, name)
    _report("skinny", "KV%d worst of all K, N, M, routes (err / (1e-5 + 1e-5 |ref|))" % KV, worst, 1.0)


@pytest.mark.parametrize("KV", range(1, 9))
def test_gemm_skinny_bnact_routes(hip, KV):
    """the BatchNorm + LeakyReLU epilogue: out = leaky((y - mean) * scale + beta) in float64, negative scales, outputs on
    both sides of 0, slopes 0 / 0.2 / 1; rtol 1e-5, atol 1e-5 * max(1, |ref|max)"""
    gen = torch.Generator().manual_seed(100 + KV)
    worst = 0.0
    M = 257
    for K in (4 * KV - 3, 4 * KV):
        A = torch.randn(M, K, generator=gen)
        for N in (3, 32):
            W = torch.randn(N, K, generator=gen).to(DEV)
            mean, beta = torch.randn(N, generator=gen).to(DEV), torch.randn(N, generator=gen).to(DEV)
            sign = torch.tensor([-1.0, 1.0]).repeat(N)[:N]  # negative scales (a negative BatchNorm weight) among them
            scale = ((torch.rand(N, generator=gen) + 0.5) * sign).to(DEV)
            z = (A.to(DEV).double() @ W.double().t() - mean.double()) * scale.double() + beta.double()
            assert bool((z > 0).any()) and bool((z < 0).any())
            for slope in (0.0, 0.2, 1.0):
                ref = torch.where(z > 0, z, z * slope)
                bar = 1e-5 * max(1.0, float(ref.abs().max())) + 1e-5 * ref.abs()
                for name, lda, off in _sk_routes(K):
                    got = _sk_call(_sk_rows(A, lda, off), off, W, M, N, K, lda, (mean, scale, beta, slope))
                    ratio = float(((got.double() - ref).abs() / bar).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, ("K%d N%d slope %g %s" % (K, N, slope, name), ratio)
    _report("skinny-bnact", "KV%d worst of all K, N, slopes, routes" % KV, worst, 1.0)


def test_gemm_skinny_second_grid_trip(hip):
    """more rows than 256 * 8192 lanes: the grid-stride loop makes a second trip (K = N = 4, 34 MB per matrix)"""
    M = 256 * 8192 + 257
    gen = torch.Generator().manual_seed(5)
    A = torch.randn(M, 4, generator=gen).to(DEV)
    W = torch.randn(4, 4, generator=gen).to(DEV)
    got = _sk_call(A, 0, W, M, 4, 4, 4)
    ref = A.double() @ W.double().t()
    ratio = float(((got.double() - ref).abs() / (1e-5 + 1e-5 * ref.abs())).max())
    _report("skinny", "M %d" % M, ratio, 1.0)
    assert ratio <= 1.0
    Ai = torch.randint(-4, 5, (M, 4), generator=gen).float().to(DEV)
    Wi = torch.randint(-4, 5, (4, 4), generator=gen).float().to(DEV)
    assert torch.equal(_sk_call(Ai, 0, Wi, M, 4, 4, 4), (Ai.double() @ Wi.double().t()).float())


@pytest.mark.parametrize("N,K", [(4, 33), (33, 4)])
def test_gemm_skinny_argument_checks(hip, N, K):
    from torch_points3d_amd import _lib
    buf = torch.zeros(4096, device=DEV)
    with pytest.raises(_lib.Tp3dError):
        _sk_call(buf, 0, buf, 8, N, K, K)
    with pytest.raises(_lib.Tp3dError):
        _sk_call(buf, 0, buf, 8, N, K, K, (buf, buf, buf, 0.2))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the k = 1 gather-concat that builds fij_hat
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cx", [3, 8, 61])
@pytest.mark.parametrize("widen", ["C", "pad4", "pad4+4"])
def test_gather_concat_k1(hip, Cx, widen):
    from torch_points3d_amd.partial_dense import _KnnInterpolate
    gen = torch.Generator().manual_seed(Cx)
    M, Nq, k, Cr = 50, 300, 16, 5
    C = Cx + Cr
    ld = {"C": C, "pad4": _pad4(C), "pad4+4": _pad4(C) + 4}[widen]
    nbr = torch.randint(0, M, (Nq, k), generator=gen)
    nbr[:, 2:13] = 7  # one support row referenced by >= 3300 edges
    E = Nq * k
    xs = torch.randn(M, Cx, generator=gen).to(DEV).requires_grad_(True)
    rij = torch.randn(E, Cr, generator=gen).to(DEV).requires_grad_(True)
    cot = torch.randn(E, ld, generator=gen).to(DEV)
    edges = nbr.to(DEV).reshape(-1, 1)
    ones = torch.ones((E, 1), device=DEV)
    out = _KnnInterpolate.apply(xs, rij, edges, ones, ld)
    want = torch.cat([xs.detach()[edges.view(-1)], rij.detach(), torch.zeros(E, ld - C, device=DEV)], 1)
    assert torch.equal(out, want)  # the weight is exactly 1
    dx, dskip = torch.autograd.grad(out, (xs, rij), cot)
    assert torch.equal(dskip, cot[:, Cx:C])
    ref = torch.zeros(M, Cx, dtype=torch.float64, device=DEV).index_add_(0, edges.view(-1), cot[:, :Cx].double())
    # fp32 sums of up to 3300 terms against their float64 sum
    err, bar = (dx.double() - ref).abs(), 1e-5 * float(ref.abs().max()) + 1e-5 * ref.abs()
    ratio = float((err / bar).max())
    _report("gather", "Cx%d ld%d dx: |hip - ref64|max %.3g, |ref|max %.3g (err / bar)"
            % (Cx, ld, float(err.max()), float(ref.abs().max())), ratio, 1.0)
    assert ratio <= 1.0
    dx2, _ = torch.autograd.grad(_KnnInterpolate.apply(xs, rij, edges, ones, ld), (xs, rij), cot)
    assert torch.equal(dx, dx2)  # atomic-free: the same bits every run


# ---------------------------------------------------------------------------------------------------------------------
# 5. RandlaKernel: a batch with clouds smaller than k, and the full table unchanged
# ---------------------------------------------------------------------------------------------------------------------
FEAT = 8


def _kernel(with_x, seed):
    from torch_points3d_amd.randla import RandlaKernel
    torch.manual_seed(seed)
    cin = FEAT if with_x else 3
    ker = RandlaKernel(point_pos_nn=[10, 8, FEAT], attention_nn=[cin + FEAT, 8, cin + FEAT], global_nn=[cin + FEAT, 8, 16])
    with torch.no_grad():  # running statistics and affine that are not the initial 0 / 1
        for m in ker.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_()
                m.running_var.uniform_(0.5, 2.0)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_()
    return ker


def _restated(ker, with_x, dtype):
    from randla_ref import RandlaEdgeList
    cin = FEAT if with_x else 3
    ref = RandlaEdgeList([10, 8, FEAT], [cin + FEAT, 8, cin + FEAT], [cin + FEAT, 8, 16])
    ref.load_state_dict(ker.state_dict(), strict=True)
    return ref.to(dtype)


def _ragged_case():
    """three clouds of 5, 400 and 1 points, k = 16: queries from every cloud, so rows with 5 and 1 real slots"""
    gen = torch.Generator().manual_seed(21)
    sizes = [5, 400, 1]
    pos = torch.rand(sum(sizes), 3, generator=gen)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    qsel = torch.cat([torch.arange(5), 5 + torch.randperm(400, generator=gen)[:100].sort()[0], torch.tensor([405])])
    x = torch.randn(sum(sizes), FEAT, generator=gen)
    cot = torch.randn(qsel.numel(), 16, generator=gen)
    return pos, batch, qsel, x, cot


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("with_x", [True, False])
def test_randla_kernel_ragged_batch(hip, with_x, fused):
    """-1 slots are edges that do not exist: output, running statistics and gradients are those of the reference's
    message passing over the kNN edge list (tests/randla_ref.py), in float64; every bar comes from that restatement's own
    fp32-vs-float64 distance"""
    from randla_golden_util import bound
    from randla_ref import edge_list
    pos, batch, qsel, x, cot = _ragged_case()
    k = 16
    nbr = hip.knn(k, pos.to(DEV), pos[qsel].to(DEV), batch.to(DEV), batch[qsel].to(DEV))[0]
    assert bool((nbr < 0).any()) and bool((nbr[:5, 5:] < 0).all()) and bool((nbr[-1, 1:] < 0).all())
    ei = edge_list(nbr.cpu())
    assert ei.shape[1] == 5 * 5 + 100 * k + 1
    ker = _kernel(with_x, 11)
    tag = "%s %s" % ("x" if with_x else "pos", "fused" if fused else "unfused")

    # eval mode first (changes no state): running statistics
    refs = {dt: _restated(ker, with_x, dt) for dt in (torch.float32, torch.float64)}
    hipk = copy.deepcopy(ker).to(DEV)
    hipk.fused = fused
    outs = {}
    for dt, ref in refs.items():
        ref.eval()
        with torch.no_grad():
            outs[dt] = ref(x.to(dt) if with_x else None, pos[qsel].to(dt), pos.to(dt), ei)
    hipk.eval()
    with torch.no_grad():
        got = hipk(x.to(DEV) if with_x else None, (pos[qsel].to(DEV), pos.to(DEV)), nbr).cpu()
    assert bool(torch.isfinite(got).all()), tag
    e64 = outs[torch.float64]
    err = float((got.double() - e64).abs().max())
    bar = 1e-5 * max(1.0, float(e64.abs().max()))
    ratio = float(((got.double() - e64).abs() / (bar + 1e-5 * e64.abs())).max())
    print("[rows:ragged] %s eval: |hip - ref64|max %.3g, |ref32 - ref64|max %.3g, bar %.3g, ratio %.3g"
          % (tag, err, float((outs[torch.float32].double() - e64).abs().max()), bar, ratio))
    assert ratio <= 1.0, tag

    # train mode: batch statistics over the real edges only
    res = {}
    for dt, ref in refs.items():
        ref.train()
        xr = x.to(dt).clone().requires_grad_(True) if with_x else None
        o = ref(xr, pos[qsel].to(dt), pos.to(dt), ei)
        (o * cot.to(dt)).sum().backward()
        res[dt] = (o.detach(), None if xr is None else xr.grad, {n: p.grad for n, p in ref.named_parameters()},
                   ref.state_dict())
    hipk.train()
    xg = x.to(DEV).clone().requires_grad_(True) if with_x else None
    out = hipk(xg, (pos[qsel].to(DEV), pos.to(DEV)), nbr)
    (out * cot.to(DEV)).sum().backward()
    assert bool(torch.isfinite(out).all()), tag
    o32, gx32, gp32, _ = res[torch.float32]
    o64, gx64, gp64, sd64 = res[torch.float64]
    atol = bound(o32, o64)
    err = (out.detach().cpu().double() - o64).abs()
    ratio = float((err / (atol + 1e-5 * o64.abs())).max())
    print("[rows:ragged] %s train out: |hip - ref64|max %.3g, atol (max(1e-5, 2 |ref32 - ref64|max)) %.3g, ratio %.3g"
          % (tag, float(err.max()), atol, ratio))
    assert ratio <= 1.0, tag
    worst = 0.0
    for name, v in hipk.state_dict().items():
        if name.endswith("num_batches_tracked"):
            assert int(v) == int(sd64[name]), name
            continue
        if "running_" in name:
            e = (v.cpu().double() - sd64[name]).abs()
            r = float((e / (1e-5 + 1e-4 * sd64[name].abs())).max())
            worst = max(worst, r)
            assert r <= 1.0, (tag, name, r)
    _report("ragged", tag + " running statistics (err / (1e-5 + 1e-4 |ref|))", worst, 1.0)

    def grad_check(name, g, g32, g64):
        grel = _rel_l2(g32, g64)
        rel, bar = _rel_l2(g.cpu(), g64), max(1e-4, 4.0 * grel)
        _report("ragged", "%s grad %s (relative L2; restatement's own %.3g)" % (tag, name, grel), rel, bar)
        assert rel <= bar, (tag, name, rel, bar)

    if with_x:
        assert bool(torch.isfinite(xg.grad).all())
        grad_check("x", xg.grad, gx32, gx64)
    for name, p in hipk.named_parameters():
        if gp64[name] is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert bool(torch.isfinite(p.grad).all()), name
        if name.endswith(".0.bias"):
            # a Linear bias in front of a train-mode BatchNorm: zero gradient analytically, round-off on every side (the
            # treatment of tests/test_randla_golden_cpu.py): small against the gradient of the weight next to it
            wn = float(gp64[name[:-4] + "weight"].norm())
            assert float(p.grad.norm()) < 1e-4 * wn + 1e-6, name
            continue
        grad_check(name, p.grad, gp32[name], gp64[name])


@pytest.mark.parametrize("with_x", [True, False])
def test_randla_kernel_full_table_keeps_its_bits(hip, with_x):
    """a table without -1 slots runs the launches it always did: the module's output is torch.equal to the same inputs
    sent through the fused kernels directly (as tests/test_gpu_kpconv_deform.py::test_rigid_block_is_the_rigid_kernel),
    and the unfused module to the plain torch chain"""
    import torch.nn.functional as F
    from torch_points3d_amd import fused as fz
    from torch_points3d_amd.partial_dense import _KnnInterpolate
    from torch_points3d_amd.randla import attentive_pool, relative_position_rows
    gen = torch.Generator().manual_seed(31)
    M, Nq, k = 700, 200, 16
    pos_s = torch.rand(M, 3, generator=gen).to(DEV)
    pos_q = pos_s[torch.randperm(M, generator=gen)[:Nq].to(DEV)]
    x = torch.randn(M, FEAT, generator=gen).to(DEV) if with_x else None
    nbr = hip.knn(k, pos_s, pos_q)[0]
    assert not bool((nbr < 0).any())
    ker = _kernel(with_x, 12).to(DEV).train()
    twin, plain, chain = copy.deepcopy(ker), copy.deepcopy(ker), copy.deepcopy(ker)
    out = ker(x, (pos_q, pos_s), nbr)
    rij = fz.rows_mlp(twin.point_pos_nn, relative_position_rows(pos_q, pos_s, nbr))
    xs = pos_s if x is None else x
    C = xs.shape[1] + rij.shape[1]
    edges = nbr.reshape(-1, 1)
    ones = torch.ones((edges.shape[0], 1), dtype=torch.float32, device=DEV)
    fij_hat = _KnnInterpolate.apply(xs, rij, edges, ones, _pad4(C))
    direct = fz.rows_mlp(twin.global_nn, attentive_pool(fz.rows_mlp(twin.attention_nn, fij_hat), fij_hat, nbr, C))
    assert torch.equal(out, direct)
    plain.fused = False
    j = nbr.reshape(-1)
    pos_i, pos_j = pos_q.repeat_interleave(k, dim=0), pos_s[j]
    vij = pos_i - pos_j
    rij = fz.rows_mlp(chain.point_pos_nn, torch.cat([pos_i, pos_j, vij, torch.norm(vij, dim=1).unsqueeze(1)], dim=1))
    fh = torch.cat([pos_j if x is None else x[j], rij], dim=1)
    msg = F.softmax(fz.rows_mlp(chain.attention_nn, fh), -1) * fh
    assert torch.equal(plain(x, (pos_q, pos_s), nbr), fz.rows_mlp(chain.global_nn, msg.reshape(Nq, k, -1).sum(dim=1)))
