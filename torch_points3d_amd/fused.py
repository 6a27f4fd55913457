"""Channel-last fused implementation of the grouped-MLP aggregation.

The reference materialises (B, C, npoint, nsample) tensors and runs Conv2d 1x1 -> BatchNorm2d -> LeakyReLU ->
max_pool2d on them (modules/pointnet2/dense.py:36-75, core/common_modules/dense_modules.py:5-29).  Here the same
arithmetic runs on (rows, C) row-major activations: hand-written HIP kernels (csrc/rows.hip) do the gather /
centre / concat, the BatchNorm statistics, the folded affine + LeakyReLU (+ max over nsample) and every
backward pass; only the dense contractions are issued as plain library GEMMs (torch.mm -> rocBLAS/hipBLASLt).
Parameters and buffers are read from the very same nn.Conv2d / nn.BatchNorm2d modules the reference layout
defines, so state_dict keys and checkpoints are unchanged.
"""
import collections

import torch
import torch.nn as nn

from . import _lib


USE_ROWS_GEMM = True  # False: forward / input-gradient contractions through torch.mm (library GEMM)


def _cl(x):
    """(B, C, N) tensor -> its (B, N, C) contiguous channel-last form (free when x is a transposed view)."""
    return x.transpose(1, 2).contiguous()


def _pad4(c):
    return (c + 3) & ~3


def _slope_of(act):
    if act is None:
        return 1.0
    if isinstance(act, nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, nn.ReLU):
        return 0.0
    return None


def layer_parts(block):
    """(conv, bn, slope) of a Conv2D/Conv1D Seq block if the fused kernels can run it, else None."""
    mods = list(block.children())
    if not mods or not isinstance(mods[0], (nn.Conv2d, nn.Conv1d)):
        return None
    conv = mods[0]
    if conv.bias is not None or any(k != 1 for k in conv.kernel_size):
        return None
    bn, act = None, None
    for m in mods[1:]:
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)) and bn is None and act is None:
            bn = m
        elif act is None:
            act = m
        else:
            return None
    if bn is None or not bn.affine or not bn.track_running_stats or bn.momentum is None:
        return None
    slope = _slope_of(act)
    if slope is None:
        return None
    return conv, bn, slope


def mlp_parts(mlp):
    parts = [layer_parts(b) for b in mlp.children()]
    return None if (not parts or any(p is None for p in parts)) else parts


FWD_X3 = True  # forward contractions of the hidden layers (more than 64 output columns) on the bf16 matrix pipe as well
               # (csrc/gemm_rows_x3.hip: exact three-term split, six term pairs, fp32 accumulation)
WGRAD_X3_ACT = True  # ... and its loader waves form the activated A operand from the previous layer's pre-BatchNorm output,
                     # so that the forward kernels write no activated side output for those layers (one (M, K) store less)
WGRAD_X3 = 6  # weight-gradient contractions of the large layers on the bf16 matrix pipe, every fp32 value split exactly into
              # three bf16 terms (csrc/gemm_tn_x3.hip): 6 = the six term pairs of weight >= 2^-15 (what is dropped is below
              # 2^-21 of a product), 9 = all nine (every product exact), 0 = the fp32 MFMA kernel for every shape.
              # The split truncates, so the dropped pairs have the sign of a * b: on one-signed operands (abs(randn), post-
              # LeakyReLU rows against a dY with a common offset) the six-term result sits 4.1-4.4e-8 of |dY|^T |A| below
              # float64 on average (nine terms and fp32 MFMA: <= 7e-9), while the largest element error stays within
              # 0.9-1.25x the fp32 MFMA kernel's (2.5-2.8e-7 of |dY|^T |A|) -- test_x3_weight_gradient_on_one_signed_operands.
              # Measured against float64 on the layers of the BASELINE step: 2.1-3.3e-7 of the scale with 6 or 9 terms
              # (hi * hi products in an accumulator of their own), 4.2-5.4e-7 for the fp32 MFMA kernel; 524288 x 128 x 128:
              # 133 us (6), 141 us (9), 185 us (fp32 MFMA) -- the matrix pipe's load lowers the shader clock (2.2 -> 1.8 GHz
              # in the counters), so the nine-term form costs more than its extra MFMAs


_ident = {}


def _identity_stats(K, dev):
    """(zeros, ones) rows of K floats: the statistics under which a BatchNorm + LeakyReLU(1) prologue is the identity"""
    key = (dev.index, K)
    hit = _ident.get(key)
    if hit is None:
        hit = _ident[key] = (torch.zeros(K, dtype=torch.float32, device=dev), torch.ones(K, dtype=torch.float32, device=dev))
    return hit


def _chain_wgrad(b, dY, l, A0, acts, Ys, stats, slopes, dA_prev=None, training=True):
    """(dW, red): the weight gradient of layer l of a fused chain, dY^T @ (activated input of the layer), on the kernel its
    plan b names.  "x3_act_red" (l >= 1) also gives red (4, C_{l-1}) = dbeta, dgamma, c1, c2, the BatchNorm-backward
    reductions of layer l - 1 from dA_prev, the gradient of its activated output: both need Y_{l-1}, which streams through
    the contraction's loader waves once (tp3d_gemm_tn_x3_act_red_f32).  Else red is None."""
    if b.wgrad not in ("x3_act", "x3_act_red"):
        return _gemm_tn_launch(b.wgrad, dY, A0 if l == 0 else acts[l - 1], b.terms, None, b.wgrad_rev), None
    ps = stats[l - 1]  # the forward pass kept no activated rows: the contraction's loader waves form them from Y_{l-1}
    if b.wgrad == "x3_act":
        return _gemm_tn_launch("x3_act", dY, Ys[l - 1], b.terms, (ps[0], ps[2], ps[3], slopes[l - 1]), b.wgrad_rev), None
    dev = dY.device
    M, N = dY.shape
    K = Ys[l - 1].shape[1]
    out = torch.empty((N, K), dtype=torch.float32, device=dev)
    red = torch.empty((4, K), dtype=torch.float32, device=dev)
    ws = _lib.gemm_tn_workspace(M, N, K, dev, x3=True)
    rws = _lib.workspace("gemm_tn_red", 4 * 2 * b.wgrad_chunks * K, dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_gemm_tn_x3_act_red_f32", _lib.ptr(dY), _lib.ptr(Ys[l - 1]), _lib.ptr(ps[0]), _lib.ptr(ps[2]), _lib.ptr(ps[3]),
                  _lib.ptr(ps[1]), float(slopes[l - 1]), _lib.ptr(dA_prev), int(training), M, N, K, 6, _lib.ptr(out), _lib.ptr(ws),
                  _lib.ptr(red), _lib.ptr(rws), int(b.wgrad_rev), _lib.stream_ptr(dev))
    return out, red


def _chain_wgrad_narrow(dY_src, Y, ls, red, slope, A0, reverse, st):
    """weight gradient of a first layer of grouped rows straight from (Y, dA, A0): dY is never written"""
    dev = Y.device
    M, C = Y.shape
    Kp = A0.shape[1]
    dW = torch.empty((C, Kp), dtype=torch.float32, device=dev)
    nws = _lib.workspace("gemm_tn_narrow", 4 * _lib.load().tp3d_gemm_tn_bn_narrow_workspace_floats(M, C, Kp), dev)
    _lib.call("tp3d_gemm_tn_bn_narrow_f32", _lib.ptr(Y), _lib.ptr(dY_src), _lib.ptr(ls[0]), _lib.ptr(ls[2]),
              _lib.ptr(ls[3]), _lib.ptr(red[2]), _lib.ptr(red[3]), slope, _lib.ptr(A0), M, C, Kp, _lib.ptr(dW),
              _lib.ptr(nws), reverse, st)
    return dW


def gemm_tn(dY, A, x3=None, act=None, reverse=0):
    """dY (M,N), A (M,K) -> dY^T @ A (N,K), split over the rows, partial tiles summed in fixed order (reproducible):
    csrc/gemm_tn_x3.hip for the shapes it serves (x3 terms, default WGRAD_X3), else the fp32 MFMA kernel csrc/gemm_tn.hip.
    reverse: the bf16-pipe kernel walks the row blocks last to first (include/tp3d_hip.h, `reverse`)."""
    dY, A = dY.contiguous(), A.contiguous()
    M, N = dY.shape
    K = A.shape[1]
    terms = WGRAD_X3 if x3 is None else x3
    kernel = "x3" if terms and M > 0 and _lib.load().tp3d_gemm_tn_x3_serves(M, N, K) else "tn"
    if act is not None:
        # A = LeakyReLU((Yp - mean) * scale + beta) formed by the contraction's loader waves (act = mean, scale, beta, slope)
        if kernel != "x3":
            raise ValueError("gemm_tn(act=): only the bf16-pipe contraction forms its A operand (shape %s x %s x %s)" % (M, N, K))
        kernel = "x3_act"
    return _gemm_tn_launch(kernel, dY, A, terms, act, reverse)


def _gemm_tn_launch(kernel, dY, A, terms, act, reverse):
    """one weight-gradient contraction on the kernel named ("tn", "x3", "x3_act"); contiguous operands"""
    dev = dY.device
    M, N = dY.shape
    K = A.shape[1]
    out = torch.empty((N, K), dtype=torch.float32, device=dev)
    ws = _lib.gemm_tn_workspace(M, N, K, dev, x3=kernel != "tn")
    with _lib.on_device(dev):
        if kernel == "x3_act":
            _lib.call("tp3d_gemm_tn_x3_act_f32", _lib.ptr(dY), _lib.ptr(A), _lib.ptr(act[0]), _lib.ptr(act[1]), _lib.ptr(act[2]),
                      float(act[3]), M, N, K, int(terms), _lib.ptr(out), _lib.ptr(ws), int(reverse), _lib.stream_ptr(dev))
        elif kernel == "x3":
            _lib.call("tp3d_gemm_tn_x3_f32", _lib.ptr(dY), _lib.ptr(A), M, N, K, int(terms), _lib.ptr(out), _lib.ptr(ws), int(reverse),
                      _lib.stream_ptr(dev))
        else:
            sync_few_row_tiles()
            _lib.call("tp3d_gemm_tn_f32", _lib.ptr(dY), _lib.ptr(A), M, N, K, _lib.ptr(out), _lib.ptr(ws),
                      _lib.stream_ptr(dev))
    return out


SKINNY_MAX = 32       # tp3d_gemm_skinny_f32: both channel counts at most this
SKINNY_MIN_ROWS = 32768


def gemm_skinny(A, W):
    """A (M,K) @ W (N,K)^T -> (M,N) for K, N <= 32 and many rows: one row per lane (csrc/gemm_skinny.hip)."""
    dev = A.device
    A, W = A.contiguous(), W.contiguous()
    M, K = A.shape
    N = W.shape[0]
    Y = torch.empty((M, N), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_gemm_skinny_f32", _lib.ptr(A), _lib.ptr(W), M, N, K, K, _lib.ptr(Y), _lib.stream_ptr(dev))
    return Y


def _is_skinny(M, a, b):
    return M >= SKINNY_MIN_ROWS and a <= SKINNY_MAX and b <= SKINNY_MAX


def gemm_rows(A, Bt, want_stats=False):
    """A (M,K) @ Bt (N,K)^T -> (M,N) with the fp32 MFMA rows kernel (csrc/gemm_rows.hip); optionally also the shifted
    partial column sums for BatchNorm (then returned as `part`).  K must be a multiple of 4.  Without statistics a
    long contraction with few output tiles is split over K-ranges (two-level summation, more workgroups)."""
    dev = A.device
    M, K = A.shape
    N = Bt.shape[0]
    Bm = Bt.contiguous()
    C = torch.empty((M, N), dtype=torch.float32, device=dev)
    part, slabs = None, None
    h = _lib.load()
    sync_few_row_tiles()
    if want_stats:
        part = _lib.workspace("gemm_rows_stats", 4 * h.tp3d_gemm_rows_stat_floats(M, N), dev)
    else:
        n = h.tp3d_gemm_rows_workspace_floats(M, N, K)
        if n:
            slabs = _lib.workspace("gemm_rows_slabs", 4 * n, dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_gemm_rows_f32", _lib.ptr(A), _lib.ptr(Bm), M, N, K, _lib.ptr(C), _lib.ptr(part), _lib.ptr(slabs),
                  _lib.stream_ptr(dev))
    return C, part


def _finalize_stats(part, M, C, gamma, beta, bn, dev, st, chunks=None):
    """(4, C) = mean, invstd, scale, beta from the shifted partial sums a rows GEMM left in `part` (training mode)."""
    stats = torch.empty((4, C), dtype=torch.float32, device=dev)
    if chunks is None:
        chunks = _lib.load().tp3d_gemm_rows_stat_chunks(M, C)
    _lib.call("tp3d_bn_finalize_f32", _lib.ptr(part), chunks, M, C, float(bn.eps),
              float(bn.momentum), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var),
              _lib.ptr(bn.num_batches_tracked), _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), st)
    _note_training_pass(bn)
    return stats


def _note_training_pass(bn):
    """The kernels update running_mean / running_var / num_batches_tracked in place without touching the tensors'
    version counters: eval-mode statistics cached on the module (_bn_stats) are keyed on this count as well."""
    bn._tp3d_train_passes = getattr(bn, "_tp3d_train_passes", 0) + 1


_replay_epoch = 0


def note_graph_replay():
    """A captured training step was replayed: parameters and running statistics of every module may have changed
    without any Python running (no version counter moves, _note_training_pass does not fire, and with flattened
    parameters the optimizer only touches the flat tensor).  dp.ShardedStep / PipelinedStep call this on every replay;
    the count is part of the eval-statistics cache key, so a validation pass after replayed training recomputes them."""
    global _replay_epoch
    _replay_epoch += 1


def eval_state_key(tensors, bns):
    """What anything folded from eval-mode parameters and running statistics is cached under: address and version
    counter of every tensor, and -- because the BatchNorm kernels and a replayed captured step write the statistics
    without moving a version counter -- the training passes of every BatchNorm in `bns` and the replay count."""
    return (tuple((t.data_ptr(), t._version) for t in tensors)
            + tuple(getattr(bn, "_tp3d_train_passes", 0) for bn in bns) + (_replay_epoch,))


FEW_ROW_TILES = 1  # 1: few-row launches (4096 / 16384 rows) of the plain rows GEMM and the fp32 weight-gradient GEMM run on
                   # quarter- / half-size workgroup tiles so that they fill the CUs (csrc/gemm_plans.h); 0: the 128 x 128
                   # plans.  Bit-identical results.  A process-wide setting of the library: with a captured step, fix it
                   # before warm-up
_few_row_pushed = None


def sync_few_row_tiles():
    """hand FEW_ROW_TILES to the library when it has changed (tp3d_set_few_row_tiles) -- in front of every launch and plan
    query it bears on, so that `bench.py --set FEW_ROW_TILES=0` and the tests switch routes within one process"""
    global _few_row_pushed
    v = int(FEW_ROW_TILES)
    if v != _few_row_pushed:
        _lib.load().tp3d_set_few_row_tiles(v)
        _few_row_pushed = v


ROWS_GEMM_MIN_COLS = 32   # narrower outputs (class scores, edge MLPs) stay on the library / skinny kernels
ROWS_GEMM_WITHOUT_STATS = True  # the rows kernel also where it has no BatchNorm statistics to fold in.  False: library GEMM
                                # there -- the choice for inference replayed from a HIP graph (KPConv unet_4 forward 1.46 ->
                                # 1.10 ms); launched eagerly the library's host side makes the forward slower (1.96 -> 2.24 ms).
                                # One setting for both, so that a captured step stays bit-identical to its eager twin
ROWS_GEMM_EPILOGUE = True  # eval-mode layers without a gradient request: BatchNorm + activation in the rows GEMM's epilogue
ROWS_GEMM_NARROW = True   # widths served by the 128 x 64 tiles (N % 128 in 1..64) on the rows kernel (else library GEMM)
CHAIN_MIN_ROWS = 32768    # the fused layer chain serves the large row matrices (grouped / per-point activations)


def _rows_gemm_serves(cout):
    if not USE_ROWS_GEMM or cout < ROWS_GEMM_MIN_COLS:
        return False
    return ROWS_GEMM_NARROW or not (0 < cout % 128 <= 64)


def _bn_stats(Y, M, C, gamma, beta, bn, training, dev, st, bias=None):
    """(4, C) = mean, invstd, scale = gamma * invstd, beta of BatchNorm over the rows of Y.  In eval mode they depend only on the
    module's parameters and running statistics, so they are computed once and reused until any of those changes."""
    key = None
    if not training:
        key = eval_state_key((gamma, beta, bn.running_mean, bn.running_var) + ((bias,) if bias is not None else ()), (bn,))
        hit = getattr(bn, "_tp3d_eval_stats", None)
        if hit is not None and hit[0] == key:
            return hit[1]
    stats = torch.empty((4, C), dtype=torch.float32, device=dev)
    ws = _lib.bn_workspace(M, C, dev)
    _lib.call("tp3d_bn_stats_f32", _lib.ptr(Y), M, C, float(bn.eps), float(bn.momentum), _lib.ptr(gamma), _lib.ptr(beta),
              _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked) if training else None,
              int(training), _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), _lib.ptr(ws), st)
    if training:
        _note_training_pass(bn)
    if key is not None:
        if bias is not None:
            stats[0].sub_(bias.detach())  # (Y + b - running_mean) * scale + beta == (Y - (running_mean - b)) * scale + beta
        bn._tp3d_eval_stats = (key, stats)
    return stats


def _bn_act_out(Y, stats, slope, pool_ns, st):
    """(out, arg): out = LeakyReLU(BatchNorm(Y)) under stats = mean, invstd, scale, beta; with pool_ns > 0 the max over
    groups of pool_ns consecutive rows and arg, the row each maximum came from (else arg is None)"""
    dev = Y.device
    M, C = Y.shape
    if pool_ns:
        G = M // pool_ns
        out = torch.empty((G, C), dtype=torch.float32, device=dev)
        arg = torch.empty((G, C), dtype=torch.int32, device=dev)
        _lib.call("tp3d_bn_act_maxpool_f32", _lib.ptr(Y), _lib.ptr(stats[0]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), slope, G,
                  pool_ns, C, _lib.ptr(out), _lib.ptr(arg), st)
        return out, arg
    out = torch.empty((M, C), dtype=torch.float32, device=dev)
    _lib.call("tp3d_bn_act_f32", _lib.ptr(Y), _lib.ptr(stats[0]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), slope, M, C,
              _lib.ptr(out), st)
    return out, None


def _bn_act_bwd(grad_out, arg, Y, stats, slope, pool_ns, training, st):
    """(dY, dgb): the backward pass of _bn_act_out -- the gradient of Y and dgb (2, C) = dbeta, dgamma"""
    dev = Y.device
    M, C = Y.shape
    dY = torch.empty_like(Y)
    dgb = torch.empty((2, C), dtype=torch.float32, device=dev)
    ws = _lib.bn_workspace(M, C, dev)
    _lib.call("tp3d_bn_act_bwd_f32", _lib.ptr(grad_out), _lib.ptr(arg), _lib.ptr(Y), _lib.ptr(stats[2]),
              _lib.ptr(stats[3]), _lib.ptr(stats[0]), _lib.ptr(stats[1]), slope, M, max(pool_ns, 1), C,
              int(training), _lib.ptr(dgb[0]), _lib.ptr(dgb[1]), _lib.ptr(dY), _lib.ptr(ws), st)
    return dY, dgb


def _layer_route(M, Kp, Cout, training, pool_ns, want_grad):
    """(path, statistics ride on the GEMM) of one Linear + BatchNorm + activation layer on (M, Kp) rows; path is one of
    "skinny_bnact", "rows_epi", "rows", "skinny", "library" """
    skinny = _is_skinny(M, Kp, Cout)
    if not training and skinny and not want_grad:
        # eval-mode edge MLP layer, no gradient wanted: Linear + BatchNorm (running statistics) + activation in ONE
        # pass over the rows (tp3d_gemm_skinny_bnact_f32) instead of GEMM, statistics lookup and affine pass
        return "skinny_bnact", False
    # the dense contraction on the fp32 MFMA rows kernel (128- or 64-column tiles); BatchNorm statistics come out of
    # its epilogue, except for the long contractions with few output tiles (the 4096-row global / decoder layers),
    # which run as a K-split launch followed by the separate statistics pass over their small output.
    # Few output tiles and a contraction of 512..1023 channels: the rows kernel has nothing to hide its K walk
    # behind and a K-split would move more slab bytes than it saves -- library GEMM + separate statistics pass
    # (93 -> 27 + 12 us on the 4096-row global layer); longer contractions go K-split for their summation order
    few_tiles = ((M + 127) // 128) * ((Cout + 127) // 128) < 128 and 512 <= Kp < 1024
    rows = _rows_gemm_serves(Cout) and Kp % 4 == 0 and not few_tiles
    # (few output tiles and a long contraction: served by the K-split launch, which has slabs and no fused statistics)
    want_stats = training and _lib.load().tp3d_gemm_rows_workspace_floats(M, Cout, Kp) == 0
    if rows and ROWS_GEMM_EPILOGUE and not training and not pool_ns and ROWS_GEMM_WITHOUT_STATS and not want_grad:
        # inference: BatchNorm (running statistics) + activation applied to the accumulators -- one launch per layer
        return "rows_epi", False
    # with nothing to fold into the epilogue (eval mode; K-split shapes) the library GEMM's KERNEL is faster on every
    # such shape of the KPConv / PointNet++ networks (tools/probes/small_gemm.py: 65536 x 64 x 256 24 vs 40 us,
    # 27 x 2048 x 1024 18 vs 63 us) but its host side costs more than this library's launch: KPConv unet_4 forward
    # replayed from a HIP graph 1.46 -> 1.10 ms with it, launched eagerly 1.96 -> 2.24 ms (ROWS_GEMM_WITHOUT_STATS)
    if rows and (want_stats or ROWS_GEMM_WITHOUT_STATS):
        return "rows", want_stats
    if skinny:
        return "skinny", False  # edge-wise MLPs of a few channels: a pure stream, one row per lane
    return "library", False  # plain library GEMM (a handful of output columns, e.g. the 10-class head)


class _LinearBNAct(torch.autograd.Function):
    """out = LeakyReLU(BatchNorm(A @ W^T)) on rows; with pool_ns > 0 also the max over groups of pool_ns rows."""

    @staticmethod
    def forward(ctx, A, weight, gamma, beta, bn, slope, pool_ns, grad_enabled, bias=None):
        # bias: the Linear's bias (reference MLP default, core/common_modules/base_modules.py:29-43).  The GEMM runs
        # without it: under batch statistics it cancels in the normalised output (it only shifts the running mean);
        # with running statistics it folds into the affine shift.
        # grad_enabled: grad mode at the call site (inside Function.forward it is always off, and under torch.no_grad()
        # the parameters still report requires_grad through ctx.needs_input_grad)
        dev = A.device
        A = A.contiguous()
        M, Kp = A.shape  # Kp >= Cin: producers pad rows with zero columns to a multiple of 4 floats
        Cout = weight.shape[0]
        W2 = weight.reshape(Cout, -1)
        Cin = W2.shape[1]
        if Kp != Cin:
            W2 = torch.nn.functional.pad(W2, (0, Kp - Cin))
        training = bn.training
        st = _lib.stream_ptr(dev)
        path, want_stats = _layer_route(M, Kp, Cout, training, pool_ns, grad_enabled and any(ctx.needs_input_grad))
        if path in ("skinny_bnact", "rows_epi"):  # one launch: the statistics are the running ones, nothing is kept
            with _lib.on_device(dev):
                stats = _bn_stats(A, M, Cout, gamma, beta, bn, False, dev, st, bias)
                out = torch.empty((M, Cout), dtype=torch.float32, device=dev)
                if path == "skinny_bnact":
                    _lib.call("tp3d_gemm_skinny_bnact_f32", _lib.ptr(A), _lib.ptr(W2.contiguous()), M, Cout, Kp, Kp,
                              _lib.ptr(stats[0]), _lib.ptr(stats[2]), _lib.ptr(stats[3]), slope, _lib.ptr(out), st)
                else:
                    sync_few_row_tiles()
                    n = _lib.load().tp3d_gemm_rows_workspace_floats(M, Cout, Kp)
                    slabs = _lib.workspace("gemm_rows_slabs", 4 * n, dev) if n else None
                    _lib.call("tp3d_gemm_rows_epi_f32", _lib.ptr(A), _lib.ptr(W2.contiguous()), M, Cout, Kp, _lib.ptr(stats[0]),
                              _lib.ptr(stats[2]), _lib.ptr(stats[3]), slope, _lib.ptr(out), _lib.ptr(slabs), st)
            return out.view(M // pool_ns, pool_ns, Cout).max(1)[0] if pool_ns else out  # ("rows_epi" is never pooled)
        part = None
        if path == "rows":
            Y, part = gemm_rows(A, W2, want_stats=want_stats)
        elif path == "skinny":
            Y = gemm_skinny(A, W2)
        else:
            Y = torch.mm(A, W2.t())
        with _lib.on_device(dev):
            if part is not None:
                stats = _finalize_stats(part, M, Cout, gamma, beta, bn, dev, st)  # mean, invstd, scale, beta
            else:
                stats = _bn_stats(Y, M, Cout, gamma, beta, bn, training, dev, st, bias)
            out, arg = _bn_act_out(Y, stats, slope, pool_ns, st)
        if training and bias is not None:  # (num_batches_tracked was advanced by the statistics kernel)
            bn.running_mean.add_(bias.detach(), alpha=float(bn.momentum))  # the kernels saw the mean without it
        ctx.save_for_backward(A, W2, Y, stats, arg)
        ctx.cfg = (slope, pool_ns, training, tuple(weight.shape), Cin, bias is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        A, W2, Y, stats, arg = ctx.saved_tensors
        slope, pool_ns, training, wshape, Cin, has_bias = ctx.cfg
        dev = grad_out.device
        grad_out = grad_out.contiguous()
        M, Cout = Y.shape
        need_A, need_W, need_bias = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[-1]  # (bias comes last)
        with _lib.on_device(dev):
            dY, dgb = _bn_act_bwd(grad_out, arg, Y, stats, slope, pool_ns, training, _lib.stream_ptr(dev))
        dW = None
        if need_W:
            dW = gemm_tn(dY, A)[:, :Cin].reshape(wshape)
        dA = None
        if need_A:
            if _is_skinny(M, W2.shape[1], Cout):
                dA = gemm_skinny(dY, W2.t())
            else:
                # (the library GEMM: the rows kernel was measured 0.22 ms/step slower on these input-gradient shapes, and
                #  issuing the weight gradients on a second stream 0.3 ms slower -- round 2)
                dA = torch.mm(dY, W2)
        dbias = None
        if has_bias and need_bias:
            # batch statistics remove the bias from the output (gradient exactly zero); running statistics do not
            dbias = torch.zeros(Y.shape[1], dtype=torch.float32, device=dev) if training else dY.sum(0)
        return dA, dW, dgb[1], dgb[0], None, None, None, None, dbias


class _MLPChain(torch.autograd.Function):
    """A whole shared MLP -- [1x1 conv -> BatchNorm -> LeakyReLU] x L (+ max over groups of pool_ns rows) -- on a large
    row matrix, with every BatchNorm / activation pass folded into the GEMM that consumes its result
    (core/common_modules/dense_modules.py:25-29 forward, autograd backward):

      forward   Y_0 = A_0 W_0^T;  Y_l = act(BN(Y_{l-1})) W_l^T  -- the activated tensor is formed by the GEMM's loader waves
                from Y_{l-1} (tp3d_gemm_rows_bnact_x3_f32 / _sp_f32), never written; BatchNorm statistics come out of each
                GEMM's epilogue
      backward  per layer the reductions (dbeta, dgamma -- a pass of their own, or riding on the weight-gradient kernel of
                the layer above, tp3d_gemm_tn_x3_act_red_f32), then
                dA_{l-1} = dY_l W_l                  dY_l formed by the loader waves, written once as a side output
                                                     (tp3d_gemm_rows_bnbwd_sp_f32)
                dW_l     = dY_l^T act(BN(Y_{l-1}))   the activated operand formed by the loader waves (tp3d_gemm_tn_x3_act_f32)
                with dY_l = BatchNorm+activation backward of (dA_l, Y_l)

    Only the pre-BatchNorm outputs Y_l are kept for the backward pass (plus the activated rows of the layers whose weight
    gradient the bf16-pipe kernel does not serve)."""

    @staticmethod
    def forward(ctx, A0, pool_ns, layers, grad_cols, grad_enabled, *params):
        # layers: [(bn module, slope)], params: [weight_0, gamma_0, beta_0, weight_1, ...]; grad_cols: None or (first, count) --
        # the only columns of A0 whose gradient the producer of A0 reads (grouped rows: the feature columns);
        # grad_enabled: grad mode at the call site (with it off, no side outputs for a backward that cannot come)
        dev = A0.device
        A0 = A0.contiguous()
        M, K0 = A0.shape
        st = _lib.stream_ptr(dev)
        L = len(layers)
        training = layers[0][0].training
        need = ctx.needs_input_grad
        first = len(need) - len(params)  # position of weight_0 among the arguments
        plan = _plan_chain(M, K0, [params[3 * l].shape[0] for l in range(L)], pool_ns, grad_enabled and any(need), need[0],
                           need[first::3], grad_cols)
        Ys, stats, W2s, cins, acts = [], [], [], [], [None] * (L - 1)
        with _lib.on_device(dev):
            for l, ((bn, slope), p) in enumerate(zip(layers, plan)):
                weight, gamma, beta = params[3 * l], params[3 * l + 1], params[3 * l + 2]
                Cout = weight.shape[0]
                W2 = weight.reshape(Cout, -1)
                Kp = K0 if l == 0 else Ys[-1].shape[1]
                cins.append(W2.shape[1])
                if W2.shape[1] != Kp:
                    W2 = torch.nn.functional.pad(W2, (0, Kp - W2.shape[1]))
                W2 = W2.contiguous()
                Y = torch.empty((M, Cout), dtype=torch.float32, device=dev)
                part = None
                if training:
                    nbytes = 16 * p.chunks * Cout if p.reverse is not None else 4 * _lib.load().tp3d_gemm_rows_stat_floats(M, Cout)
                    part = _lib.workspace("gemm_rows_stats", nbytes, dev)  # (the plain rows kernel sizes its own buffer)
                if p.kernel == "narrow":
                    # a handful of input channels (grouped rows: relative position + features): the streaming kernel
                    _lib.call("tp3d_gemm_rows_narrow_f32", _lib.ptr(A0), _lib.ptr(W2), M, Cout, Kp, _lib.ptr(Y), _lib.ptr(part), p.reverse, st)
                elif p.kernel in ("rows", "bn_act_rows"):
                    src = A0
                    if l:  # a width the split-role kernel does not serve: the separate pass, then the plain rows GEMM
                        src = _bn_act_out(Ys[-1], stats[-1], layers[l - 1][1], 0, st)[0]
                        acts[l - 1] = src if p.keep_act else None
                    sync_few_row_tiles()
                    _lib.call("tp3d_gemm_rows_f32", _lib.ptr(src), _lib.ptr(W2), M, Cout, Kp, _lib.ptr(Y), _lib.ptr(part), None, st)
                else:
                    if l == 0:
                        # the first layer on the bf16 pipe as well: the same kernel with the identity as its prologue
                        # ((y - 0) * 1 + 0, slope 1) -- 524288 x 128 x 132: 229 us on the fp32 rows kernel
                        ident = _identity_stats(Kp, dev)
                        src, mean, scale, shift, pslope = A0, ident[0], ident[1], ident[0], 1.0
                    else:
                        # the previous layer's BatchNorm + activation in the loader waves of the split-role kernel (or of its
                        # twin on the matrix pipe: the same contraction as bf16 term pairs); with a backward pass to come,
                        # the activated rows leave as a side output of the same kernel
                        ps = stats[-1]
                        src, mean, scale, shift, pslope = Ys[-1], ps[0], ps[2], ps[3], layers[l - 1][1]
                        acts[l - 1] = torch.empty((M, Kp), dtype=torch.float32, device=dev) if p.keep_act else None
                    _lib.call("tp3d_gemm_rows_bnact_sp_f32" if p.kernel == "sp" else "tp3d_gemm_rows_bnact_x3_f32", _lib.ptr(src),
                              _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(shift), pslope, _lib.ptr(W2), M, Cout, Kp, _lib.ptr(Y),
                              _lib.ptr(part), _lib.ptr(acts[l - 1]) if l else None, p.reverse, st)
                if training:
                    stats.append(_finalize_stats(part, M, Cout, gamma, beta, bn, dev, st, p.chunks))
                else:
                    stats.append(_bn_stats(Y, M, Cout, gamma, beta, bn, False, dev, st))
                Ys.append(Y)
                W2s.append(W2)
            out, arg = _bn_act_out(Ys[-1], stats[-1], layers[-1][1], pool_ns, st)
        ctx.save_for_backward(A0, arg, *Ys, *stats, *W2s, *(acts if plan[0].bwd else []))
        ctx.cfg = (L, pool_ns, training, [s_ for _, s_ in layers], [tuple(params[3 * l].shape) for l in range(L)], cins)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L, pool_ns, training, slopes, wshapes, cins = ctx.cfg
        saved = ctx.saved_tensors
        A0, arg = saved[0], saved[1]
        Ys, stats, W2s = saved[2:2 + L], saved[2 + L:2 + 2 * L], saved[2 + 2 * L:2 + 3 * L]
        dev = grad_out.device
        st = _lib.stream_ptr(dev)
        M = A0.shape[0]
        dcur = grad_out.contiguous()
        grads = [None] * (3 * L)
        if not ctx.plan[0].bwd:  # (the forward pass saw no gradient request: it kept no operands for this)
            raise RuntimeError("_MLPChain.backward: the forward pass ran without a gradient request (grad mode off at the call site)")
        acts = saved[2 + 3 * L:2 + 3 * L + (L - 1)]  # the activated rows the plan kept (side outputs of the forward kernels)
        red_next = None  # reductions of the next layer down, when the weight-gradient kernel above it produced them
        with _lib.on_device(dev):
            for l in range(L - 1, -1, -1):
                Y, ls, W2, slope, b = Ys[l], stats[l], W2s[l], slopes[l], ctx.plan[l].bwd
                C, Kp = W2.shape
                pooled_arg, ns = (arg, pool_ns) if (pool_ns and l == L - 1) else (None, 0)
                if b.kind == "passes":
                    dY, dgb = _bn_act_bwd(dcur, pooled_arg, Y, ls, slope, ns, training, st)
                    grads[3 * l + 1], grads[3 * l + 2] = dgb[1], dgb[0]
                    if b.wgrad:
                        grads[3 * l] = _chain_wgrad(b, dY, l, A0, acts, Ys, stats, slopes)[0][:, :cins[l]].reshape(wshapes[l])
                    if b.dx:
                        dcur = torch.mm(dY, W2)
                    continue
                red, red_next = red_next, None
                if b.reduce_rev is not None:
                    # dbeta, dgamma, c1, c2 of the layer from the gradient of its activated (or pooled) output
                    red = torch.empty((4, C), dtype=torch.float32, device=dev)
                    _lib.call("tp3d_bn_bwd_reduce_f32", _lib.ptr(dcur), _lib.ptr(pooled_arg), _lib.ptr(Y), _lib.ptr(ls[2]), _lib.ptr(ls[3]),
                              _lib.ptr(ls[0]), _lib.ptr(ls[1]), slope, M, max(ns, 1), C, int(training), _lib.ptr(red[0]),
                              _lib.ptr(red[1]), _lib.ptr(red[2]), _lib.ptr(red[3]), _lib.ptr(_lib.bn_workspace(M, C, dev)), b.reduce_rev, st)
                grads[3 * l + 1], grads[3 * l + 2] = red[1], red[0]
                if b.kind == "narrow":
                    # the first layer of grouped rows (a handful of input channels, nobody reads their gradient): the
                    # reduction pass, then dW straight from (Y, dA, A0) -- dY is never written
                    dW = _chain_wgrad_narrow(dcur, Y, ls, red, slope, A0, b.wgrad_rev, st)
                    grads[3 * l] = dW[:, :cins[l]].reshape(wshapes[l])
                    continue
                # "loader": reductions, then the input-gradient GEMM whose loader waves form dY (side output for dW)
                dY = torch.empty_like(Y) if b.write_dY else None
                # dA_{l-1}[M,Kp] = dY_l[M,C] (W^T)[Kp,C]^T (a transposed copy of the weight: reading it as stored, four
                # strided scalars per slot, made the loader waves the bottleneck -- 8.55 vs 8.32 ms/step)
                dprev = torch.empty((M, Kp), dtype=torch.float32, device=dev)
                c0, ncol = b.cols if b.cols else (0, Kp)
                pad_hi = Kp - c0 - ncol
                Wt = W2.t()[c0:c0 + ncol].contiguous()
                pad_lo_k, pad_hi_k = c0, pad_hi  # columns outside cols the kernel zeroes itself (at most 32 on a side)
                if c0 > 32 or pad_hi > 32:  # (never with grouped / interpolated rows: 3 and <= 3 columns)
                    dprev.zero_()
                    pad_lo_k = pad_hi_k = 0
                _lib.call("tp3d_gemm_rows_bnbwd_sp_f32", _lib.ptr(Y), _lib.ptr(dcur), _lib.ptr(ls[0]), _lib.ptr(ls[2]),
                          _lib.ptr(ls[3]), _lib.ptr(red[2]), _lib.ptr(red[3]), slope, _lib.ptr(Wt), M, ncol, C,
                          _lib.ptr(dprev) + 4 * c0, Kp, pad_lo_k, pad_hi_k, _lib.ptr(dY), _lib.ptr(pooled_arg), max(ns, 1), b.dx_rev, st)
                if b.wgrad:
                    # ("x3_act_red": Y_{l-1} streams through this contraction anyway, the layer below gets its reductions here)
                    dW, red_next = _chain_wgrad(b, dY, l, A0, acts, Ys, stats, slopes, dprev, training)
                    grads[3 * l] = dW[:, :cins[l]].reshape(wshapes[l])
                dcur = dprev
        return (dcur if ctx.plan[0].bwd.dx else None, None, None, None, None) + tuple(grads)


def _chain_ok(rows, parts):
    """the fused layer chain serves MLPs on large row matrices whose widths suit the rows kernel's operands"""
    if not USE_MLP_CHAIN or rows.shape[0] < CHAIN_MIN_ROWS or rows.shape[1] % 4:
        return False
    for conv, bn, slope in parts:
        cout = conv.weight.shape[0]
        if getattr(conv, "bias", None) is not None or cout % 4 or cout < ROWS_GEMM_MIN_COLS or cout > 1536:
            return False
    return True


# The switches of the chain (each the A/B handle of a measured step, `bench.py --set NAME=0|1`; DESIGN.md section 5 has
# the numbers).  The first design -- prologues in the MFMA waves of the plain rows / weight-gradient kernels, the backward
# pass fused the same way (12.0 vs 10.3 ms/step) -- left the tree in round 3 together with its three entry points.
USE_MLP_CHAIN = True        # whole shared MLPs as one autograd node on the split-role / bf16-pipe kernels (else layer by layer)
CHAIN_BWD_LOADER = True     # input-gradient GEMMs form dY in their loader waves (else: apply pass + library GEMM)
CHAIN_BWD_POOLED = True     # ... also for the max-pooled last layer of a set-abstraction MLP (groups of 64, 128 ... rows)
ROW_ORDER_ALTERNATE = True  # consecutive big kernels of a chain walk the rows in opposite directions (`reverse`, tp3d_hip.h)
WGRAD_NARROW = True  # first layer of grouped rows (<= 16 input channels, no input gradient wanted): dW from (Y, dA, A0) in one
                     # streaming kernel (tp3d_gemm_tn_bn_narrow_f32) instead of the dY pass + the 64-column MFMA tile kernel
FWD_NARROW = True    # ... and its forward contraction (tp3d_gemm_rows_narrow_f32) instead of the MFMA tile kernel
WGRAD_RED = True     # a hidden layer's weight-gradient kernel also runs the BatchNorm-backward reductions of the layer below
                     # (tp3d_gemm_tn_x3_act_red_f32: Y of that layer streams through its loader waves anyway)

# The routing of one _MLPChain call, one record per layer, made once at forward time (_plan_chain) and kept for backward:
# kernel "x3_identity" / "narrow" / "rows" (first layer), "x3" / "sp" / "bn_act_rows" (later layers); the statistics chunks it
# leaves; its row direction (None: the plain rows kernel takes none); whether the layer's activated input rows are kept
_ChainLayer = collections.namedtuple("_ChainLayer", "kernel chunks reverse keep_act bwd")
# kind "loader" / "narrow" / "passes"; cols: None or the (first, count) columns of the input gradient contracted; reduce_rev:
# direction of the layer's own tp3d_bn_bwd_reduce_f32 pass, None where the reductions ride on the weight-gradient kernel of
# the layer above ("passes": tp3d_bn_act_bwd_f32 has them); dx: the input gradient is computed, dx_rev: direction of the
# "loader" kernel that does; wgrad None / "tn" / "x3" / "x3_act" / "x3_act_red" / "narrow", its direction ("tn" takes none),
# the chunk count of "x3_act_red", the bf16 term pairs of the "x3" kernels
_ChainLayerBwd = collections.namedtuple("_ChainLayerBwd", "kind cols reduce_rev dx dx_rev write_dY wgrad wgrad_rev wgrad_chunks terms")


def _plan_chain(M, K0, widths, pool_ns, want_grad, need_in, need_w, grad_cols):
    """The complete routing of one _MLPChain call on (M, K0) rows through layers of the given output widths, as a tuple of
    _ChainLayer: sizes and flags in, plain data out.  The switches above and the library's shape queries are read here and
    nowhere else, so the backward pass runs what the forward pass prepared for.  want_grad: a backward pass can come;
    need_in / need_w[l]: the gradients of the input rows / of layer l's weight are wanted."""
    h = _lib.load()
    L = len(widths)
    Ks = [K0] + list(widths[:-1])
    alt = bool(ROW_ORDER_ALTERNATE)
    # the bf16-pipe weight-gradient contraction serves the layer: its loader waves can form the activated rows again from
    # Y_{l-1} (tp3d_gemm_tn_x3_act_f32), so the forward kernels need not keep them
    tn = ["x3" if WGRAD_X3 and h.tp3d_gemm_tn_x3_serves(M, widths[l], Ks[l]) else "tn" for l in range(L)]
    keep = [bool(want_grad and l > 0 and not (WGRAD_X3_ACT and need_w[l] and tn[l] == "x3")) for l in range(L)]

    # alternate the direction the row blocks are walked in, layer by layer: a layer starts where the previous one (or the
    # producer of A0, front to back) ended, on the rows the memory-side cache still holds; the plain rows kernel takes no
    # direction and walks front to back
    fwd, prev = [], 0
    for l in range(L):
        Cout, Kp, side = widths[l], Ks[l], int(keep[l])
        sp = h.tp3d_gemm_rows_sp_chunks(M, Cout, Kp, side) if l else 0
        x3 = h.tp3d_gemm_rows_x3_chunks(M, Cout, Kp, side) if (FWD_X3 and (sp or not l)) else 0
        if x3:  # the bf16 matrix pipe; the first layer with the identity as its BatchNorm + activation prologue
            kernel, chunks = "x3" if l else "x3_identity", x3
        elif sp:
            kernel, chunks = "sp", sp
        elif not l and FWD_NARROW and h.tp3d_gemm_tn_bn_narrow_serves(M, Cout, Kp):
            kernel, chunks = "narrow", h.tp3d_gemm_rows_narrow_chunks(M)
        else:
            kernel, chunks = "bn_act_rows" if l else "rows", h.tp3d_gemm_rows_stat_chunks(M, Cout)
        directed = kernel not in ("rows", "bn_act_rows")
        prev = int(directed and alt and not prev)
        fwd.append((kernel, chunks, prev if directed else None, keep[l]))
    if not want_grad:
        return tuple(_ChainLayer(*f, bwd=None) for f in fwd)

    kinds, cols = [], []
    for l in range(L):
        C, Kp = widths[l], Ks[l]
        pooled = bool(pool_ns) and l == L - 1
        want_prev = l > 0 or need_in
        # the grouped rows' producer reads the gradient of the feature columns only: contract just those
        cols.append(grad_cols if (l == 0 and grad_cols is not None and grad_cols[1] >= ROWS_GEMM_MIN_COLS) else None)
        pow2 = pooled and pool_ns >= 64 and (pool_ns & (pool_ns - 1)) == 0
        if (CHAIN_BWD_LOADER and (not pooled or (CHAIN_BWD_POOLED and pow2)) and want_prev
                and h.tp3d_gemm_rows_bnbwd_sp_serves(M, cols[l][1] if cols[l] else Kp, C)):
            kinds.append("loader")
        elif (WGRAD_NARROW and not pooled and not want_prev and need_w[l] and l == 0
                and h.tp3d_gemm_tn_bn_narrow_serves(M, C, Kp)):
            kinds.append("narrow")
        else:
            kinds.append("passes")

    # consecutive big kernels walk the rows in opposite directions: each starts on the rows its predecessor touched
    # last, which the memory-side cache (256 MB against 268 MB per activation matrix) still holds.  `turn` counts them;
    # the even ones walk last to first (the producer of grad_out wrote front to back)
    rev = (int(alt), 0)
    bwd, turn = [None] * L, 0
    red_above = False  # the weight-gradient kernel of the layer above produces this layer's reductions
    for l in range(L - 1, -1, -1):
        plain = "x3_act" if (l > 0 and not keep[l]) else tn[l]  # the weight-gradient kernel without reductions
        if kinds[l] == "passes":  # (the kernels after a pass of their own walk front to back)
            wgrad = plain if need_w[l] else None
            bwd[l] = _ChainLayerBwd("passes", cols[l], None, l > 0 or need_in, None, True, wgrad, 0 if wgrad in ("x3", "x3_act") else None,
                                    0, WGRAD_X3)
            continue
        reduce_rev = None
        if not red_above:
            reduce_rev, turn = rev[turn % 2], turn + 1
        red_above = False
        if kinds[l] == "narrow":
            bwd[l] = _ChainLayerBwd("narrow", cols[l], reduce_rev, False, None, False, "narrow", rev[turn % 2], 0, WGRAD_X3)
            turn += 1
            continue
        dx_rev, turn = rev[turn % 2], turn + 1
        wgrad, wgrad_rev, chunks = None, None, 0
        if need_w[l] and WGRAD_RED and l > 0 and not keep[l] and kinds[l - 1] != "passes":
            chunks = h.tp3d_gemm_tn_x3_red_chunks(M, widths[l], Ks[l]) if WGRAD_X3 == 6 else 0
            if chunks:
                wgrad, wgrad_rev, red_above = "x3_act_red", rev[turn % 2], True
            turn += 1  # also where the kernel declines the shape (the skipped turn): kept for bit-identity with earlier results
        if need_w[l] and not chunks:
            wgrad, wgrad_rev, turn = plain, (rev[turn % 2] if plain != "tn" else None), turn + 1
        bwd[l] = _ChainLayerBwd("loader", cols[l], reduce_rev, True, dx_rev, need_w[l], wgrad, wgrad_rev, chunks, WGRAD_X3)
    return tuple(_ChainLayer(*f, bwd=b) for f, b in zip(fwd, bwd))


class _BNAct(torch.autograd.Function):
    """out = LeakyReLU(BatchNorm(Y)) on rows (M, C): the BatchNorm + activation that follows a KPConv (SimpleBlock,
    modules/KPConv/blocks.py:86-89) or any other row-major producer; with pool_ns > 0 also the max over groups of
    pool_ns consecutive rows (first maximum wins)."""

    @staticmethod
    def forward(ctx, Y, gamma, beta, bn, slope, pool_ns=0):
        dev = Y.device
        Y = Y.contiguous()
        M, C = Y.shape
        training = bn.training
        st = _lib.stream_ptr(dev)
        with _lib.on_device(dev):
            stats = _bn_stats(Y, M, C, gamma, beta, bn, training, dev, st)  # mean, invstd, scale, shift
            out, arg = _bn_act_out(Y, stats, slope, pool_ns, st)
        ctx.save_for_backward(Y, stats, arg)
        ctx.cfg = (slope, training, pool_ns)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        Y, stats, arg = ctx.saved_tensors
        slope, training, pool_ns = ctx.cfg
        dev = grad_out.device
        with _lib.on_device(dev):
            dY, dgb = _bn_act_bwd(grad_out.contiguous(), arg, Y, stats, slope, pool_ns, training, _lib.stream_ptr(dev))
        return dY, dgb[1], dgb[0], None, None, None


def bn_act(Y, bn, slope, pool_ns=0):
    return _BNAct.apply(Y, bn.weight, bn.bias, bn, slope, pool_ns)


def relation_rows(pos, new_pos, idx):
    """(B*np*ns, 12) rows [ |d|, centroid xyz, neighbour xyz, d, 0, 0 ] of Relation-Shape convolution (no gradient:
    positions are data)."""
    dev = pos.device
    B, N, _ = pos.shape
    _, npnt, ns = idx.shape
    out = torch.empty((B * npnt * ns, 12), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_relation_rows_f32", _lib.ptr(pos.contiguous()), _lib.ptr(new_pos.contiguous()),
                  _lib.ptr(idx.contiguous()), B, N, npnt, ns, 12, _lib.ptr(out), _lib.stream_ptr(dev))
    return out


class _NbrMaxPool(torch.autograd.Function):
    """max over each query's neighbours of the support rows, shadow neighbours contributing zeros."""

    @staticmethod
    def forward(ctx, x, nbr):
        dev = x.device
        xf = x.contiguous()
        Nq, Mn = nbr.shape
        M, C = xf.shape
        out = torch.empty((Nq, C), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0]
        arg = torch.empty((Nq, C), dtype=torch.int32, device=dev) if need else None
        with _lib.on_device(dev):
            _lib.call("tp3d_nbr_maxpool_fwd_f32", _lib.ptr(xf), _lib.ptr(nbr), Nq, M, Mn, C, _lib.ptr(out), _lib.ptr(arg),
                      _lib.stream_ptr(dev))
        ctx.save_for_backward(nbr, arg)
        ctx.cfg = (M, C)
        return out

    @staticmethod
    def backward(ctx, g):
        nbr, arg = ctx.saved_tensors
        M, C = ctx.cfg
        dev = g.device
        g = g.contiguous()
        Nq, Mn = nbr.shape
        dx = torch.empty((M, C), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            inv, inv_bytes, ready, token = _lib.neighbour_inverse(nbr, M, dev)
            _lib.call("tp3d_nbr_maxpool_bwd_f32", _lib.ptr(g), _lib.ptr(arg), _lib.ptr(nbr), Nq, M, Mn, C, _lib.ptr(dx),
                      _lib.ptr(inv), inv_bytes, ready, _lib.stream_ptr(dev))
            _lib.inverse_built(token, dev)
        return dx, None


def nbr_maxpool(x, nbr):
    return _NbrMaxPool.apply(x.float(), nbr)


def linear_bn_act(A, conv, bn, slope, pool_ns=0):
    return _LinearBNAct.apply(A, conv.weight, bn.weight, bn.bias, bn, slope, pool_ns, torch.is_grad_enabled(), getattr(conv, "bias", None))


def _bn1d_of(m):
    """nn.BatchNorm1d inside a FastBatchNorm1d-style wrapper (attribute `batch_norm`) or the module itself."""
    inner = getattr(m, "batch_norm", m)
    if isinstance(inner, nn.BatchNorm1d) and inner.affine and inner.track_running_stats and inner.momentum is not None:
        return inner
    return None


def seq_parts(seq):
    """(linear, bn1d, slope) of nn.Sequential(Linear, BatchNorm[, activation]) or None."""
    mods = list(seq.children()) if isinstance(seq, nn.Sequential) else []
    if len(mods) not in (2, 3) or not isinstance(mods[0], nn.Linear):
        return None
    bn = _bn1d_of(mods[1])
    slope = _slope_of(mods[2] if len(mods) == 3 else None)
    if bn is None or slope is None:
        return None
    return mods[0], bn, slope


def rows_seq(seq, x):
    """Linear -> BatchNorm1d -> activation on rows (N, C) through the fused kernels when the block has that shape and
    the rows live on the GPU; otherwise the module itself."""
    parts = seq_parts(seq) if x.is_cuda else None
    if parts is None:
        return seq(x)
    lin, bn, slope = parts
    return linear_bn_act(x.float(), lin, bn, slope)


def rows_mlp(mlp, x):
    """A partial-dense MLP: nn.Sequential of [Linear, BatchNorm, activation] blocks."""
    for block in mlp.children():
        x = rows_seq(block, x)
    return x


def run_mlp(rows, parts, pool_ns=0):
    """Shared MLP over rows; the last layer optionally max-pools groups of pool_ns consecutive rows."""
    if _chain_ok(rows, parts):
        flat = []
        for conv, bn, slope in parts:
            flat += [conv.weight, bn.weight, bn.bias]
        return _MLPChain.apply(rows, pool_ns, [(bn, slope) for _, bn, slope in parts], getattr(rows, "_tp3d_grad_cols", None),
                               torch.is_grad_enabled(), *flat)
    for i, (conv, bn, slope) in enumerate(parts):
        rows = linear_bn_act(rows, conv, bn, slope, pool_ns if i == len(parts) - 1 else 0)
    return rows


def scatter_table(idx, weight, nbins, div):
    """The inverted form of a neighbour table idx (B, rows, slots) over `nbins` support points (with the interpolation
    weights lined up, if given): what the backward pass of group_concat / interp_concat gathers through.  It depends on
    the geometry only, so a stepper that computes the geometry ahead of the training pass (dp.PipelinedStep) builds it
    there as well; pass it as `table=` and the backward pass skips the inversion."""
    dev = idx.device
    B = idx.shape[0]
    L = idx[0].numel()
    nbytes = _lib.load().tp3d_scatter_workspace_bytes(B, L, nbins, int(weight is not None))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idx = idx.contiguous()
    w = None if weight is None else weight.contiguous()
    with _lib.on_device(dev):
        _lib.call("tp3d_rows_scatter_invert", _lib.ptr(idx), _lib.ptr(w), B, L, div, nbins, _lib.ptr(buf), nbytes,
                  _lib.stream_ptr(dev))
    return buf


class _GroupConcat(torch.autograd.Function):
    """rows[(b,j,s)] = [pos[b,idx]-new_pos[b,j] (/r), x_cl[b,idx], 0-pad to 4k columns]; differentiable wrt x_cl."""

    @staticmethod
    def forward(ctx, pos, new_pos, x_cl, idx, radius, normalize, table=None):
        dev = pos.device
        B, N, _ = pos.shape
        _, npnt, ns = idx.shape
        C = 0 if x_cl is None else x_cl.shape[2]
        pos, new_pos, idx = pos.contiguous(), new_pos.contiguous(), idx.contiguous()
        xc = None if x_cl is None else x_cl.contiguous()
        ld = _pad4(C + 3)
        out = torch.empty((B * npnt * ns, ld), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.call("tp3d_group_concat_fwd_f32", _lib.ptr(pos), _lib.ptr(new_pos), _lib.ptr(xc), _lib.ptr(idx), B, N,
                      npnt, ns, C, ld, float(radius), int(bool(normalize)), _lib.ptr(out), _lib.stream_ptr(dev))
        ctx.save_for_backward(idx, table)
        ctx.dims = (B, N, npnt, ns, C, ld)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        idx, table = ctx.saved_tensors
        B, N, npnt, ns, C, ld = ctx.dims
        if C == 0 or not ctx.needs_input_grad[2]:
            return None, None, None, None, None, None, None
        dev = grad_rows.device
        grad_rows = grad_rows.contiguous()
        g = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        L = npnt * ns
        with _lib.on_device(dev):
            if table is not None:  # inverted ahead of the pass (scatter_table)
                _lib.call("tp3d_rows_scatter_apply_f32", _lib.ptr(grad_rows), B, L, 1, N, ld, 3, C, 0, _lib.ptr(g),
                          _lib.ptr(table), table.numel(), _lib.stream_ptr(dev))
            else:
                ws, ws_bytes = _lib.scatter_workspace(B, L, N, False, dev)
                _lib.call("tp3d_rows_scatter_bwd_f32", _lib.ptr(grad_rows), _lib.ptr(idx), None, B, L, 1, N, ld, 3, C,
                          _lib.ptr(g), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev))
        return None, None, g, None, None, None, None


def group_concat(pos, new_pos, x_cl, idx, radius, normalize, table=None):
    rows = _GroupConcat.apply(pos, new_pos, x_cl, idx, radius, normalize, table)
    if x_cl is not None:
        rows._tp3d_grad_cols = (3, x_cl.shape[2])  # _GroupConcat.backward reads these columns of the gradient and no others
    return rows


class _InterpConcat(torch.autograd.Function):
    """rows[(b,i)] = [sum_t w_t * feat_cl[b, idx_t], skip_cl[b,i]]; differentiable wrt feat_cl and skip_cl."""

    @staticmethod
    def forward(ctx, feat_cl, idx, weight, skip_cl, table=None):
        dev = feat_cl.device
        B, m, C1 = feat_cl.shape
        n = idx.shape[1]
        C2 = 0 if skip_cl is None else skip_cl.shape[2]
        feat_cl, idx, weight = feat_cl.contiguous(), idx.contiguous(), weight.contiguous()
        sk = None if skip_cl is None else skip_cl.contiguous()
        ld = _pad4(C1 + C2)
        out = torch.empty((B * n, ld), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.call("tp3d_interp_concat_fwd_f32", _lib.ptr(feat_cl), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(sk), B,
                      m, n, C1, C2, ld, _lib.ptr(out), _lib.stream_ptr(dev))
        ctx.save_for_backward(idx, weight, table)
        ctx.dims = (B, m, n, C1, C2, ld)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        idx, weight, table = ctx.saved_tensors
        B, m, n, C1, C2, ld = ctx.dims
        dev = grad_rows.device
        grad_rows = grad_rows.contiguous()
        g_feat = None
        if ctx.needs_input_grad[0]:
            g_feat = torch.empty((B, m, C1), dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                if table is not None:  # inverted ahead of the pass (scatter_table)
                    _lib.call("tp3d_rows_scatter_apply_f32", _lib.ptr(grad_rows), B, 3 * n, 3, m, ld, 0, C1, 1,
                              _lib.ptr(g_feat), _lib.ptr(table), table.numel(), _lib.stream_ptr(dev))
                else:
                    ws, ws_bytes = _lib.scatter_workspace(B, 3 * n, m, True, dev)
                    _lib.call("tp3d_rows_scatter_bwd_f32", _lib.ptr(grad_rows), _lib.ptr(idx), _lib.ptr(weight), B, 3 * n,
                              3, m, ld, 0, C1, _lib.ptr(g_feat), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev))
        g_skip = None
        if C2 and ctx.needs_input_grad[3]:
            g_skip = grad_rows.view(B, n, ld)[:, :, C1:C1 + C2]
        return g_feat, None, None, g_skip, None


def interp_concat(feat_cl, idx, weight, skip_cl, table=None):
    rows = _InterpConcat.apply(feat_cl, idx, weight, skip_cl, table)
    if skip_cl is not None and not (skip_cl.requires_grad and torch.is_grad_enabled()):
        # the skip columns carry no gradient (the network's input features): _InterpConcat.backward reads the interpolated
        # columns of the rows' gradient and no others
        rows._tp3d_grad_cols = (0, feat_cl.shape[2])
    return rows


def cat_rows(parts):
    """cat of (B, n, C_i) tensors on the channel axis -> (B*n, pad4(sum C_i)) rows with zero padding columns."""
    B, n = parts[0].shape[0], parts[0].shape[1]
    width = sum(p.shape[2] for p in parts)
    if _pad4(width) != width:
        parts = list(parts) + [parts[0].new_zeros((B, n, _pad4(width) - width))]
    return torch.cat(parts, 2).reshape(B * n, -1)


def idw_weights(dist):
    """(1/(d+1e-8)) / sum over the 3 neighbours, evaluated in the reference's order (dense.py:137-139)."""
    dev = dist.device
    dist = dist.contiguous()
    w = torch.empty_like(dist)
    with _lib.on_device(dev):
        _lib.call("tp3d_idw_weights_f32", _lib.ptr(dist), dist.numel() // 3, _lib.ptr(w), _lib.stream_ptr(dev))
    return w
