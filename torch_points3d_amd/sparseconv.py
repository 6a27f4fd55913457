"""Sparse voxel convolution (the SparseConv3d family) on MI355X.

Mirrors torch_points3d/modules/SparseConv3d/nn/torchsparse.py (`Conv3d`, `Conv3dTranspose`, `BatchNorm`, `ReLU`, `cat`,
`SparseTensor`), modules/SparseConv3d/modules.py (`ResBlock`, `BottleneckBlock`, `ResNetDown`, `ResNetUp`) and the two
networks applications/sparseconv3d.py assembles from applications/conf/sparseconv3d/*.yaml (`SparseConv3dUnet`,
`SparseConv3dEncoder`): same constructor arguments and attribute names, hence state_dict keys.

Semantics ("Sparse voxel convolution"): a sparse tensor is F (N, C) fp32, C (N, 4) int32 [x, y, z, batch], a
tensor stride s and a cache, shared by every tensor derived from it, of coordinate sets per stride and kernel maps per
(kernel_size, tensor stride, stride).  Offsets are {-1, 0, 1} * s per axis for an odd kernel and {0, 1} * s for
kernel_size 2, the kernel index has x slowest and z fastest, the weight is `kernel` (k^3, Cin, Cout) ((Cin, Cout) for
k = 1).  That shape and offset order are recalled from torchsparse 1.x; neither torchsparse nor MinkowskiEngine could be
run next to this code, so a reference checkpoint's offset order is NOT verified.  The dense equivalents (F.conv3d with
padding 1 / F.conv_transpose3d) are what the tests hold the kernels to.

Coordinate sets and kernel maps are built on the device (csrc/sparseconv.hip): one device->host read per new set,
none for a cached one.  Every product -- forward, transposed forward and both input gradients -- is one gather-GEMM
kernel over a table this module built; the weight gradient is a second kernel with a fixed-order reduction.
"""
import torch
import torch.nn as nn

from . import _lib
from . import fused as _fused
from . import torchpoints as _tp
from .kpconv import _require_gpu
from .kpconv_blocks import FastBatchNorm1d

# Route of the first layer of a wide kernel (Cin <= 4, 27 < K <= 125: WideConv3d with kernel_size 5).  "wide": the
# hit-compacting kernels (tp3d_sparse_conv_wide_f32, tp3d_sparse_wgrad_wide_f32) wherever they serve the shape; "generic":
# the kernels every other layer takes; "auto": the wide kernels for the shape classes where tools/bench_ms_svconv.py
# (profiles/ms_svconv_bench.json, MI355X) measured them faster than the generic route by more than the spread of its 30
# samples: Cin = 1 (forward 0.099 vs 0.130 ms, weight gradient 0.23 vs 0.59 ms at Cout = 32).  At Cin = 4 the forward ties
# (0.206 vs 0.204 ms) and the weight gradient loses (0.78 vs 0.59 ms); Cin = 2 and 3 are not measured: all generic.
WIDE_ROUTE = "auto"

COORD_LIMIT = 1 << 18  # |x|, |y|, |z| below this at tensor stride 1
BATCH_LIMIT = 1 << 9   # batch index below this ...
CLOUD_LIMIT_MAX = 1 << 24  # ... or below SparseTensor(clouds=K), K up to this (SP_CLOUD_LIMIT_MAX of csrc/sparseconv.hip)
_BAD_RANGE, _BAD_DUP, _BAD_SPAN = 1, 2, 4


def _check_clouds(clouds):
    """the opt-in bound on the batch index: None (2^9, the default) or an int in [1, 2^24]"""
    if clouds is None:
        return None
    if isinstance(clouds, bool) or int(clouds) != clouds or not 1 <= int(clouds) <= CLOUD_LIMIT_MAX:
        raise ValueError("clouds must be None or an integer in [1, 2^24], got %r" % (clouds,))
    return int(clouds)


def _raise_bad(flags, clouds=None):
    if flags & _BAD_RANGE:
        raise ValueError("sparse coordinates out of range: need 0 <= batch < %s and every voxel [c, c + tensor stride) to "
                         "hold a coordinate with |x|, |y|, |z| < 2^18" % ("2^9" if clouds is None else "clouds = %d" % clouds))
    if flags & _BAD_SPAN:
        raise ValueError("sparse coordinates span too large a box: extent_x * extent_y * extent_z * batches must stay "
                         "below 2^62")
    if flags & _BAD_DUP:
        raise ValueError("duplicate coordinates in a sparse tensor: every (x, y, z, batch) row must be distinct")


def check_coords_host(coords, stride=1, clouds=None):
    """The accepted-input rule on a host tensor (what the device build flags in its read-back): a voxel of tensor stride
    `stride` covers [c, c + stride) per axis and must hold a coordinate of (-2^18, 2^18) -- |c| < 2^18 at stride 1, and
    -2^18 itself (the floor of -(2^18 - 1)) at a coarser one.  The batch index stays below 2^9, or below `clouds`."""
    limit = BATCH_LIMIT if _check_clouds(clouds) is None else int(clouds)
    c = coords.long()
    flags = 0
    if c.numel():
        xyz = c[:, :3]
        if (bool((xyz >= COORD_LIMIT).any()) or bool((xyz + stride - 1 <= -COORD_LIMIT).any()) or bool((c[:, 3] < 0).any())
                or bool((c[:, 3] >= limit).any())):
            flags |= _BAD_RANGE
        elif torch.unique(c, dim=0).shape[0] != c.shape[0]:
            flags |= _BAD_DUP
    _raise_bad(flags, clouds)


class _CoordSet(object):
    """coords (n, 4) int32 in the set's row order, sorted keys, owner row per sorted slot, 16 ints of bounds (device)."""

    __slots__ = ("coords", "keys", "rows", "meta", "n")

    def __init__(self, coords, keys, rows, meta, n):
        self.coords, self.keys, self.rows, self.meta, self.n = coords, keys, rows, meta, n


def _build_set(coords, ts, down, clouds=None):
    """`coords` of tensor stride ts.  down == 0: their set; else the distinct floor(c / down) * down, ascending (batch, x, y, z).
    clouds: the bound on the batch index when it is not 2^9 (tp3d_sparse_set_build_clouds_i32)."""
    dev = coords.device
    N = coords.shape[0]
    if N == 0:
        raise ValueError("a sparse tensor needs at least one voxel")
    keys = torch.empty((N,), dtype=torch.int64, device=dev)
    rows = torch.empty((N,), dtype=torch.int32, device=dev)
    out_coords = torch.empty((N, 4), dtype=torch.int32, device=dev) if down else None
    meta = torch.empty((16,), dtype=torch.int32, device=dev)
    nbytes = _lib.load().tp3d_sparse_workspace_bytes(N)
    ws = _lib.workspace("sparse_set", nbytes, dev)
    with _lib.on_device(dev):
        if clouds is None:
            _lib.call("tp3d_sparse_set_build_i32", _lib.ptr(coords), N, int(ts), int(down), _lib.ptr(keys), _lib.ptr(rows),
                      _lib.ptr(out_coords), _lib.ptr(meta), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        else:
            _lib.call("tp3d_sparse_set_build_clouds_i32", _lib.ptr(coords), N, int(ts), int(down), int(clouds), _lib.ptr(keys),
                      _lib.ptr(rows), _lib.ptr(out_coords), _lib.ptr(meta), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    host = meta.cpu()  # the one read of a new set: row count and bad-input flags
    _raise_bad(int(host[7]), clouds)
    n = int(host[8])
    if down:
        return _CoordSet(out_coords[:n], keys[:n], rows[:n], meta, n)
    return _CoordSet(coords, keys, rows, meta, n)


class _KernelMap(object):
    """forward (Nout, K): input row at coord(o) + offset_k; inverse (Nin, K): output row o with in(o, k) == i."""

    __slots__ = ("forward", "inverse", "n_in", "n_out", "K")

    def __init__(self, forward, inverse, n_in, n_out, K):
        self.forward, self.inverse, self.n_in, self.n_out, self.K = forward, inverse, n_in, n_out, K


def _search(coords, n, ksize, step, sign, target):
    """(n, ksize^3) int32: rows of the coordinate set `target` at coords + sign * offsets * step, -1 where absent (any
    query coordinates: a set's own, or the quantised points of pvcnn.py)"""
    dev = coords.device
    table = torch.empty((n, ksize ** 3), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_sparse_kmap_i32", _lib.ptr(coords), n, ksize, int(step), sign, _lib.ptr(target.keys),
                  _lib.ptr(target.rows), _lib.ptr(target.meta), target.n, _lib.ptr(table), _lib.stream_ptr(dev))
    return table


def _build_kmap(in_set, out_set, ksize, ts, same_set):
    forward = _search(out_set.coords, out_set.n, ksize, ts, 1, in_set)
    if same_set and ksize % 2 == 1:
        dev = forward.device
        inverse = torch.empty_like(forward)
        with _lib.on_device(dev):
            _lib.call("tp3d_sparse_kmap_mirror_i32", _lib.ptr(forward), in_set.n, ksize ** 3, _lib.ptr(inverse),
                      _lib.stream_ptr(dev))
    else:
        inverse = _search(in_set.coords, in_set.n, ksize, ts, -1, out_set)
    return _KernelMap(forward, inverse, in_set.n, out_set.n, ksize ** 3)


class SparseTensor(object):
    """F (N, C) fp32 features, C (N, 4) int32 [x, y, z, batch], s the tensor stride; `cmaps` / `kmaps` are shared by every
    tensor derived from this one.  Host tensors are validated on construction; device tensors in the read-back of the
    first coordinate-set build.  `clouds` = None: batch indices below 2^9.  clouds = K (up to 2^24): batch indices in
    [0, K) -- one cloud per cluster of PointGroup's scorers; every coordinate set of the tensor is then built with that
    bound and every tensor derived from it (`_like`, strided outputs, `cat`) inherits it.  The key holds extent_x *
    extent_y * extent_z * clouds < 4e18, so many clouds want a scene-sized box.  (`clouds` is the last parameter, behind
    the caches, so that positional callers keep working; pass it by keyword.)"""

    def __init__(self, feats, coords, stride=1, cmaps=None, kmaps=None, clouds=None):
        if coords.dim() != 2 or coords.shape[1] != 4 or feats.dim() != 2 or feats.shape[0] != coords.shape[0]:
            raise ValueError("SparseTensor needs feats (N, C) and coords (N, 4) = [x, y, z, batch]")
        self.F = feats
        self.C = coords if coords.dtype == torch.int32 else coords.int()
        self.s = int(stride)
        self.clouds = _check_clouds(clouds)
        self.cmaps = {} if cmaps is None else cmaps
        self.kmaps = {} if kmaps is None else kmaps
        if cmaps is None and self.C.device.type != "cuda":
            check_coords_host(self.C, self.s, self.clouds)

    def to(self, device):
        device = torch.device(device)
        if device == self.F.device:
            return self
        return SparseTensor(self.F.to(device), self.C.to(device), self.s, clouds=self.clouds)

    def _like(self, feats):
        return SparseTensor(feats, self.C, self.s, self.cmaps, self.kmaps, self.clouds)

    def _on(self, feats, ts):
        """`feats` on this tensor's cached coordinate set of tensor stride ts"""
        return SparseTensor(feats, self.cmaps[ts].coords, ts, self.cmaps, self.kmaps, self.clouds)

    def __add__(self, other):
        return self._like(self.F + other.F)

    # coordinate sets and kernel maps ------------------------------------------------------------------------------
    def _set(self, ts):
        cs = self.cmaps.get(ts)
        if cs is None and ts == self.s:
            _require_gpu(self.C)
            cs = self.cmaps[ts] = _build_set(self.C.contiguous(), ts, 0, self.clouds)
        return cs

    def _kmap(self, ksize, ts, stride):
        """the map between the set of stride ts (input side) and the set of stride ts * stride (output side)"""
        key = (ksize, ts, stride)
        km = self.kmaps.get(key)
        if km is None:
            in_set = self.cmaps.get(ts) if ts != self.s else self._set(ts)
            if in_set is None:
                raise RuntimeError("no coordinate set of tensor stride %d: a transposed convolution of stride %d returns to "
                                   "the set a forward convolution started from, and none has produced it" % (ts, stride))
            if stride == 1:
                out_set = in_set
            else:
                out_set = self.cmaps.get(ts * stride)
                if out_set is None:
                    if ts != self.s:
                        raise RuntimeError("no coordinate set of tensor stride %d" % (ts * stride))
                    out_set = self.cmaps[ts * stride] = _build_set(in_set.coords, ts, ts * stride, self.clouds)
            km = self.kmaps[key] = _build_kmap(in_set, out_set, ksize, ts, stride == 1)
        return km


def cat(*args):
    """concatenates the features of tensors on the same coordinate set"""
    first = args[0]
    for t in args[1:]:
        if t.s != first.s or t.F.shape[0] != first.F.shape[0]:
            raise ValueError("cat needs tensors on one coordinate set")
    return first._like(torch.cat([t.F for t in args], dim=1))


def _wide_route(K, cin):
    """True when the layer (K offsets, cin input channels) is one the wide kernels are meant for and WIDE_ROUTE asks for them"""
    if WIDE_ROUTE not in ("auto", "wide", "generic"):
        raise ValueError("sparseconv.WIDE_ROUTE must be 'auto', 'wide' or 'generic', not %r" % (WIDE_ROUTE,))
    return K > 27 and (cin == 1 if WIDE_ROUTE == "auto" else (WIDE_ROUTE == "wide" and cin <= 4))


def _conv_launch(x, table, W, n_out, K, cin, cout, transposed):
    dev = x.device
    y = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    if not transposed and _wide_route(K, cin) and _lib.load().tp3d_sparse_conv_wide_serves(K, cin, cout):
        with _lib.on_device(dev):
            _lib.call("tp3d_sparse_conv_wide_f32", _lib.ptr(x), _lib.ptr(table), _lib.ptr(W), n_out, x.shape[0], K, cin, cout,
                      _lib.ptr(y), _lib.stream_ptr(dev))
        return y
    with _lib.on_device(dev):
        _lib.call("tp3d_sparse_conv_f32", _lib.ptr(x), _lib.ptr(table), _lib.ptr(W), n_out, x.shape[0], K, cin, cout,
                  int(transposed), _lib.ptr(y), _lib.stream_ptr(dev))
    return y


class _GatherConv(torch.autograd.Function):
    """y[r] = sum_k x[table_y[r, k]] . W[k]; table_x (rows of x, K) is the adjoint table (dX gathers dy through it)."""

    @staticmethod
    def forward(ctx, x, W, table_y, table_x):
        x = x.detach().float().contiguous()
        Wc = W.detach().float().contiguous()
        K, cin, cout = Wc.shape
        y = _conv_launch(x, table_y, Wc, table_y.shape[0], K, cin, cout, False)
        ctx.save_for_backward(x, Wc, table_y, table_x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, table_y, table_x = ctx.saved_tensors
        K, cin, cout = W.shape
        dy = dy.float().contiguous()
        dev = dy.device
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _conv_launch(dy, table_x, W, x.shape[0], K, cout, cin, True)
        if ctx.needs_input_grad[1]:
            n = table_y.shape[0]
            dw = torch.empty_like(W)
            h = _lib.load()
            # (a shape the wide kernel declines -- its accumulators do not fit the LDS -- has no chunks: the generic kernel)
            wide = _wide_route(K, cin) and h.tp3d_sparse_wgrad_wide_chunks(n, K, cin, cout) > 0
            entry = "tp3d_sparse_wgrad_wide_f32" if wide else "tp3d_sparse_wgrad_f32"
            floats = (h.tp3d_sparse_wgrad_wide_workspace_floats if wide else h.tp3d_sparse_wgrad_workspace_floats)(n, K, cin, cout)
            ws = _lib.workspace("sparse_wgrad", 4 * floats, dev) if floats else None
            with _lib.on_device(dev):
                _lib.call(entry, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(table_y), n, x.shape[0], K, cin, cout,
                          _lib.ptr(dw), _lib.ptr(ws), floats, _lib.stream_ptr(dev))
        return dx, dw, None, None


class _RowsLinear(torch.autograd.Function):
    """kernel_size 1: y = x @ W on the rows GEMM (csrc/gemm_rows.hip), weight gradient on csrc/gemm_tn.hip."""

    @staticmethod
    def forward(ctx, x, W):
        x = x.detach().float().contiguous()
        Wc = W.detach().float().contiguous()
        ctx.save_for_backward(x, Wc)
        return _fused.gemm_rows(x, Wc.t().contiguous())[0]

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.float().contiguous()
        dx = _fused.gemm_rows(dy, W)[0] if ctx.needs_input_grad[0] else None
        dw = _fused.gemm_tn(x, dy, x3=0) if ctx.needs_input_grad[1] else None
        return dx, dw


def _check_conv_args(kernel_size, stride, dilation):
    if dilation != 1:
        raise NotImplementedError("sparse convolution: dilation %r is not supported (only 1)" % (dilation,))
    if kernel_size not in (1, 2, 3):
        raise NotImplementedError("sparse convolution: kernel_size %r is not supported (1, 2 or 3; WideConv3d serves "
                                  "kernel_size 5 at stride 1)" % (kernel_size,))
    if stride not in (1, 2):
        raise NotImplementedError("sparse convolution: stride %r is not supported (1 or 2)" % (stride,))


class Conv3d(nn.Module):
    """torchsparse-style sparse convolution: `kernel` (k^3, Cin, Cout), (Cin, Cout) for k = 1; bias off by default."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transposed=False):
        super().__init__()
        self._check_args(kernel_size, stride, dilation, transposed)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation, self.transposed = kernel_size, stride, dilation, transposed
        K = kernel_size ** 3
        shape = (K, in_channels, out_channels) if K > 1 else (in_channels, out_channels)
        self.kernel = nn.Parameter(torch.zeros(*shape))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.reset_parameters()

    @staticmethod
    def _check_args(kernel_size, stride, dilation, transposed):
        _check_conv_args(kernel_size, stride, dilation)

    def reset_parameters(self):
        # torchsparse 1.x: uniform(-std, std), std = 1 / sqrt(fan) with the fan of the side the kernel multiplies
        n = (self.out_channels if self.transposed else self.in_channels) * self.kernel_size ** 3
        std = 1.0 / (n ** 0.5)
        with torch.no_grad():
            self.kernel.uniform_(-std, std)
            if self.bias is not None:
                self.bias.uniform_(-std, std)

    def extra_repr(self):
        return "%d, %d, kernel_size=%d, stride=%d%s" % (self.in_channels, self.out_channels, self.kernel_size, self.stride,
                                                        ", transposed" if self.transposed else "")

    def forward(self, inputs):
        _require_gpu(inputs.F, inputs.C, self.kernel)
        k, st, ts = self.kernel_size, self.stride, inputs.s
        if k == 1 and st == 1:
            W = self.kernel
            if self.in_channels % 4 == 0 and self.out_channels % 4 == 0:
                y = _RowsLinear.apply(inputs.F, W)
            else:  # the rows GEMM contracts in groups of four columns: other widths take the one-offset gather
                km = inputs._kmap(1, ts, 1)
                y = _GatherConv.apply(inputs.F, W.unsqueeze(0), km.forward, km.inverse)
            out = inputs._like(y)
        elif not self.transposed:
            km = inputs._kmap(k, ts, st)
            y = _GatherConv.apply(inputs.F, self.kernel.reshape(k ** 3, self.in_channels, self.out_channels), km.forward,
                                  km.inverse)
            out = inputs._like(y) if st == 1 else inputs._on(y, ts * st)
        else:
            if st > 1 and ts % st != 0:
                raise RuntimeError("transposed sparse convolution of stride %d on a tensor of stride %d" % (st, ts))
            fine = ts // st
            if inputs._set(ts) is None or inputs.cmaps.get(fine) is None:
                raise RuntimeError("transposed sparse convolution: no cached coordinate set of tensor stride %d -- it returns "
                                   "to the set a forward convolution of the same stride started from" % fine)
            km = inputs._kmap(k, fine, st)
            y = _GatherConv.apply(inputs.F, self.kernel.reshape(k ** 3, self.in_channels, self.out_channels), km.inverse,
                                  km.forward)
            out = inputs._on(y, fine)
        if self.bias is not None:
            out.F = out.F + self.bias
        return out


class Conv3dTranspose(Conv3d):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transpose=False):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, dilation=dilation, bias=bias,
                         transposed=True)


class WideConv3d(Conv3d):
    """Conv3d that also takes kernel_size 5: stride 1, dilation 1, not transposed (the first layer of MS-SVConv).  Same
    parameter (`kernel` (k^3, Cin, Cout)) and initialisation; offsets {-2 .. 2} * tensor stride per axis, x slowest, z fastest
    -- the continuation of the recalled torchsparse 1.x order, not verified against a checkpoint.  Up to 4 input
    channels the layer takes the wide kernels (WIDE_ROUTE), else the generic ones."""

    @staticmethod
    def _check_args(kernel_size, stride, dilation, transposed):
        if dilation != 1:
            raise NotImplementedError("sparse convolution: dilation %r is not supported (only 1)" % (dilation,))
        if kernel_size not in (3, 5):
            raise NotImplementedError("WideConv3d: kernel_size %r is not supported (3 or 5)" % (kernel_size,))
        if stride != 1:
            raise NotImplementedError("WideConv3d: stride %r is not supported (only 1)" % (stride,))
        if transposed:
            raise NotImplementedError("WideConv3d: the transposed form is not supported")


class _FeatureBatchNorm(nn.BatchNorm1d):
    def forward(self, inputs):
        return inputs._like(super().forward(inputs.F))


class BatchNorm(nn.Module):
    def __init__(self, num_features, *, eps=1e-5, momentum=0.1):
        super().__init__()
        self.bn = _FeatureBatchNorm(num_features=num_features, eps=eps, momentum=momentum)

    def forward(self, feats):
        return self.bn(feats)

    def __repr__(self):
        return self.bn.__repr__()


class ReLU(nn.ReLU):
    def __init__(self, inplace=True):
        super().__init__(inplace=False)  # (features may be saved by the convolution in front)

    def forward(self, inputs):
        return inputs._like(super().forward(inputs.F))


class Seq(nn.Sequential):
    """core/common_modules/base_modules.py Seq: modules numbered in the order they were appended"""

    def __init__(self):
        super().__init__()
        self._num_modules = 0

    def append(self, module):
        self.add_module(str(self._num_modules), module)
        self._num_modules += 1
        return self


class ResBlock(nn.Module):
    """conv3 - BN - ReLU - conv3 - BN - ReLU plus the (1x1 conv - BN when the width changes) shortcut (modules.py:9-50)"""

    def __init__(self, input_nc, output_nc, convolution):
        super().__init__()
        self.block = (Seq().append(convolution(input_nc, output_nc, kernel_size=3, stride=1)).append(BatchNorm(output_nc))
                      .append(ReLU()).append(convolution(output_nc, output_nc, kernel_size=3, stride=1))
                      .append(BatchNorm(output_nc)).append(ReLU()))
        if input_nc != output_nc:
            self.downsample = Seq().append(Conv3d(input_nc, output_nc, kernel_size=1, stride=1)).append(BatchNorm(output_nc))
        else:
            self.downsample = None

    def forward(self, x):
        out = self.block(x)
        return out + (self.downsample(x) if self.downsample else x)


class BottleneckBlock(nn.Module):
    """1x1 - conv3 - 1x1 at width output_nc // reduction, each with BN and ReLU, plus the shortcut (modules.py:53-87)"""

    def __init__(self, input_nc, output_nc, convolution, reduction=4):
        super().__init__()
        mid = output_nc // reduction
        self.block = (Seq().append(Conv3d(input_nc, mid, kernel_size=1, stride=1)).append(BatchNorm(mid)).append(ReLU())
                      .append(convolution(mid, mid, kernel_size=3, stride=1)).append(BatchNorm(mid)).append(ReLU())
                      .append(Conv3d(mid, output_nc, kernel_size=1)).append(BatchNorm(output_nc)).append(ReLU()))
        if input_nc != output_nc:
            self.downsample = Seq().append(convolution(input_nc, output_nc, kernel_size=1, stride=1)).append(BatchNorm(output_nc))
        else:
            self.downsample = None

    def forward(self, x):
        out = self.block(x)
        return out + (self.downsample(x) if self.downsample else x)


_BLOCKS = {"ResBlock": ResBlock, "BottleneckBlock": BottleneckBlock}


class ResNetDown(nn.Module):
    """strided conv - BN - ReLU, then N blocks (modules.py:93-142)"""

    CONVOLUTION = Conv3d

    def __init__(self, down_conv_nn=[], kernel_size=2, dilation=1, stride=2, N=1, block="ResBlock", **kwargs):
        super().__init__()
        block = _BLOCKS[block]
        conv1_output = down_conv_nn[0] if stride > 1 else down_conv_nn[1]
        conv = self.CONVOLUTION
        conv_first = conv
        if kernel_size > 3:  # (the blocks below are always kernel_size 3)
            if conv is not Conv3d:
                raise NotImplementedError("%s: kernel_size %r is not supported (a transposed convolution takes 2 or 3)"
                                          % (type(self).__name__, kernel_size))
            conv_first = WideConv3d
        self.conv_in = (Seq().append(conv_first(in_channels=down_conv_nn[0], out_channels=conv1_output, kernel_size=kernel_size,
                                                stride=stride, dilation=dilation))
                        .append(BatchNorm(conv1_output)).append(ReLU()))
        if N > 0:
            self.blocks = Seq()
            for _ in range(N):
                self.blocks.append(block(conv1_output, down_conv_nn[1], conv))
                conv1_output = down_conv_nn[1]
        else:
            self.blocks = None

    def forward(self, x):
        out = self.conv_in(x)
        if self.blocks:
            out = self.blocks(out)
        return out


class ResNetUp(ResNetDown):
    """the decoder's form: every convolution of the stage, the stride-1 ones of its blocks included, is transposed"""

    CONVOLUTION = Conv3dTranspose

    def __init__(self, up_conv_nn=[], kernel_size=2, dilation=1, stride=2, N=1, **kwargs):
        super().__init__(down_conv_nn=up_conv_nn, kernel_size=kernel_size, dilation=dilation, stride=stride, N=N, **kwargs)

    def forward(self, x, skip):
        return super().forward(cat(x, skip) if skip is not None else x)


def sparseconv3d_config(name, input_nc, in_feat=32, block="ResBlock"):
    """The resolved option lists of applications/conf/sparseconv3d/<name>.yaml (FEAT = input_nc)."""
    f = in_feat
    if name in ("unet_4", "encoder_4"):
        down = dict(N=[0, 1, 2, 2, 3], down_conv_nn=[[input_nc, f], [f, f], [f, 2 * f], [2 * f, 4 * f], [4 * f, 8 * f]],
                    kernel_size=[3, 3, 3, 3, 3], stride=[1, 2, 2, 2, 2], block=block)
    elif name == "encoder_2":
        down = dict(N=[0, 1, 2], down_conv_nn=[[input_nc, f], [f, f], [f, 2 * f]], kernel_size=[3, 3, 3], stride=[1, 2, 2],
                    block=block)
    elif name == "unet_2":
        down = dict(N=[0, 1, 2], down_conv_nn=[[input_nc, f], [f, f], [f, 2 * f]], kernel_size=[2, 2], stride=[1, 2, 2],
                    block=block)
    else:
        raise ValueError("unknown sparseconv3d configuration %r" % (name,))
    cfg = dict(down_conv=down)
    if name == "unet_4":
        cfg["up_conv"] = dict(N=[1, 1, 1, 1, 0], block=block, kernel_size=[3, 3, 3, 3, 3], stride=[2, 2, 2, 2, 1],
                              up_conv_nn=[[8 * f, 4 * f], [4 * f + 4 * f, 4 * f], [4 * f + 2 * f, 3 * f], [3 * f + f, 3 * f],
                                          [3 * f + f, 3 * f]])
    elif name == "unet_2":
        cfg["up_conv"] = dict(N=[1, 1, 0], block=block, kernel_size=[2, 2, 3], stride=[2, 2, 1],
                              up_conv_nn=[[4 * f + 2 * f, 3 * f], [3 * f + f, 3 * f], [3 * f + f, 3 * f]])
    else:
        width = 8 * f if name == "encoder_4" else 2 * f
        cfg["innermost"] = dict(aggr="mean", nn=[width, width], negative_slope=0.2)
    return cfg


def _stage_options(opts, i):
    return {k: (v[i] if isinstance(v, list) else v) for k, v in opts.items()}


class _BaseSparseConv3d(nn.Module):
    """BaseSparseConv3d of applications/sparseconv3d.py:95-141: the stages, `weight_initialization`, the optional
    `output_nc` head (Linear without bias - BatchNorm1d - ReLU)."""

    def __init__(self, config, input_nc, in_feat=32, block="ResBlock", output_nc=None):
        super().__init__()
        cfg = sparseconv3d_config(config, input_nc, in_feat, block) if isinstance(config, str) else config
        down, up = cfg["down_conv"], cfg.get("up_conv")
        n_down = len(down["down_conv_nn"])
        # a stage list without `N` (conf/models/*/ms_svconv_base.yaml) takes ResNetDown's default of one block per stage;
        # keys that ResNetDown has no use for (module_name, dimension, bn_momentum, ...) end in its **kwargs
        down = dict(down, N=down.get("N", [1] * n_down))
        if up is not None:
            up = dict(up, N=up.get("N", [1] * len(up["up_conv_nn"])))
        def per_layer(opts, key, n):  # a scalar (PointGroup's scorers: `kernel_size: 3`) holds for every layer
            return not isinstance(opts[key], (list, tuple)) or len(opts[key]) == n

        for key in ("N", "kernel_size", "stride"):
            if not per_layer(down, key, n_down) or (up is not None and not per_layer(up, key, len(up["up_conv_nn"]))):
                raise ValueError("sparseconv3d configuration %r: `%s` has not one entry per layer (the reference cannot build "
                                 "this file either)" % (config, key))
        self.down_modules = nn.ModuleList(ResNetDown(**_stage_options(down, i)) for i in range(n_down))
        self.up_modules = nn.ModuleList()
        if up is not None:
            self.up_modules.extend(ResNetUp(**_stage_options(up, i)) for i in range(len(up["up_conv_nn"])))
            default_output_nc = up["up_conv_nn"][-1][-1]
        inner = cfg.get("innermost")
        self.inner_modules = nn.ModuleList()
        if inner is not None:
            aggr = inner.get("aggr", "mean")
            if aggr not in _GLOBAL_AGGR:
                raise NotImplementedError("sparseconv3d innermost: aggr %r is not served (\"mean\" or \"max\")" % (aggr,))
            slope = inner["negative_slope"] if "negative_slope" in inner else inner["activation"]["negative_slope"]
            self.inner_modules.append(_GLOBAL_AGGR[aggr](inner["nn"], slope))
            default_output_nc = inner["nn"][-1]
        self.weight_initialization()
        self._output_nc = default_output_nc
        self._has_mlp_head = output_nc is not None
        if self._has_mlp_head:
            self._output_nc = output_nc
            self.mlp = nn.Sequential(nn.Sequential(nn.Linear(default_output_nc, output_nc, bias=False),
                                                   FastBatchNorm1d(output_nc, momentum=0.1), nn.ReLU()))

    @property
    def has_mlp_head(self):
        return self._has_mlp_head

    @property
    def output_nc(self):
        return self._output_nc

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, Conv3d):
                nn.init.kaiming_normal_(m.kernel, mode="fan_out", nonlinearity="relu")
            if isinstance(m, BatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    @staticmethod
    def _input(data):
        if isinstance(data, SparseTensor):
            return data
        batch = data.batch.unsqueeze(-1) if data.batch.dim() == 1 else data.batch
        return SparseTensor(data.x, torch.cat([data.coords.int(), batch.int()], -1))


class _GlobalMean(nn.Module):
    """GlobalBaseModule(aggr="mean") of core/base_conv/message_passing.py:132-151 without positions: `nn` = Linear - BatchNorm
    - LeakyReLU on every row, then the mean per cloud."""

    def __init__(self, widths, negative_slope):
        super().__init__()
        self.nn = nn.Sequential(*[nn.Sequential(nn.Linear(widths[i - 1], widths[i]), FastBatchNorm1d(widths[i], momentum=0.1),
                                                nn.LeakyReLU(negative_slope)) for i in range(1, len(widths))])

    def forward(self, x, batch, clouds):
        x = self.nn(x)
        out = torch.zeros((clouds, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
        count = torch.zeros((clouds,), dtype=x.dtype, device=x.device).index_add_(0, batch, torch.ones_like(x[:, 0]))
        return out / count.clamp(min=1).unsqueeze(-1)


class _GlobalMax(_GlobalMean):
    """GlobalBaseModule(aggr="max"): the same `nn` on every row, then the maximum per cloud (torchpoints.segment_max).  The
    rows of a strided coordinate set ascend in (batch, x, y, z), so a cloud's rows are consecutive and their offsets come
    from a search in the batch column on the device: no device read.  ordered=False (the rows of an input set, in the
    caller's order): they are first sorted by cloud, stably, on the device.  A cloud without rows gives zeros."""

    def forward(self, x, batch, clouds, ordered=True):
        x = self.nn(x)
        if not ordered:
            batch, perm = torch.sort(batch, stable=True)
            x = x[perm]
        seg = torch.searchsorted(batch.contiguous(), torch.arange(clouds + 1, dtype=batch.dtype, device=batch.device))
        return _tp.segment_max(x, seg)


_GLOBAL_AGGR = {"mean": _GlobalMean, "max": _GlobalMax}


class SparseConv3dUnet(_BaseSparseConv3d):
    """forward: SparseTensor (or an object with x, coords, batch) -> (N, output_nc) features in the input's row order"""

    def __init__(self, config="unet_4", input_nc=3, in_feat=32, block="ResBlock", output_nc=None):
        super().__init__(config, input_nc, in_feat, block, output_nc)

    def forward(self, data):
        data = self._input(data)
        stack_down = []
        for i in range(len(self.down_modules) - 1):
            data = self.down_modules[i](data)
            stack_down.append(data)
        data = self.down_modules[-1](data)
        stack_down.append(None)
        for up in self.up_modules:
            data = up(data, stack_down.pop())
        return self.mlp(data.F) if self.has_mlp_head else data.F


class SparseConv3dEncoder(_BaseSparseConv3d):
    """forward: -> (clouds, output_nc), one row per cloud.  `clouds` (default: largest batch index + 1, one device read;
    given, the forward reads nothing back beyond the one read of every new coordinate set).  A tensor built with
    SparseTensor(clouds=K) brings its K along."""

    def __init__(self, config="encoder_4", input_nc=3, in_feat=32, block="ResBlock", output_nc=None):
        super().__init__(config, input_nc, in_feat, block, output_nc)

    def forward(self, data, clouds=None):
        data = self._input(data)
        s_in = data.s
        for down in self.down_modules:
            data = down(data)
        batch = data.C[:, 3].long()
        if clouds is None:
            clouds = data.clouds if data.clouds is not None else int(batch.max()) + 1
        inner = self.inner_modules[0]
        # (a strided set's rows ascend by cloud; the input set keeps the caller's row order)
        x = inner(data.F, batch, clouds, ordered=data.s != s_in) if isinstance(inner, _GlobalMax) else inner(data.F, batch, clouds)
        return self.mlp(x) if self.has_mlp_head else x
