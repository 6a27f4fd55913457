"""Plain-torch restatement of the sparse voxel convolution family ("Sparse voxel convolution").

Coordinate sets come from torch.unique on floored coordinates; every convolution scatters its input to a dense
[B, C, X, Y, Z] grid, runs F.conv3d / F.conv_transpose3d and reads the result at the output set:

    k = 3, stride 1      F.conv3d(stride=1, padding=1)
    k = 3, stride 2      F.conv3d(stride=2, padding=1)
    k = 2, stride 2      F.conv3d(stride=2, padding=0)
    k = 2, stride 1      F.conv3d(stride=1, padding=0) over the grid with one more zero cell on the high side
    k = 1, stride 2      F.conv3d(stride=2, padding=0)
    transposed k = 3, 2  F.conv_transpose3d(stride=2, padding=1, output_padding=1)
    transposed k = 2, 2  F.conv_transpose3d(stride=2, padding=0)
    transposed k = 1, 2  F.conv_transpose3d(stride=2, padding=0, output_padding=1)
    transposed k = 3, 1  F.conv_transpose3d(stride=1, padding=1)
    transposed k = 2, 1  F.conv_transpose3d(stride=1, padding=0) (one cell longer on the high side; never read)

`lookup` / `kernel_map` compare rows, not packed keys, so they are exact over the whole accepted range (|x|, |y|, |z| <=
2^18, 0 <= batch < 2^9 is 66 bits); `conv_by_table` is the same sum over such a table, for clouds too wide for a grid.

Works in fp32 and float64 (the dtype of the features and weights) on any device.  The blocks and networks below restate
modules/SparseConv3d/modules.py and applications/sparseconv3d.py with the reference's attribute names.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def down_coords(C, ts2):
    """distinct floor(c / ts2) * ts2 per axis, batch kept, ascending (batch, x, y, z)"""
    c = C.long()
    fl = torch.div(c[:, :3], ts2, rounding_mode="floor") * ts2
    u = torch.unique(torch.cat([c[:, 3:4], fl], 1), dim=0)  # lexicographic rows: (batch, x, y, z)
    return torch.cat([u[:, 1:], u[:, :1]], 1).int()


def offsets(ksize, ts):
    r = [-1, 0, 1] if ksize == 3 else ([0, 1] if ksize == 2 else [0])
    return [(a * ts, b * ts, c * ts) for a in r for b in r for c in r]  # x slowest, z fastest


def _row_ids(rows):
    """one int64 per (x, y, z, batch) row, equal exactly where the rows are equal: a mixed-radix key over the rows' own
    bounding box where that fits 62 bits, else the row's rank among the distinct rows"""
    lo = rows.min(0).values
    ext = rows.max(0).values - lo + 1
    if float(ext.double().prod()) < 2.0 ** 62:
        d = rows - lo
        return ((d[:, 3] * ext[0] + d[:, 0]) * ext[1] + d[:, 1]) * ext[2] + d[:, 2]
    return torch.unique(rows, dim=0, return_inverse=True)[1]


def lookup(Cq, off, Cs):
    """row of Cs at Cq + off, -1 where absent"""
    q = Cq.long().clone()
    q[:, :3] += torch.tensor(off, device=q.device)
    ids = _row_ids(torch.cat([Cs.long(), q], 0))
    ks, order = torch.sort(ids[:len(Cs)])
    kq = ids[len(Cs):]
    pos = torch.searchsorted(ks, kq).clamp(max=ks.numel() - 1)
    return torch.where(ks[pos] == kq, order[pos], torch.full_like(pos, -1))


def kernel_map(C_in, C_out, ksize, ts):
    """(forward (Nout, K), inverse (Nin, K)) int32: in(o, k) and out(i, k)"""
    offs = offsets(ksize, ts)
    fwd = torch.stack([lookup(C_out, o, C_in) for o in offs], 1)
    inv = torch.stack([lookup(C_in, tuple(-v for v in o), C_out) for o in offs], 1)
    return fwd.int(), inv.int()


def _dense(Fx, C, ts, origin, shape, B):
    g = torch.zeros((B, Fx.shape[1]) + tuple(shape), dtype=Fx.dtype, device=Fx.device)
    c = C.long()
    i = (c[:, :3] - origin) // ts
    g[c[:, 3], :, i[:, 0], i[:, 1], i[:, 2]] = Fx
    return g


def _read(g, C, ts, origin):
    c = C.long()
    i = (c[:, :3] - origin) // ts
    return g[c[:, 3], :, i[:, 0], i[:, 1], i[:, 2]]


def conv(Fx, C_in, C_out, W, ksize, stride, ts, transposed=False):
    """Fx on the rows of its own set; ts = tensor stride of the FINE set (the input of a forward, the output of a
    transposed convolution).  W (k^3, Cin, Cout) or (Cin, Cout)."""
    if ksize == 1 and stride == 1:
        return Fx @ W.reshape(Fx.shape[1], -1)
    cin, cout = W.shape[-2], W.shape[-1]
    Wd = W.reshape(ksize, ksize, ksize, cin, cout)
    fine, coarse = (C_out, C_in) if transposed else (C_in, C_out)
    both = torch.cat([fine.long(), coarse.long()], 0)
    B = int(both[:, 3].max()) + 1
    cs = ts * stride
    origin = torch.div(both[:, :3].min(0).values, cs, rounding_mode="floor") * cs  # a multiple of the coarse stride
    n_coarse = (both[:, :3].max(0).values - origin) // cs + 1
    n_fine = n_coarse * stride
    if not transposed:
        g = _dense(Fx, C_in, ts, origin, n_fine.tolist(), B)
        if ksize == 2 and stride == 1:
            g = F.pad(g, (0, 1, 0, 1, 0, 1))  # offsets {0, 1}: the last cell of every axis reads one past the grid
        out = F.conv3d(g, Wd.permute(4, 3, 0, 1, 2), stride=stride, padding=1 if ksize == 3 else 0)
        return _read(out, C_out, cs, origin)
    g = _dense(Fx, C_in, cs, origin, n_coarse.tolist(), B)
    pad = 1 if ksize == 3 else 0  # (k = 2, stride 2: rows 2j and 2j + 1, no padding on either side)
    # the fine grid has stride * n_coarse cells per axis: (n - 1) stride - 2 pad + k + output_padding
    opad = stride + 2 * pad - ksize if stride > 1 else 0
    out = F.conv_transpose3d(g, Wd.permute(3, 4, 0, 1, 2), stride=stride, padding=pad, output_padding=opad)
    return _read(out, C_out, ts, origin)


def conv_by_table(Fx, table, W):
    """y[r] = sum_k Fx[table[r, k]] @ W[k] over the entries >= 0, in the dtype of Fx and W; differentiable.  With
    kernel_map's forward table this is the forward convolution, with the inverse table the transposed one."""
    K = table.shape[1]
    W = W.reshape(K, Fx.shape[1], -1)
    y = torch.zeros((table.shape[0], W.shape[2]), dtype=Fx.dtype, device=Fx.device)
    for k in range(K):
        hit = torch.nonzero(table[:, k] >= 0).squeeze(1)
        if hit.numel():
            y = y.index_add(0, hit, Fx[table[hit, k].long()] @ W[k])
    return y


# ------------------------------------------------------------------------------------------------ modules and networks
class RefTensor(object):
    def __init__(self, Fx, C, s=1, sets=None):
        self.F, self.C, self.s = Fx, C, s
        self.sets = {s: C} if sets is None else sets

    def like(self, Fx):
        return RefTensor(Fx, self.C, self.s, self.sets)


class Conv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transposed=False):
        super().__init__()
        self.k, self.stride, self.transposed = kernel_size, stride, transposed
        shape = (kernel_size ** 3, in_channels, out_channels) if kernel_size > 1 else (in_channels, out_channels)
        self.kernel = nn.Parameter(torch.zeros(shape))

    def forward(self, x):
        if self.k == 1 or self.stride == 1:
            return x.like(conv(x.F, x.C, x.C, self.kernel, self.k, 1, x.s, self.transposed))
        if not self.transposed:
            s2 = x.s * self.stride
            if s2 not in x.sets:
                x.sets[s2] = down_coords(x.C, s2).to(x.C.device)
            return RefTensor(conv(x.F, x.C, x.sets[s2], self.kernel, self.k, self.stride, x.s), x.sets[s2], s2, x.sets)
        fine = x.s // self.stride
        return RefTensor(conv(x.F, x.C, x.sets[fine], self.kernel, self.k, self.stride, fine, True), x.sets[fine], fine, x.sets)


class Conv3dTranspose(Conv3d):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transpose=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, transposed=True)


class BatchNorm(nn.Module):
    def __init__(self, num_features, *, eps=1e-5, momentum=0.1):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum)

    def forward(self, x):
        return x.like(self.bn(x.F))


class ReLU(nn.Module):
    def forward(self, x):
        return x.like(torch.relu(x.F))


def cat(*args):
    return args[0].like(torch.cat([a.F for a in args], 1))


def _seq(*mods):
    s = nn.Sequential()
    for i, m in enumerate(mods):
        s.add_module(str(i), m)
    return s


class ResBlock(nn.Module):
    def __init__(self, input_nc, output_nc, convolution):
        super().__init__()
        self.block = _seq(convolution(input_nc, output_nc, kernel_size=3, stride=1), BatchNorm(output_nc), ReLU(),
                          convolution(output_nc, output_nc, kernel_size=3, stride=1), BatchNorm(output_nc), ReLU())
        self.downsample = None
        if input_nc != output_nc:
            self.downsample = _seq(Conv3d(input_nc, output_nc, kernel_size=1, stride=1), BatchNorm(output_nc))

    def forward(self, x):
        out = self.block(x)
        return out.like(out.F + (self.downsample(x).F if self.downsample is not None else x.F))


class BottleneckBlock(nn.Module):
    def __init__(self, input_nc, output_nc, convolution, reduction=4):
        super().__init__()
        m = output_nc // reduction
        self.block = _seq(Conv3d(input_nc, m, kernel_size=1, stride=1), BatchNorm(m), ReLU(),
                          convolution(m, m, kernel_size=3, stride=1), BatchNorm(m), ReLU(),
                          Conv3d(m, output_nc, kernel_size=1), BatchNorm(output_nc), ReLU())
        self.downsample = None
        if input_nc != output_nc:
            self.downsample = _seq(convolution(input_nc, output_nc, kernel_size=1, stride=1), BatchNorm(output_nc))

    def forward(self, x):
        out = self.block(x)
        return out.like(out.F + (self.downsample(x).F if self.downsample is not None else x.F))


class ResNetDown(nn.Module):
    CONVOLUTION = Conv3d

    def __init__(self, down_conv_nn, kernel_size=2, dilation=1, stride=2, N=1, block="ResBlock"):
        super().__init__()
        blk = {"ResBlock": ResBlock, "BottleneckBlock": BottleneckBlock}[block]
        w = down_conv_nn[0] if stride > 1 else down_conv_nn[1]
        conv_ = self.CONVOLUTION
        self.conv_in = _seq(conv_(down_conv_nn[0], w, kernel_size=kernel_size, stride=stride), BatchNorm(w), ReLU())
        self.blocks = None
        if N > 0:
            mods = []
            for _ in range(N):
                mods.append(blk(w, down_conv_nn[1], conv_))
                w = down_conv_nn[1]
            self.blocks = _seq(*mods)

    def forward(self, x, skip=None):
        if skip is not None:
            x = cat(x, skip)
        out = self.conv_in(x)
        return self.blocks(out) if self.blocks is not None else out


class ResNetUp(ResNetDown):
    CONVOLUTION = Conv3dTranspose


class Net(nn.Module):
    """the U-Net (cfg with `up_conv`) or the encoder (cfg with `innermost`) from the resolved option lists"""

    def __init__(self, cfg):
        super().__init__()
        d = cfg["down_conv"]
        self.down_modules = nn.ModuleList(
            ResNetDown(d["down_conv_nn"][i], d["kernel_size"][i], 1, d["stride"][i], d["N"][i], d["block"])
            for i in range(len(d["down_conv_nn"])))
        self.up_modules = nn.ModuleList()
        u = cfg.get("up_conv")
        if u is not None:
            self.up_modules.extend(ResNetUp(u["up_conv_nn"][i], u["kernel_size"][i], 1, u["stride"][i], u["N"][i], u["block"])
                                   for i in range(len(u["up_conv_nn"])))
        self.inner_modules = nn.ModuleList()
        inner = cfg.get("innermost")
        if inner is not None:
            w = inner["nn"]
            head = nn.Module()
            lin = nn.Sequential(nn.Linear(w[0], w[1]), nn.Module(), nn.LeakyReLU(inner["negative_slope"]))
            lin[1].batch_norm = nn.BatchNorm1d(w[1], momentum=0.1)
            head.nn = nn.Sequential(lin)
            self.inner_modules.append(head)

    def forward(self, Fx, C):
        x = RefTensor(Fx, C)
        stack = []
        for m in self.down_modules[:-1]:
            x = m(x)
            stack.append(x)
        x = self.down_modules[-1](x)
        stack.append(None)
        for m in self.up_modules:
            x = m(x, stack.pop())
        if len(self.inner_modules):
            lin = self.inner_modules[0].nn[0]
            h = lin[2](lin[1].batch_norm(lin[0](x.F)))
            b = x.C[:, 3].long()
            n = int(b.max()) + 1
            s = torch.zeros((n, h.shape[1]), dtype=h.dtype, device=h.device).index_add_(0, b, h)
            c = torch.zeros((n,), dtype=h.dtype, device=h.device).index_add_(0, b, torch.ones_like(h[:, 0]))
            return s / c.unsqueeze(-1)
        return x.F
