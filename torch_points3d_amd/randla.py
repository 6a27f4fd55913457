"""RandLA-Net down-convolution on the HIP kNN (BASELINE config 5).

Mirrors torch_points3d/modules/RandLANet/modules.py:9-67 (`RandlaKernel`, `RandlaConv`),
core/base_conv/message_passing.py:35-58 (`BaseConvolutionDown.forward`) and core/spatial_ops/sampling.py:103-112
(`RandomSampler`): same constructor arguments and attribute names (point_pos_nn / attention_nn / global_nn under
`_conv`), same message (relative-position encoding [pos_i, pos_j, pos_i - pos_j, |.|] -> MLP, concatenation with the
neighbour feature, softmax attention over channels, sum over the k neighbours, global MLP).

The reference runs this as a torch_geometric MessagePassing over an edge list built by torch_cluster's `knn`; here the
neighbour table (Nq, k) comes from libtp3d_hip.so's exact grid kNN and, because every query owns exactly k consecutive
edges, the "add" aggregation is a sum over a (Nq, k, C) view -- no scatter.  A table with -1 slots (a cloud smaller
than k) is compacted to its real edges first (`RandlaKernel._forward_ragged`).  Parity: unpinned (torch_cluster absent;
the reference's own model test skips randlanet, test/test_models.py:116-125).

`RandLANetSeg` assembles the two networks of conf/models/segmentation/randlanet.yaml on pointnet2_mp.SegmentationMP.
In eval mode, where no gradient is wanted, the whole per-edge chain of a RandlaKernel can run as one kernel
(csrc/randla_lfa.hip; `RandlaKernel(lfa=...)`, `lfa_route`): DESIGN.md "RandLA-Net: networks and the fused edge pass".
"""
import copy
import math
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import fused as _fused
from . import pointnet2_mp as _mp
from . import torchpoints as _tp
from .kpconv_blocks import PDData
from .partial_dense import MLP, _KnnInterpolate


def relative_position_rows(pos_q, pos_s, nbr):
    """(Nq*k, 12) rows [pos_i, pos_j, pos_i - pos_j, |pos_i - pos_j|, 0, 0] of the edges of a fixed-k table
    (modules.py:36-41); positions carry no gradient."""
    Nq, k = nbr.shape
    dev = pos_q.device
    pq, ps = _tp._f32(pos_q), _tp._f32(pos_s)
    nb = _tp._i64(nbr)
    out = torch.empty((Nq * k, 12), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_randla_relpos_f32", _lib.ptr(pq), _lib.ptr(ps), _lib.ptr(nb), Nq, k, ps.shape[0], _lib.ptr(out),
                  _lib.stream_ptr(dev))
    return out


class _AttentivePool(torch.autograd.Function):
    """out (Nq, C) = sum over the k edges of a query of softmax_c(g[e]) * f[e, :C]   (modules.py:46-52, aggr="add")."""

    @staticmethod
    def forward(ctx, g, f, nbr, C):
        g, f = g.contiguous(), f.contiguous()
        Nq, k = nbr.shape
        dev = g.device
        if g.shape[0] != Nq * k or f.shape[0] != Nq * k or g.shape[1] < C or f.shape[1] < C:
            raise ValueError("attentive_pool: g %s / f %s do not match a (%d, %d) neighbour table with %d channels"
                             % (tuple(g.shape), tuple(f.shape), Nq, k, C))
        out = torch.empty((Nq, C), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.call("tp3d_attn_pool_fwd_f32", _lib.ptr(g), _lib.ptr(f), _lib.ptr(nbr), Nq, k, C, g.shape[1],
                      f.shape[1], _lib.ptr(out), _lib.stream_ptr(dev))
        ctx.save_for_backward(g, f, nbr)
        ctx.C = C
        return out

    @staticmethod
    def backward(ctx, dout):
        g, f, nbr = ctx.saved_tensors
        Nq, k = nbr.shape
        dev = g.device
        dout = dout.float().contiguous()
        dg = torch.empty_like(g) if g.shape[1] == ctx.C else torch.zeros_like(g)
        df = torch.empty_like(f)
        with _lib.on_device(dev):
            _lib.call("tp3d_attn_pool_bwd_f32", _lib.ptr(g), _lib.ptr(f), _lib.ptr(dout), _lib.ptr(nbr), Nq, k, ctx.C,
                      g.shape[1], f.shape[1], _lib.ptr(dg), _lib.ptr(df), _lib.stream_ptr(dev))
        return dg, df, None, None


def attentive_pool(g, f, nbr, C):
    return _AttentivePool.apply(g, f, nbr, C)


LFA_K, LFA_CMAX, LFA_AMAX = 16, 64, 128  # csrc/randla_lfa.hip: neighbours per query, C / P1 / P2, A1

# Width classes of the one-kernel eval pass (by C = Cx + P2) and whether the recorded fused time is not above the
# recorded rows time (profiles/randla_bench.json, tools/bench_randla.py: the three levels of Randlanet_Conv on a
# 10^6-point scene, fused / rows 0.578 / 0.732, 0.374 / 0.909, 0.417 / 0.514 ms).  A class that lost or was not
# measured routes to rows.
LFA_MEASURED_WIN = {16: True, 32: True, 64: True}


def _widths(mlp):
    """channel list of an MLP: the list itself, or [in, out, out, ...] of the Linear layers of an `MLP` module"""
    if isinstance(mlp, (list, tuple)):
        return [int(c) for c in mlp]
    lins = [m for m in mlp.modules() if isinstance(m, nn.Linear)]
    return [lins[0].in_features] + [m.out_features for m in lins]


def lfa_width_class(C):
    for top in sorted(LFA_MEASURED_WIN):
        if C <= top:
            return top
    return None


def lfa_route(k, Cx, point_pos_nn, attention_nn, holes, training, device):
    """"fused" (csrc/randla_lfa.hip, tp3d_randla_lfa_eval_f32) or "rows" (the row kernels between rows_mlp calls) for
    one RandlaKernel forward.  Pure: k neighbours per query, Cx feature columns of the support (3 when x is None),
    the two MLPs as channel lists or `MLP` modules, whether the table has -1 slots, the module's training flag, the
    device of the tensors.  The kernel serves k = 16, two-layer MLPs, C = Cx + P2 <= 64, P1, P2 <= 64, A1 <= 128, eval
    mode, a full table, on the GPU -- and of those only the width classes that LFA_MEASURED_WIN records as no slower."""
    if training or holes or torch.device(device).type != "cuda":
        return "rows"
    pp, at = _widths(point_pos_nn), _widths(attention_nn)
    if k != LFA_K or len(pp) != 3 or len(at) != 3 or pp[0] != 10:
        return "rows"
    P1, P2, A1 = pp[1], pp[2], at[1]
    C = Cx + P2
    if at[0] != C or at[2] != C:
        return "rows"
    if C > LFA_CMAX or P1 > LFA_CMAX or P2 > LFA_CMAX or A1 > LFA_AMAX:
        return "rows"
    return "fused" if LFA_MEASURED_WIN.get(lfa_width_class(C), False) else "rows"


def _fold_layer(layer):
    """[Linear, FastBatchNorm1d, LeakyReLU(0.2)] in eval mode -> W, s = gamma / sqrt(var + eps), t = beta + s (b - mean)"""
    lin, bn = layer[0], layer[1].batch_norm
    s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    b = lin.bias if lin.bias is not None else torch.zeros_like(bn.running_mean)
    return [lin.weight.reshape(-1), s, bn.bias + s * (b - bn.running_mean)]


def _lfa_servable(mlp):
    """what the folding assumes of an MLP's layers, beyond the widths lfa_route reads"""
    for layer in mlp:
        if not (len(layer) == 3 and isinstance(layer[0], nn.Linear) and hasattr(layer[1], "batch_norm")
                and isinstance(layer[2], nn.LeakyReLU) and layer[2].negative_slope == 0.2
                and layer[1].batch_norm.affine and layer[1].batch_norm.track_running_stats):
            return False
    return True


_LFA_CONSTS = weakref.WeakKeyDictionary()  # point_pos_nn module -> (fused.eval_state_key of both MLPs, folded constants)


def _lfa_consts(point_pos_nn, attention_nn):
    """the folded constants of the two MLPs as one dense buffer, per layer W, s, t (include/tp3d_hip.h); kept until a
    parameter or buffer is written (its version counter moves), moved (its address changes), or may have been written
    behind the version counters: a training pass of one of the four BatchNorms (the HIP BatchNorm kernels update the
    running statistics through raw pointers) or a replayed captured step (fused.eval_state_key)"""
    tensors = [t for mlp in (point_pos_nn, attention_nn) for layer in mlp
               for t in (layer[0].weight, layer[0].bias, layer[1].batch_norm.weight, layer[1].batch_norm.bias,
                         layer[1].batch_norm.running_mean, layer[1].batch_norm.running_var) if t is not None]
    key = _fused.eval_state_key(tensors, [layer[1].batch_norm for mlp in (point_pos_nn, attention_nn) for layer in mlp])
    hit = _LFA_CONSTS.get(point_pos_nn)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        consts = torch.cat([t.detach().float() for mlp in (point_pos_nn, attention_nn) for layer in mlp
                            for t in _fold_layer(layer)])
    _LFA_CONSTS[point_pos_nn] = (key, consts)
    return consts


def randla_lfa_eval(pos_q, pos_s, x, nbr, point_pos_nn, attention_nn):
    """(Nq, C) = sum over a query's 16 edges, in slot order, of softmax_c(attention_nn(f)) * f, f = [x_j | point_pos_nn(
    relative position)], both MLPs in eval mode: one HIP kernel, no per-edge tensor.  No gradient."""
    dev = pos_s.device
    pq, ps = _tp._f32(pos_q), _tp._f32(pos_s)
    nb = _tp._i64(nbr)
    Nq, k = nb.shape
    xs = None if x is None else x.detach().float().contiguous()
    Cx = 3 if xs is None else xs.shape[1]
    consts = _lfa_consts(point_pos_nn, attention_nn)
    pp, at = _widths(point_pos_nn), _widths(attention_nn)
    out = torch.empty((Nq, Cx + pp[2]), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_randla_lfa_eval_f32", _lib.ptr(pq), _lib.ptr(ps), _lib.ptr(xs), _lib.ptr(nb), Nq, ps.shape[0], k,
                  Cx, pp[1], pp[2], at[1], _lib.ptr(consts), _lib.ptr(out), _lib.stream_ptr(dev))
    return out


class RandomSampler(object):
    """floor(N * ratio) (or num_to_sample) indices drawn uniformly WITH replacement (sampling.py:109-111).
    sort=True hands the same draw out in ascending order -- the same multiset of rows, permuted -- so that `batch[idx]`
    of a sorted batch vector stays sorted (what the kNN requires of a multi-cloud batch)."""

    def __init__(self, ratio=None, num_to_sample=None, sort=False):
        self._sort = bool(sort)
        if num_to_sample is not None:
            if ratio is not None:
                raise ValueError("Can only specify ratio or num_to_sample or subsampling_param, not several !")
            self._num_to_sample = num_to_sample
        elif ratio is not None:
            self._ratio = ratio
        else:
            raise Exception('At least ["ratio, num_to_sample, subsampling_param"] should be defined')

    def _get_num_to_sample(self, n):
        return self._num_to_sample if hasattr(self, "_num_to_sample") else math.floor(n * self._ratio)

    def sample(self, pos, batch=None, **kwargs):
        if len(pos.shape) != 2:
            raise ValueError(" This class is for sparse data and expects the pos tensor to be of dimension 2")
        idx = torch.randint(0, pos.shape[0], (self._get_num_to_sample(pos.shape[0]),), device=pos.device)
        return torch.sort(idx)[0] if self._sort else idx

    def __call__(self, pos, x=None, batch=None):
        return self.sample(pos, batch=batch, x=x)


class RandlaKernel(nn.Module):
    """Local spatial encoding + attentive pooling over a fixed-k neighbour table."""

    def __init__(self, point_pos_nn=None, attention_nn=None, global_nn=None, *args, **kwargs):
        super().__init__()
        self.point_pos_nn = MLP(point_pos_nn)
        self.attention_nn = MLP(attention_nn)
        self.global_nn = MLP(global_nn)
        self.fused = kwargs.get("fused", True)
        self.lfa = kwargs.get("lfa", "rows")
        if self.lfa not in ("auto", "fused", "rows"):
            raise ValueError("lfa must be 'auto', 'fused' or 'rows', not %r" % (self.lfa,))

    def _lfa_route(self, x, pos_s, nbr, holes):
        """the route of this forward: lfa_route's answer, and "rows" as well wherever a gradient is wanted (the
        one-kernel pass has no backward) or a layer is not the [Linear, BatchNorm, LeakyReLU(0.2)] the folding assumes"""
        Cx = 3 if x is None else x.shape[1]
        route = lfa_route(nbr.shape[1], Cx, self.point_pos_nn, self.attention_nn, holes, self.training, pos_s.device)
        if route == "fused":
            wants_grad = torch.is_grad_enabled() and (
                (x is not None and x.requires_grad) or any(p.requires_grad for p in self.point_pos_nn.parameters())
                or any(p.requires_grad for p in self.attention_nn.parameters()))
            if wants_grad or not (_lfa_servable(self.point_pos_nn) and _lfa_servable(self.attention_nn)):
                route = "rows"
        return route

    def forward(self, x, pos, nbr):
        """x (M,C) or None, pos = (query positions (Nq,3), support positions (M,3)), nbr (Nq,k) rows of the support;
        -1 slots (a cloud with fewer than k points) are edges that do not exist"""
        pos_q, pos_s = pos
        Nq, k = nbr.shape
        holes = bool((nbr < 0).any())  # one host read per forward
        if self.lfa != "rows":
            route = self._lfa_route(x, pos_s, nbr, holes)
            if route == "fused":
                return _fused.rows_mlp(self.global_nn, randla_lfa_eval(pos_q, pos_s, x, nbr, self.point_pos_nn,
                                                                       self.attention_nn))
            if self.lfa == "fused":
                raise ValueError("RandlaKernel(lfa='fused'): the one-kernel pass serves eval mode without gradients, a "
                                 "full (Nq, 16) table on the GPU and the widths lfa_route accepts")
        if holes:
            return self._forward_ragged(x, pos_q, pos_s, nbr)
        if pos_s.is_cuda and self.fused:
            return self._forward_fused(x, pos_q, pos_s, nbr)
        j = nbr.reshape(-1)
        pos_i = pos_q.repeat_interleave(k, dim=0)
        pos_j = pos_s[j]
        x_j = pos_j if x is None else x[j]
        vij = pos_i - pos_j
        dij = torch.norm(vij, dim=1).unsqueeze(1)
        rij = _fused.rows_mlp(self.point_pos_nn, torch.cat([pos_i, pos_j, vij, dij], dim=1))
        fij_hat = torch.cat([x_j, rij], dim=1)
        s_ij = F.softmax(_fused.rows_mlp(self.attention_nn, fij_hat), -1)
        msg = s_ij * fij_hat
        return _fused.rows_mlp(self.global_nn, msg.reshape(Nq, k, -1).sum(dim=1))

    def _forward_ragged(self, x, pos_q, pos_s, nbr):
        """A table with -1 slots: the edge rows are compacted to the real edges first -- the reference's kNN edge list,
        so the BatchNorms of the edge-wise MLPs see what they see there -- and the messages go back into a zero
        (Nq*k, C) buffer, summed per query in slot order (one writer per row: deterministic)."""
        Nq, k = nbr.shape
        flat = _tp._i64(nbr).reshape(-1)
        real = torch.nonzero(flat >= 0).reshape(-1)
        j = flat[real]
        pos_i = pos_q[torch.div(real, k, rounding_mode="floor")]
        if pos_s.is_cuda and self.fused:
            edges = j.reshape(-1, 1)  # every real edge as a query of its own with one neighbour
            rij = _fused.rows_mlp(self.point_pos_nn, relative_position_rows(pos_i, pos_s, edges))
            xs = _tp._f32(pos_s) if x is None else x
            C = xs.shape[1] + rij.shape[1]
            ones = torch.ones((edges.shape[0], 1), dtype=torch.float32, device=nbr.device)
            fij_hat = _KnnInterpolate.apply(xs, rij, edges, ones, (C + 3) // 4 * 4)
            msg = F.softmax(_fused.rows_mlp(self.attention_nn, fij_hat), -1) * fij_hat[:, :C]
        else:
            pos_j = pos_s[j]
            x_j = pos_j if x is None else x[j]
            vij = pos_i - pos_j
            dij = torch.norm(vij, dim=1).unsqueeze(1)
            rij = _fused.rows_mlp(self.point_pos_nn, torch.cat([pos_i, pos_j, vij, dij], dim=1))
            fij_hat = torch.cat([x_j, rij], dim=1)
            msg = F.softmax(_fused.rows_mlp(self.attention_nn, fij_hat), -1) * fij_hat
        rows = msg.new_zeros((Nq * k, msg.shape[1])).index_copy(0, real, msg)
        return _fused.rows_mlp(self.global_nn, rows.reshape(Nq, k, -1).sum(dim=1))

    def _forward_fused(self, x, pos_q, pos_s, nbr):
        """Same arithmetic; the edge-wise pieces between the MLPs are HIP row kernels (csrc/randla.hip) and the
        neighbour-feature gather + concatenation is the k = 1 case of the interpolation kernel (weight exactly 1),
        whose backward is the atomic-free inverse-index gather."""
        Nq, k = nbr.shape
        nbr = _tp._i64(nbr)
        rij = _fused.rows_mlp(self.point_pos_nn, relative_position_rows(pos_q, pos_s, nbr))
        xs = _tp._f32(pos_s) if x is None else x
        C = xs.shape[1] + rij.shape[1]
        edges = nbr.reshape(-1, 1)
        ones = torch.ones((edges.shape[0], 1), dtype=torch.float32, device=nbr.device)
        fij_hat = _KnnInterpolate.apply(xs, rij, edges, ones, (C + 3) // 4 * 4)  # (Nq*k, pad4(C)) = [x_j | rij | 0]
        g_fij = _fused.rows_mlp(self.attention_nn, fij_hat)
        return _fused.rows_mlp(self.global_nn, attentive_pool(g_fij, fij_hat, nbr, C))


class RandlaConv(nn.Module):
    def __init__(self, ratio=None, k=None, *args, **kwargs):
        super().__init__()
        self.sampler = RandomSampler(ratio, sort=bool(kwargs.get("sort", False)))
        self.k = k
        self.edge_list = bool(kwargs.get("edge_list", False))
        if kwargs.get("index") == 0 and kwargs.get("nb_feature") is not None:
            kwargs["point_pos_nn"][-1] = kwargs.get("nb_feature")
            kwargs["attention_nn"][0] = kwargs["attention_nn"][-1] = kwargs.get("nb_feature") * 2
            kwargs["down_conv_nn"][0] = kwargs.get("nb_feature") * 2
        self._conv = RandlaKernel(point_pos_nn=kwargs["point_pos_nn"], attention_nn=kwargs["attention_nn"],
                                  global_nn=kwargs["down_conv_nn"], fused=kwargs.get("fused", True),
                                  lfa=kwargs.get("lfa", "rows"))

    def forward(self, data, **kwargs):
        x, pos, batch = data.x, data.pos, data.batch
        idx = self.sampler(pos, batch=batch)
        q_pos, q_batch = pos[idx], batch[idx]
        nbr, _ = _tp.knn(self.k, pos, q_pos, batch, q_batch)  # exact kNN of every sampled point in its own cloud
        out = data.shallow_copy() if hasattr(data, "shallow_copy") else PDData(**vars(data))
        out.idx = idx
        out.neighbors = nbr
        if self.edge_list:
            # the reference's edge list (message_passing.py:49-52: edge_index = stack([col, row])): query-major, each
            # query's neighbours closest first -- row 0 = support index, row 1 = query index
            row = torch.arange(nbr.shape[0], device=nbr.device).repeat_interleave(self.k)
            col = nbr.reshape(-1)
            keep = col >= 0
            out.edge_index = torch.stack([col[keep], row[keep]], dim=0)
        out.x = self._conv(x, (q_pos, pos), nbr)
        out.pos = q_pos
        out.batch = q_batch
        return out


class DilatedResidualBlock(nn.Module):
    """Two RandlaConv in sequence inside a residual frame (modules/RandLANet/modules.py:70-102 on
    core/base_conv/message_passing.py:212-255 `BaseResnetBlock`): the shortcut rows are gathered with the LAST
    convolution's sample indices, resized by `shortcut_feature_resize_nn` and added to the up-sampled convolution output.
    As in the reference, `features_downsample_nn` is evaluated on the input (its BatchNorm statistics move in training
    mode) but its result is not what the convolutions consume -- they read `data.x` -- and `activation` is unused."""

    def __init__(self, indim, outdim, ratio1, ratio2, point_pos_nn1, point_pos_nn2, attention_nn1, attention_nn2,
                 global_nn1, global_nn2, *args, **kwargs):
        super().__init__()
        if kwargs.get("index") == 0 and kwargs.get("nb_feature") is not None:
            indim = kwargs.get("nb_feature")
        self.indim, self.outdim, self.convdim = indim, outdim, outdim
        self.features_downsample_nn = MLP([indim, outdim // 4])
        self.features_upsample_nn = MLP([outdim, outdim])
        self.shortcut_feature_resize_nn = MLP([indim, outdim])
        self.activation = nn.ReLU()
        kw = dict(kwargs)
        self.conv1 = RandlaConv(ratio1, 16, point_pos_nn=point_pos_nn1, attention_nn=attention_nn1,
                                down_conv_nn=global_nn1, **kw)
        kw["nb_feature"] = None
        self.conv2 = RandlaConv(ratio2, 16, point_pos_nn=point_pos_nn2, attention_nn=attention_nn2,
                                down_conv_nn=global_nn2, **kw)

    def convs(self, data):
        return self.conv2(self.conv1(data))

    def forward(self, data, **kwargs):
        shortcut = data.x
        _fused.rows_mlp(self.features_downsample_nn, data.x)  # evaluated, not consumed (see the class note)
        out = self.convs(data)
        x = _fused.rows_mlp(self.features_upsample_nn, out.x)
        if out.idx is not None:
            shortcut = shortcut[out.idx]
        out.x = _fused.rows_mlp(self.shortcut_feature_resize_nn, shortcut) + x
        return out


class RandLANetRes(nn.Module):
    """conf/models/segmentation/randlanet.yaml `Randlanet_Res` down module: lists of two entries per argument"""

    def __init__(self, indim, outdim, ratio, point_pos_nn, attention_nn, down_conv_nn, *args, **kwargs):
        super().__init__()
        self._conv = DilatedResidualBlock(indim, outdim, ratio[0], ratio[1], point_pos_nn[0], point_pos_nn[1],
                                          attention_nn[0], attention_nn[1], down_conv_nn[0], down_conv_nn[1], *args, **kwargs)

    def forward(self, data):
        return self._conv(data)


def randla_config(name, feat):
    """conf/models/segmentation/randlanet.yaml resolved for FEAT (the innermost width is the YAML's 128 + 3 = 131)."""
    common = dict(innermost=dict(aggr="max", nn=[128 + 3, 128]), mlp_cls=dict(nn=[64, 64, 64, 64, 64], dropout=0.5))
    if name == "Randlanet_Conv":
        return dict(
            down_conv=dict(module_name="RandlaConv", ratio=[0.25, 0.25, 0.25], k=[16, 16, 16],
                           point_pos_nn=[[10, 8, feat], [10, 8, 16], [10, 16, 32]],
                           attention_nn=[[2 * feat, 8, 2 * feat], [32, 64, 32], [64, 128, 64]],
                           down_conv_nn=[[2 * feat, 8, 16], [32, 64, 32], [64, 128, 128]]),
            up_conv=dict(up_conv_nn=[[128 + 128, 128], [128 + 32, 64], [64 + 16, 64], [64 + feat, 64]],
                         up_k=[1, 1, 1, 1], skip=True), **common)
    if name == "Randlanet_Res":
        return dict(
            down_conv=dict(module_name="RandLANetRes", ratio=[[1, 1], [0.5, 0.5]], indim=[3, 32], outdim=[32, 128],
                           point_pos_nn=[[[10, 8, feat], [10, 16, 16]], [[10, 16, 32], [10, 32, 64]]],
                           attention_nn=[[[2 * feat, 8, 2 * feat], [32, 64, 32]], [[64, 128, 64], [128, 256, 128]]],
                           down_conv_nn=[[[2 * feat, 8, 16], [32, 64, 32]], [[64, 64, 64], [128, 128, 128]]]),
            up_conv=dict(up_conv_nn=[[128 + 128, 128], [128 + 32, 64], [64 + feat, 64]], up_k=[1, 1, 1], skip=True),
            **common)
    raise ValueError("unknown RandLA-Net config %r" % name)


class RandLANetSeg(_mp.SegmentationMP):
    """RandLANetSeg (models/segmentation/randlanet.py on Segmentation_MP): SegmentationMP over RandlaConv
    (`Randlanet_Conv`) or RandLANetRes (`Randlanet_Res`) down modules, GlobalBaseModule innermost, FPModule(up_k = 1) up.

    cfg: a config name of randla_config or a dict with the YAML's fields; data.x is (N, input_nc), data.batch sorted.
    The samplers sort their draw (RandomSampler(sort=True)): every level's batch vector stays sorted, so a batch may
    hold several clouds.  lfa: the edge-pass route of every RandlaKernel ("auto": one kernel in eval mode where
    lfa_route serves the widths, the row kernels otherwise)."""

    def __init__(self, cfg, input_nc, num_classes, lfa="auto"):
        if isinstance(cfg, str):
            cfg = randla_config(cfg, input_nc)
        down = copy.deepcopy(cfg["down_conv"])  # RandlaConv writes nb_feature into its level-0 lists
        residual = down.get("module_name", "RandlaConv") == "RandLANetRes"

        def make_down(i):
            kw = dict(point_pos_nn=down["point_pos_nn"][i], attention_nn=down["attention_nn"][i],
                      down_conv_nn=down["down_conv_nn"][i], index=i, nb_feature=input_nc, sort=True, lfa=lfa)
            if residual:
                return RandLANetRes(down["indim"][i], down["outdim"][i], down["ratio"][i], **kw)
            return RandlaConv(down["ratio"][i], down["k"][i], **kw)

        super().__init__(cfg, num_classes, make_down)
