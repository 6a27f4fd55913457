"""PosPool / PPNet ("A Closer Look at Local Aggregation Operators in Point Cloud Analysis") on MI355X.

Mirrors torch_points3d/modules/PPNet/ops.py (`PosPoolLayer`), modules/PPNet/blocks.py (`SimpleBlock`,
`SimpleInputBlock`, `ResnetBBlock`, `PPStageBlock`) and the network models/segmentation/ppnet.py assembles from
conf/models/segmentation/ppnet.yaml (`PPNet`, `PPNetxyz`): same constructor arguments, attribute names (hence
state_dict keys) and defaults -- LeakyReLU(0.2), BatchNorm momentum 0.02 in the layer and 0.01 in the blocks, search
radius 2.5 * sigma * prev_grid_size, bottleneck_ratio 2, `unary_2` and `shortcut_op` without activation.

The aggregation itself -- a parameter-free gather that multiplies every neighbour's feature row by a geometric prior of
its relative position and reduces over the neighbours -- is one HIP kernel per direction (csrc/pospool.hip); the
backward pass sums per support point through the inverted neighbour table shared with the KPConv kernels (csrc/inverse_table.hip; no atomics).
Differentiable wrt `features`; positions carry no gradient.  Everything around it is shared with kpconv_blocks.py: the
radius search, `GridSampling3D`, the strided shortcut (`fused.nbr_maxpool`), `fused.bn_act` / `fused.rows_seq` behind
the same `fused=` switch and the `precomputed=` path.

`avg` divides by n_q + 1e-5 with the reference's own count rule (ops.py:107-108): n_q is the number of slots of row q
whose index is below the largest index of the table AFTER its shadows were rewritten to M.  With any shadow in the table
that is the number of real neighbours; a table without a single shadow counts one slot fewer in the rows that hold the
largest index.  The caller's table keeps its -1 entries.
"""
import torch
import torch.nn as nn

from . import _lib
from . import fused as _fused
from .grid_sampling import GridSampling3D
from .kpconv import _require_gpu
from .kpconv_blocks import (FastBatchNorm1d, PDData, RadiusNeighbourFinder, _copy, block_query_data,  # noqa: F401
                            bn_act_rows, strided_shortcut)  # (PDData: re-exported)
from .partial_dense import FPModule_PD

_EMBEDDING = {"xyz": 0, "sin_cos": 1}
_REDUCTION = {"sum": 0, "avg": 1}
_dim_mat_cache = {}


def sin_cos_width(num_inputs):
    """F of the sin_cos embedding: C / 6 wavelengths per axis, or 1 for the C == 9 layout [sin, cos] x 3 + xyz."""
    return 1 if num_inputs == 9 else num_inputs // 6


def _dim_mat(feat_dim, device):
    """1000^(j / F), j < F, evaluated on the host with the reference's expression (ops.py:70-71, 84-85) and kept on the
    device per (F, device)."""
    key = (feat_dim, device.type, device.index)
    t = _dim_mat_cache.get(key)
    if t is None:
        feat_range = torch.arange(feat_dim, dtype=torch.float32)
        t = _dim_mat_cache[key] = torch.pow(1.0 * 1000, (1.0 / feat_dim) * feat_range).to(device)
    return t


def _check_width(num_inputs, position_embedding, reduction):
    if position_embedding not in _EMBEDDING:
        raise NotImplementedError("Position embedding {} not supported in PosPool".format(position_embedding))
    if reduction == "max":
        raise NotImplementedError("PosPool reduction 'max' is not available: the reference cannot run it either (it hands "
                                  "torch.max's (values, indices) tuple to BatchNorm and raises AttributeError)")
    if reduction not in _REDUCTION:
        raise NotImplementedError("Reduction {} not supported in PosPool".format(reduction))
    if position_embedding == "xyz" and num_inputs % 3 != 0:
        raise ValueError("PosPool 'xyz' needs a feature width divisible by 3, got %d" % num_inputs)
    if position_embedding == "sin_cos" and num_inputs % 6 != 0 and num_inputs != 9:
        raise ValueError("PosPool 'sin_cos' needs a feature width divisible by 6 (or 9), got %d" % num_inputs)


class _PosPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, query, support, nbr, radius, embedding, reduction):
        dev = query.device
        x = features.detach().float().contiguous()
        Nq, Mn = nbr.shape
        M, C = x.shape
        dim_mat = _dim_mat(sin_cos_width(C), dev) if embedding == 1 else None
        out = torch.empty((Nq, C), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0] and reduction == 1
        counts = torch.empty((Nq,), dtype=torch.float32, device=dev) if need else None
        padding = torch.empty((1,), dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            stream = _lib.stream_ptr(dev)
            _lib.call("tp3d_pospool_padding_i64", _lib.ptr(nbr), Nq * Mn, M, _lib.ptr(padding), stream)
            _lib.call("tp3d_pospool_fwd_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(x),
                      _lib.ptr(padding), _lib.ptr(dim_mat), Nq, M, Mn, C, radius, embedding, reduction, _lib.ptr(out),
                      _lib.ptr(counts), stream)
        ctx.save_for_backward(query, support, nbr, counts, dim_mat)
        ctx.cfg = (radius, embedding, reduction, M, C)
        return out

    @staticmethod
    def backward(ctx, d_out):
        query, support, nbr, counts, dim_mat = ctx.saved_tensors
        radius, embedding, reduction, M, C = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        dev = d_out.device
        d_out = d_out.float().contiguous()
        Nq, Mn = nbr.shape
        dx = torch.empty((M, C), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            inv, inv_bytes, ready, token = _lib.neighbour_inverse(nbr, M, dev)
            _lib.call("tp3d_pospool_bwd_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(d_out),
                      _lib.ptr(counts), _lib.ptr(dim_mat), Nq, M, Mn, C, radius, embedding, reduction, _lib.ptr(dx),
                      _lib.ptr(inv), inv_bytes, ready, _lib.stream_ptr(dev))
            _lib.inverse_built(token, dev)
        return dx, None, None, None, None, None, None


def pospool(query, support, neighbors, features, radius, position_embedding="xyz", reduction="avg"):
    """Position pooling: (Nq, C) = reduce over the neighbours of geo(relative position) * features[neighbour].
    query (Nq, 3), support (M, 3), neighbors (Nq, Mn) int64 with -1 (or >= M) for a shadow, features (M, C)."""
    _check_width(features.shape[1], position_embedding, reduction)
    _require_gpu(query, support, neighbors, features)
    if not float(radius) > 0.0:
        raise ValueError("PosPool needs a positive radius")
    q = query.detach().float().contiguous()
    s = support.detach().float().contiguous()
    nbr = neighbors.long().contiguous()
    return _PosPool.apply(features, q, s, nbr, float(radius), _EMBEDDING[position_embedding], _REDUCTION[reduction])


class PosPoolLayer(nn.Module):
    """PosPool -> BatchNorm -> activation [-> Linear -> BatchNorm -> activation when the width changes or
    `output_conv`] with the reference's fields (ops.py:7-35)."""

    def __init__(self, num_inputs, num_outputs, radius, position_embedding="xyz", reduction="avg", output_conv=False,
                 activation=nn.LeakyReLU(negative_slope=0.2), bn_momentum=0.02, bn=FastBatchNorm1d, fused=True):
        super().__init__()
        _check_width(num_inputs, position_embedding, reduction)
        self.num_inputs = num_inputs
        self.num_outputs = num_outputs
        self.radius = radius
        self.position_embedding = position_embedding
        self.reduction = reduction
        self.output_conv = True if num_outputs != num_inputs else output_conv
        self.fused = fused
        self.bn = bn(num_inputs, momentum=bn_momentum) if bn else None
        self.activation = activation
        if self.output_conv:
            self.oconv = nn.Sequential(nn.Linear(num_inputs, num_outputs, bias=False), bn(num_outputs, momentum=bn_momentum),
                                       activation)

    def forward(self, query_points, support_points, neighbors, x):
        x = pospool(query_points, support_points, neighbors, x, self.radius, self.position_embedding, self.reduction)
        x = bn_act_rows(x, self.bn, self.activation, self.fused)
        if self.output_conv:
            x = _fused.rows_seq(self.oconv, x) if self.fused else self.oconv(x)
        return x


class _PosPoolBlock(nn.Module):
    """What SimpleBlock and SimpleInputBlock share: the search, the layer, the sampler of a strided block and the
    forward pass around `_features` (blocks.py:59-83, 142-167)."""

    DENSITY_PARAMETER = 2.5

    def _build(self, num_inputs, num_outputs, grid_size, prev_grid_size, sigma, max_num_neighbors, position_embedding,
               reduction, output_conv, activation, bn_momentum, bn, sampler, fused):
        self.fused = fused
        search_radius = self.DENSITY_PARAMETER * sigma * prev_grid_size
        self.neighbour_finder = RadiusNeighbourFinder(search_radius, max_num_neighbors)
        self.pospool = PosPoolLayer(num_inputs, num_outputs, search_radius, position_embedding=position_embedding,
                                    reduction=reduction, output_conv=output_conv, activation=activation,
                                    bn_momentum=bn_momentum, bn=bn, fused=fused)
        self.is_strided = prev_grid_size != grid_size
        self.sampler = (sampler if sampler is not None else GridSampling3D(grid_size)) if self.is_strided else None

    def _features(self, x):
        return x

    def forward(self, data, precomputed=None, **kwargs):
        query_data, q_pos, idx_neighboors = block_query_data(self, data, precomputed)
        query_data.x = self.pospool(q_pos, data.pos, idx_neighboors, self._features(data.x))
        query_data.block_idx = data.block_idx + 1
        return query_data


class SimpleBlock(_PosPoolBlock):
    """PosPool layer on a radius neighbourhood; strided when prev_grid_size != grid_size (blocks.py:13-86)."""

    def __init__(self, down_conv_nn=None, grid_size=None, prev_grid_size=None, sigma=1.0, max_num_neighbors=16,
                 position_embedding="xyz", reduction="avg", output_conv=False, activation=nn.LeakyReLU(negative_slope=0.2),
                 bn_momentum=0.01, bn=FastBatchNorm1d, sampler=None, fused=True, **kwargs):
        super().__init__()
        assert len(down_conv_nn) == 2
        num_inputs, num_outputs = down_conv_nn
        self._build(num_inputs, num_outputs, grid_size, prev_grid_size, sigma, max_num_neighbors, position_embedding,
                    reduction, output_conv, activation, bn_momentum, bn, sampler, fused)


class SimpleInputBlock(_PosPoolBlock):
    """Linear -> BatchNorm -> activation on the input features, then the PosPool layer (blocks.py:89-170)."""

    def __init__(self, down_conv_nn=None, grid_size=None, prev_grid_size=None, sigma=1.0, max_num_neighbors=16,
                 position_embedding="xyz", reduction="avg", output_conv=False, activation=nn.LeakyReLU(negative_slope=0.2),
                 bn_momentum=0.01, bn=FastBatchNorm1d, sampler=None, fused=True, **kwargs):
        super().__init__()
        assert len(down_conv_nn) == 3
        num_inputs, d_2, num_outputs = down_conv_nn
        if bn:
            self.unary_1 = nn.Sequential(nn.Linear(num_inputs, d_2, bias=False), bn(d_2, momentum=bn_momentum), activation)
        else:
            self.unary_1 = nn.Sequential(nn.Linear(num_inputs, d_2, bias=False), activation)
        self._build(d_2, num_outputs, grid_size, prev_grid_size, sigma, max_num_neighbors, position_embedding, reduction,
                    output_conv, activation, bn_momentum, bn, sampler, fused)

    def _features(self, x):
        return _fused.rows_seq(self.unary_1, x) if self.fused else self.unary_1(x)


class ResnetBBlock(nn.Module):
    """unary -> SimpleBlock (`aggregation`) -> unary, plus the shortcut (neighbourhood max-pool when strided), summed,
    then the activation (blocks.py:173-297).  d_2 = num_outputs // bottleneck_ratio."""

    def __init__(self, down_conv_nn=None, grid_size=None, prev_grid_size=None, sigma=1, max_num_neighbors=16,
                 position_embedding="xyz", reduction="avg", output_conv=False, activation=nn.LeakyReLU(negative_slope=0.2),
                 has_bottleneck=True, bottleneck_ratio=2, bn_momentum=0.01, bn=FastBatchNorm1d, sampler=None, fused=True,
                 **kwargs):
        super().__init__()
        assert len(down_conv_nn) == 2, "down_conv_nn should be of size 2"
        num_inputs, num_outputs = down_conv_nn
        d_2 = num_outputs // bottleneck_ratio
        self.fused = fused
        self.is_strided = prev_grid_size != grid_size
        self.has_bottleneck = has_bottleneck
        channel_size = [d_2, d_2] if has_bottleneck else [num_inputs, num_outputs]
        self.aggregation = SimpleBlock(down_conv_nn=channel_size, grid_size=grid_size, prev_grid_size=prev_grid_size,
                                       sigma=sigma, max_num_neighbors=max_num_neighbors,
                                       position_embedding=position_embedding, reduction=reduction, output_conv=output_conv,
                                       activation=activation, bn_momentum=bn_momentum, bn=bn, sampler=sampler, fused=fused)
        if has_bottleneck:
            if bn:
                self.unary_1 = nn.Sequential(nn.Linear(num_inputs, d_2, bias=False), bn(d_2, momentum=bn_momentum),
                                             activation)
                self.unary_2 = nn.Sequential(nn.Linear(d_2, num_outputs, bias=False), bn(num_outputs, momentum=bn_momentum))
            else:
                self.unary_1 = nn.Sequential(nn.Linear(num_inputs, d_2, bias=False), activation)
                self.unary_2 = nn.Sequential(nn.Linear(d_2, num_outputs, bias=False))
        if num_inputs != num_outputs:
            if bn:
                self.shortcut_op = nn.Sequential(nn.Linear(num_inputs, num_outputs, bias=False),
                                                 bn(num_outputs, momentum=bn_momentum))
            else:
                self.shortcut_op = nn.Linear(num_inputs, num_outputs, bias=False)
        else:
            self.shortcut_op = nn.Identity()
        self.activation = activation

    def forward(self, data, precomputed=None, **kwargs):
        output = _copy(data)
        shortcut_x = data.x
        seq = _fused.rows_seq if self.fused else (lambda m, x: m(x))
        if self.has_bottleneck:
            output.x = seq(self.unary_1, output.x)
        output = self.aggregation(output, precomputed=precomputed)
        if self.has_bottleneck:
            output.x = seq(self.unary_2, output.x)
        if self.is_strided:
            shortcut_x = strided_shortcut(shortcut_x, output.idx_neighboors, self.fused)
        output.x = self.activation(output.x + seq(self.shortcut_op, shortcut_x))
        return output

    @property
    def sampler(self):
        return self.aggregation.sampler

    @property
    def neighbour_finder(self):
        return self.aggregation.neighbour_finder


_BLOCKS = {"SimpleBlock": SimpleBlock, "SimpleInputBlock": SimpleInputBlock, "ResnetBBlock": ResnetBBlock}


class PPStageBlock(nn.Module):
    """Sequence of blocks built from per-block lists (blocks.py:300-375)."""

    def __init__(self, block_names=None, down_conv_nn=None, grid_size=None, prev_grid_size=None, has_bottleneck=None,
                 bottleneck_ratio=None, max_num_neighbors=None, position_embedding=None, reduction=None, output_conv=None,
                 bn_momentum=None, **kwargs):
        super().__init__()
        assert len(block_names) == len(down_conv_nn)
        self.blocks = nn.ModuleList()
        for i, name in enumerate(block_names):
            block_kwargs = {k: (v[i] if isinstance(v, (list, tuple)) else v) for k, v in kwargs.items()}
            self.blocks.append(_BLOCKS[name](
                down_conv_nn=down_conv_nn[i], grid_size=grid_size[i], prev_grid_size=prev_grid_size[i],
                has_bottleneck=has_bottleneck[i], max_num_neighbors=max_num_neighbors[i], bottleneck_ratio=bottleneck_ratio,
                position_embedding=position_embedding, reduction=reduction, output_conv=output_conv,
                bn_momentum=bn_momentum, **block_kwargs))

    def forward(self, data, precomputed=None, **kwargs):
        for block in self.blocks:
            data = block(data, precomputed=precomputed)
        return data

    @property
    def sampler(self):
        return [b.sampler for b in self.blocks]

    @property
    def neighbour_finder(self):
        return [b.neighbour_finder for b in self.blocks]


MAX_NUM_NEIGHBORS = [[26, 26], [26, 31], [31, 38], [38, 41], [41, 39]]


def ppnet_config(input_nc, in_feat=72, in_grid_size=0.04, position_embedding="sin_cos", reduction="avg", output_conv=False,
                 bottleneck_ratio=2, bn_momentum=0.01):
    """The resolved option lists of `PPNet` (sin_cos) / `PPNetxyz` in conf/models/segmentation/ppnet.yaml."""
    f, g = in_feat, in_grid_size
    down = []
    for i in range(5):
        if i == 0:
            nn_, names, neck = [[input_nc, f, f], [f, 2 * f]], ["SimpleInputBlock", "ResnetBBlock"], [False, True]
            prev = [g, g]
        else:
            w = f * 2 ** i
            nn_, names, neck = [[w, 2 * w], [2 * w, 2 * w]], ["ResnetBBlock", "ResnetBBlock"], [True, True]
            prev = [2 ** (i - 1) * g, 2 ** i * g]
        down.append(dict(down_conv_nn=nn_, grid_size=[2 ** i * g, 2 ** i * g], prev_grid_size=prev, block_names=names,
                         has_bottleneck=neck, max_num_neighbors=list(MAX_NUM_NEIGHBORS[i]),
                         position_embedding=position_embedding, reduction=reduction, output_conv=output_conv,
                         bottleneck_ratio=bottleneck_ratio, bn_momentum=bn_momentum))
    up_nn = [[32 * f + 16 * f, 8 * f], [8 * f + 8 * f, 4 * f], [4 * f + 4 * f, 2 * f], [2 * f + 2 * f, f]]
    up = [dict(up_k=1, up_conv_nn=c, bn_momentum=bn_momentum) for c in up_nn]
    return dict(down_conv=down, up_conv=up, mlp_cls=dict(nn=[f, f], dropout=0, bn_momentum=bn_momentum))


class PPNet(nn.Module):
    """The segmentation network of models/segmentation/ppnet.py without category heads: five `PPStageBlock` stages,
    four `FPModule_PD` (up_k = 1, skip), `FC_layer` = Linear -> FastBatchNorm1d -> LeakyReLU(0.2) -> Linear ("Class") ->
    LogSoftmax; every Linear xavier-normal.  forward: data (pos (N,3), x (N, input_nc), batch (N) sorted) ->
    (N, num_classes) log-probabilities."""

    def __init__(self, input_nc, num_classes, in_grid_size, in_feat=72, position_embedding="sin_cos", reduction="avg",
                 output_conv=False, bottleneck_ratio=2, bn_momentum=0.01, config=None, fused=True):
        super().__init__()
        self.fused = fused
        cfg = config if config is not None else ppnet_config(input_nc, in_feat, in_grid_size, position_embedding, reduction,
                                                             output_conv, bottleneck_ratio, bn_momentum)
        self.down_modules = nn.ModuleList(PPStageBlock(fused=fused, **opt) for opt in cfg["down_conv"])
        self.inner_modules = nn.ModuleList([nn.Identity()])
        self.up_modules = nn.ModuleList(FPModule_PD(fused=fused, **opt) for opt in cfg["up_conv"])
        mlp = cfg["mlp_cls"]
        self.FC_layer = nn.Sequential()
        width = mlp["nn"][0]
        for i in range(1, len(mlp["nn"])):
            self.FC_layer.add_module(str(i), nn.Sequential(nn.Linear(width, mlp["nn"][i], bias=False),
                                                           FastBatchNorm1d(mlp["nn"][i], momentum=mlp["bn_momentum"]),
                                                           nn.LeakyReLU(0.2)))
            width = mlp["nn"][i]
        if mlp["dropout"]:
            self.FC_layer.add_module("Dropout", nn.Dropout(p=mlp["dropout"]))
        self.FC_layer.add_module("Class", nn.Linear(width, num_classes, bias=False))
        self.FC_layer.add_module("Softmax", nn.LogSoftmax(-1))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, data, precomputed_down=None, precomputed_up=None):
        stack_down = []
        for i in range(len(self.down_modules) - 1):
            data = self.down_modules[i](data, precomputed=precomputed_down)
            stack_down.append(data)
        data = self.down_modules[-1](data, precomputed=precomputed_down)
        for up in self.up_modules:
            data = up((data, stack_down.pop()), precomputed=precomputed_up)
        x = data.x
        for name, m in self.FC_layer.named_children():
            x = _fused.rows_seq(m, x) if (self.fused and isinstance(m, nn.Sequential)) else m(x)
        return x
