"""Message-passing RSConv on ragged batches (RSConv_2LD / RSConv_4LD), on the HIP kernels of csrc/rsconv_mp.hip.

Mirrors (same constructor arguments and attribute names -- hence state_dict keys -- and forward contracts):
  * `Convolution`, `RSConvDown`   torch_points3d/modules/RSConv/message_passing.py:10-60 over BaseConvolutionDown,
                                  core/base_conv/message_passing.py:35-58
  * `RSConvMP`                    conf/models/segmentation/rsconv.yaml:3-55 (`RSConv_2LD`, `RSConv_4LD`, class
                                  rsconv.RSConv_MP = Segmentation_MP) nested as models/base_architectures/unet.py nests it
The sampler, the radius search (CSR `Edges`), the set-abstraction forward (BaseConvolutionDown) and the nested network
with its head (SegmentationMP: GlobalBaseModule, FPModule) are those of pointnet2_mp.py.  Per edge (j -> i) the layer computes

    h_ij = [ |p_i - p_j|, p_i - p_j, p_i, p_j ]        torchpoints.rsconv_relation_rows   (E, 12), 10 used
    M_ij = local_nn(h_ij)                              fused.rows_mlp: BatchNorm over ALL edges, so M exists in memory
    out_i = global_nn(act(max_j M_ij * x_j))           torchpoints.rsconv_msgmax: x[col], the product and the rows the
                                                       max reads are never written

Two places where the reference cannot be followed literally (it lists both models as known to fail,
test/test_models.py:116-125); DESIGN.md "message-passing RSConv":
  * `BaseConvolutionDown.forward` (core/base_conv/message_passing.py:53) hands `conv` the tuple (pos[idx], pos) while
    edge_index = [support rows; query rows].  Under torch_geometric's (source, target) convention pos_j would index the
    SAMPLED cloud with support indices.  `Convolution.message` evidently means pos_i = the query and pos_j = the support
    point: that reading is evaluated here, source = pos, target = pos[idx].
  * `self.sampler(pos, batch)` passes the batch vector as BaseSampler.__call__'s `x`.  It is treated as the batch, as
    for PointNet2MP.
"""
import torch.nn as nn

from . import fused as _fused
from . import torchpoints as _tp
from .partial_dense import MLP
from .pointnet2_mp import BaseConvolutionDown, FPSSampler, RadiusNeighbourFinder, SegmentationMP, _edge_start_of


class Convolution(nn.Module):
    """out[i] = global_nn(activation(max over the edges (j -> i) of local_nn(h_ij) * x_j)), x_j = pos_j without features.

    forward(x, (pos_s, pos_q), edges): x (M, C) or None, support / query positions, `edges` = (row, col) of a finder
    (rows ascending).  local_nn must end in the width of x (3 when x is None).  A query without an edge gets
    activation(0.0).  fused=False runs the MLPs as plain module calls instead of fused.rows_mlp."""

    def __init__(self, local_nn, activation=nn.ReLU(), global_nn=None, aggr="max", **kwargs):
        super().__init__()
        if aggr != "max":
            raise NotImplementedError("RSConv message passing is served for aggr='max' only, got %r" % (aggr,))
        self.local_nn = MLP(local_nn)
        self.activation = activation
        self.global_nn = MLP(global_nn) if global_nn is not None else None
        self.fused = kwargs.get("fused", True)

    def _mlp(self, mlp, rows):
        return _fused.rows_mlp(mlp, rows) if self.fused else mlp(rows)

    def forward(self, x, pos, edges):
        pos_s, pos_q = pos
        edge_start, col = _edge_start_of(edges, pos_q.shape[0])
        if x is None:
            x = pos_s.detach()  # positions carry no gradient anywhere in this project
        rows = _tp.rsconv_relation_rows(pos_s, pos_q, edge_start, col, ld=12 if self.fused else 10)
        weights = self._mlp(self.local_nn, rows)
        if weights.shape[1] != x.shape[1]:
            raise ValueError("local_nn ends in %d channels, the features have %d" % (weights.shape[1], x.shape[1]))
        out = self.activation(_tp.rsconv_msgmax(weights, x, edge_start, col))
        if self.global_nn is not None:
            out = self._mlp(self.global_nn, out)
        return out


class RSConvDown(BaseConvolutionDown):
    """FPSSampler(ratio) + RadiusNeighbourFinder(radius) (at most 64 neighbours, its default) + Convolution(local_nn,
    global_nn=down_conv_nn)."""

    def __init__(self, ratio=None, radius=None, local_nn=None, down_conv_nn=None, *args, **kwargs):
        super().__init__()
        self.sampler = FPSSampler(ratio)
        self.neighbour_finder = RadiusNeighbourFinder(radius)
        self._index = kwargs.get("index", None)
        self._conv = Convolution(local_nn=local_nn, global_nn=down_conv_nn, fused=kwargs.get("fused", True))


def rsconv_mp_config(name):
    """conf/models/segmentation/rsconv.yaml:3-55 resolved.  Both configurations are self-consistent only for
    `data.x is None` and FEAT = 3: the first local_nn ends in FEAT and multiplies pos_j (3 wide), the last up_conv_nn
    has no room for skip features, and the innermost width is 128 + 3 (written as 131 in RSConv_4LD).  They are
    resolved that way.  The `ratios` / `radius` keys under RSConv_2LD's up_conv are kept but unused, as the
    reference's FPModule(**kwargs) ignores them."""
    feat = 3
    if name == "RSConv_2LD":
        return dict(
            down_conv=dict(ratios=[0.2, 0.25], radius=[0.1, 0.2], local_nn=[[10, 8, feat], [10, 32, 64, 64]],
                           down_conv_nn=[[feat, 16, 32, 64], [64, 64, 128]]),
            innermost=dict(aggr="max", nn=[128 + feat, 128]),
            up_conv=dict(ratios=[1, 0.25, 0.2], radius=[0.2, 0.2, 0.1], up_conv_nn=[[128 + 128, 64], [64 + 64, 64], [64, 64]],
                         up_k=[1, 3, 3], skip=True),
            mlp_cls=dict(nn=[64, 64, 64, 64, 64], dropout=0.5))
    if name == "RSConv_4LD":
        return dict(
            down_conv=dict(ratios=[0.5, 0.5, 0.5, 0.5], radius=[0.1, 0.2, 0.3, 0.4],
                           local_nn=[[10, 8, feat], [10, 16, 16], [10, 32, 32], [10, 64, 64]],
                           down_conv_nn=[[feat, 16, 16], [16, 32, 32], [32, 64, 64], [64, 128, 128]]),
            innermost=dict(aggr="max", nn=[128 + feat, 128]),
            up_conv=dict(up_conv_nn=[[128 + 128, 128], [128 + 64, 64], [64 + 32, 32], [32 + 16, 32], [32, 64]],
                         up_k=[1, 3, 3, 3, 3], skip=True),
            mlp_cls=dict(nn=[64, 64, 64, 64, 64], dropout=0.1))
    raise ValueError("unknown message-passing RSConv config %r" % name)


class RSConvMP(SegmentationMP):
    """RSConv_MP segmentation network: SegmentationMP over RSConvDown.

    cfg: "RSConv_2LD" / "RSConv_4LD" (rsconv_mp_config) or a dict with the YAML's fields (down_conv: ratios, radius,
    local_nn, down_conv_nn; the rest as SegmentationMP).  data.x = None for the two named configurations."""

    def __init__(self, cfg, num_classes, fused=True):
        if isinstance(cfg, str):
            cfg = rsconv_mp_config(cfg)
        down = cfg["down_conv"]
        super().__init__(cfg, num_classes, lambda i: RSConvDown(
            ratio=down["ratios"][i], radius=down["radius"][i], local_nn=down["local_nn"][i],
            down_conv_nn=down["down_conv_nn"][i], index=i, fused=fused))
