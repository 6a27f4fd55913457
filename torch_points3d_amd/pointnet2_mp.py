"""Message-passing PointNet++ on ragged batches (clouds of different sizes in one batch), on the HIP kernels.

Mirrors (same constructor arguments and attribute names -- hence state_dict keys -- and forward contracts):
  * `FPSSampler`                       torch_points3d/core/spatial_ops/sampling.py:13-63
  * `RadiusNeighbourFinder`            torch_points3d/core/spatial_ops/neighbour_finder.py:25-39
  * `MultiscaleRadiusNeighbourFinder`  torch_points3d/core/spatial_ops/neighbour_finder.py:89-153
  * `PointConv`                        torch_geometric.nn.PointConv as modules/pointnet2/message_passing.py:20,26 uses it
  * `SAModule`                         torch_points3d/modules/pointnet2/message_passing.py:9-31 over
                                       BaseMSConvolutionDown, core/base_conv/message_passing.py:61-94
  * `BaseConvolutionDown`              the forward of core/base_conv/message_passing.py:35-58 and 61-94, one or more scales
  * `GlobalBaseModule`, `FPModule`     torch_points3d/core/base_conv/message_passing.py:132-151, 157-176
  * `SegmentationMP`, `PointNet2MP`    conf/models/segmentation/pointnet2.yaml:5-57 (`pointnet2`, `pointnet2ms`) nested as
                                       models/base_architectures/unet.py:93-138 nests it, with the Segmentation_MP head
                                       (models/segmentation/base.py:27-55)
The reference gets sampling and the radius search from torch_cluster and the max from torch_scatter; here they are
entry points of libtp3d_hip.so: tp3d_fps_ragged_f32 (csrc/fps.hip), the partial-dense ball query, and the edge-list
kernels of csrc/pointconv.hip.  The neighbourhood of a query is a run of an edge list in CSR form (`Edges`), so
BatchNorm inside `local_nn` sees the real edges only -- nothing is padded.

Differences from the reference stack that its tree does not pin (DESIGN.md "message-passing PointNet++"): the
sampling quota's rounding, the deterministic start row of the sampler, and PointConv's self-loop rewriting.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused as _fused
from . import torchpoints as _tp
from .kpconv_blocks import PDData
from .partial_dense import MLP, knn_interpolate


def _is_list(v):
    return isinstance(v, (list, tuple))


class BaseSampler(object):
    """ratio / num_to_sample / subsampling_param handling of sampling.py:13-50"""

    def __init__(self, ratio=None, num_to_sample=None, subsampling_param=None):
        if num_to_sample is not None:
            if (ratio is not None) or (subsampling_param is not None):
                raise ValueError("Can only specify ratio or num_to_sample or subsampling_param, not several !")
            self._num_to_sample = num_to_sample
        elif ratio is not None:
            self._ratio = ratio
        elif subsampling_param is not None:
            self._subsampling_param = subsampling_param
        else:
            raise Exception('At least ["ratio, num_to_sample, subsampling_param"] should be defined')

    def __call__(self, pos, x=None, batch=None):
        return self.sample(pos, batch=batch, x=x)

    def _get_ratio_to_sample(self, batch_size):
        if hasattr(self, "_ratio"):
            return self._ratio
        return self._num_to_sample / float(batch_size)


class FPSSampler(BaseSampler):
    """Furthest-point sampling of every cloud of the batch: indices into pos, cloud after cloud.  Call it with
    `batch=` by keyword: BaseSampler's second positional argument is `x`."""

    def sample(self, pos, batch=None, **kwargs):
        if len(pos.shape) != 2:
            raise ValueError(" This class is for sparse data and expects the pos tensor to be of dimension 2")
        return _tp.fps_ragged(pos, batch, ratio=self._get_ratio_to_sample(pos.shape[0]))


class Edges(tuple):
    """(row, col) of a radius search -- row = query index, ascending; col = support row, ascending within a query --
    carrying the CSR offsets `edge_start` (Nq + 1) the kernels read."""

    def __new__(cls, edge_start, col):
        nq = edge_start.numel() - 1
        counts = edge_start[1:] - edge_start[:-1]
        row = torch.repeat_interleave(torch.arange(nq, device=col.device), counts, output_size=col.numel())
        self = super().__new__(cls, (row, col))
        self.edge_start = edge_start
        return self


def _radius(x, y, r, batch_x, batch_y, max_num_neighbors):
    """torch_geometric's `radius(x, y, r, batch_x, batch_y, max_num_neighbors)`: the first max_num_neighbors support
    rows in index order (torchpoints.radius_edges; one host read for the edge count)."""
    return Edges(*_tp.radius_edges(r, max_num_neighbors, x, y, batch_x, batch_y))


class RadiusNeighbourFinder(object):
    def __init__(self, radius, max_num_neighbors=64, conv_type="message_passing"):
        self._radius = radius
        self._max_num_neighbors = max_num_neighbors
        self._conv_type = conv_type.lower()

    def find_neighbours(self, x, y, batch_x=None, batch_y=None):
        if self._conv_type == "message_passing":
            return _radius(x, y, self._radius, batch_x, batch_y, self._max_num_neighbors)
        if self._conv_type in ("dense", "partial_dense"):
            return _tp.ball_query(self._radius, self._max_num_neighbors, x, y, mode=self._conv_type, batch_x=batch_x,
                                  batch_y=batch_y)[0]
        raise NotImplementedError

    def __call__(self, x, y, batch_x=None, batch_y=None):
        return self.find_neighbours(x, y, batch_x, batch_y)

    def __repr__(self):
        return str(self.__class__.__name__) + " " + str(self.__dict__)


class MultiscaleRadiusNeighbourFinder(object):
    """Radius search at several scales; a scalar radius or neighbour count is repeated for every scale."""

    def __init__(self, radius, max_num_neighbors=64):
        if not _is_list(max_num_neighbors) and _is_list(radius):
            self._radius = list(radius)
            self._max_num_neighbors = [max_num_neighbors for _ in self._radius]
            return
        if not _is_list(radius) and _is_list(max_num_neighbors):
            self._max_num_neighbors = list(max_num_neighbors)
            self._radius = [radius for _ in self._max_num_neighbors]
            return
        if _is_list(max_num_neighbors):
            if len(max_num_neighbors) != len(radius):
                raise ValueError("Both lists max_num_neighbors and radius should be of the same length")
            self._max_num_neighbors = list(max_num_neighbors)
            self._radius = list(radius)
            return
        self._max_num_neighbors = [max_num_neighbors]
        self._radius = [radius]

    def find_neighbours(self, x, y, batch_x=None, batch_y=None, scale_idx=0):
        if scale_idx >= self.num_scales:
            raise ValueError("Scale %i is out of bounds %i" % (scale_idx, self.num_scales))
        return _radius(x, y, self._radius[scale_idx], batch_x, batch_y, self._max_num_neighbors[scale_idx])

    @property
    def num_scales(self):
        return len(self._radius)

    def __call__(self, x, y, batch_x=None, batch_y=None, scale_idx=0):
        return self.find_neighbours(x, y, batch_x, batch_y, scale_idx)


def _edge_start_of(edges, nq):
    """CSR offsets of an edge list: `Edges` carries them; a plain (row, col) pair with ascending rows gets them counted"""
    es = getattr(edges, "edge_start", None)
    if es is not None:
        return es, edges[1]
    row, col = edges
    es = torch.zeros(nq + 1, dtype=torch.int64, device=row.device)
    es[1:] = torch.cumsum(torch.bincount(row, minlength=nq), 0)
    return es, col


class PointConv(nn.Module):
    """out[i] = global_nn( max over the edges (j -> i) of local_nn( cat([x_j, pos_j - pos_i]) ) ).

    forward(x, (pos_s, pos_q), edges): x (M, C) or None, support / query positions, `edges` = (row, col) of a finder
    (rows ascending).  No self-loop rewriting (torch_geometric 1.7.2 defaults to add_self_loops=True):
    a sampled query is itself a support point at distance 0, so it always has an edge.  A query WITHOUT an edge gets
    0.0 (torch_scatter's fill value)."""

    def __init__(self, local_nn=None, global_nn=None):
        super().__init__()
        self.local_nn = local_nn
        self.global_nn = global_nn

    def forward(self, x, pos, edges):
        pos_s, pos_q = pos
        edge_start, col = _edge_start_of(edges, pos_q.shape[0])
        rows = _tp.pointconv_rows(x, pos_s, pos_q, edge_start, col)
        width = (0 if x is None else x.shape[1]) + 3
        if self.local_nn is not None:
            rows = _fused.rows_mlp(self.local_nn, rows)
            width = rows.shape[1]
        out = _tp.segment_max(rows, edge_start, C=width)
        if self.global_nn is not None:
            out = _fused.rows_mlp(self.global_nn, out)
        return out


def copy_from_to(data, batch):
    for key in data.keys:
        if key not in batch.keys:
            setattr(batch, key, getattr(data, key, None))


class BaseConvolutionDown(nn.Module):
    """Set abstraction: sample once, then per scale of the finder search + the shared convolution, scales concatenated.
    A subclass sets `sampler`, `neighbour_finder` (multi-scale or not), `_conv` and `_index`."""

    def conv(self, x, pos, edge_index, batch):
        return self._conv(x, pos, edge_index)

    def forward(self, data, **kwargs):
        out = PDData()
        x, pos, batch = data.x, data.pos, data.batch
        idx = self.sampler(pos, batch=batch)
        out.idx = idx
        pos_q, batch_q = pos[idx], batch[idx]
        finder = self.neighbour_finder
        scales = [dict(scale_idx=s) for s in range(finder.num_scales)] if hasattr(finder, "num_scales") else [{}]
        ms_x = []
        for scale in scales:
            edges = finder(pos, pos_q, batch_x=batch, batch_y=batch_q, **scale)
            ms_x.append(self.conv(x, (pos, pos_q), edges, batch))
        out.x = ms_x[0] if len(ms_x) == 1 else torch.cat(ms_x, -1)
        out.pos = pos_q
        out.batch = batch_q
        copy_from_to(data, out)
        return out


class SAModule(BaseConvolutionDown):
    """FPSSampler(ratio) + MultiscaleRadiusNeighbourFinder(radius, radius_num_point) + PointConv(MLP(down_conv_nn))."""

    def __init__(self, ratio=None, radius=None, radius_num_point=None, down_conv_nn=None, *args, **kwargs):
        super().__init__()
        self.sampler = FPSSampler(ratio=ratio)
        self.neighbour_finder = MultiscaleRadiusNeighbourFinder(radius, max_num_neighbors=radius_num_point)
        self._index = kwargs.get("index", None)
        local_nn = MLP(down_conv_nn) if down_conv_nn is not None else None
        self._conv = PointConv(local_nn=local_nn, global_nn=None)
        self._radius = radius
        self._ratio = ratio
        self._num_points = radius_num_point

    def extra_repr(self):
        return "{}(ratio {}, radius {}, radius_points {})".format(self.__class__.__name__, self._ratio, self._radius,
                                                                  self._num_points)


def global_max_pool(x, batch):
    """per-cloud max of the rows of x (N, C) under a sorted batch vector (tp3d_segment_max_fwd_f32)"""
    seg, _, _ = _tp._segments(_tp._i64(batch))
    return _tp.segment_max(x, seg)


def global_mean_pool(x, batch):
    seg, nclouds, _ = _tp._segments(_tp._i64(batch))
    total = torch.zeros((nclouds, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
    return total / (seg[1:] - seg[:-1]).clamp(min=1).to(x.dtype).unsqueeze(-1)


class GlobalBaseModule(nn.Module):
    """MLP(cat[x, pos]) then one pooled row per cloud; pos becomes zeros (clouds, 3), batch = arange(clouds)."""

    def __init__(self, nn, aggr="max", *args, **kwargs):
        super().__init__()
        self.nn = MLP(nn)
        self.pool = global_max_pool if aggr == "max" else global_mean_pool

    def forward(self, data, **kwargs):
        out = PDData()
        x, pos, batch = data.x, data.pos, data.batch
        if pos is not None:
            x = _fused.rows_mlp(self.nn, torch.cat([x, pos], dim=1))
        else:
            x = _fused.rows_mlp(self.nn, x)
        x = self.pool(x, batch)
        out.x = x
        if pos is not None:
            out.pos = pos.new_zeros((x.size(0), 3))
        out.batch = torch.arange(x.size(0), device=batch.device)
        copy_from_to(data, out)
        return out


class FPModule(nn.Module):
    """Feature propagation: knn_interpolate (k nearest, inverse squared distance) onto the skip level, concatenation
    with the skip features (fused into the interpolation kernel), MLP(bias=False)."""

    def __init__(self, up_k, up_conv_nn, *args, **kwargs):
        super().__init__()
        self.k = up_k
        self._skip = kwargs.get("skip", True)
        self._index = kwargs.get("index", None)
        bn_momentum = kwargs.get("bn_momentum", 0.1)
        self.nn = MLP(up_conv_nn, bn_momentum=bn_momentum, bias=False)

    def forward(self, data, **kwargs):
        out = PDData()
        data, data_skip = data
        x, pos, batch = data.x, data.pos, data.batch
        x_skip, pos_skip, batch_skip = data_skip.x, data_skip.pos, data_skip.batch
        skip = x_skip if (x_skip is not None and self._skip) else None
        x = knn_interpolate(x, pos, pos_skip, batch, batch_skip, k=self.k, skip=skip)
        out.x = _fused.rows_mlp(self.nn, x)
        copy_from_to(data_skip, out)
        return out


def mp_config(name, feat):
    """conf/models/segmentation/pointnet2.yaml:5-57 resolved for FEAT."""
    if name == "pointnet2":
        return dict(
            down_conv=dict(ratios=[0.2, 0.25], radius=[0.2, 0.4], radius_num_points=[64, 64],
                           down_conv_nn=[[feat + 3, 64, 64, 128], [128 + 3, 128, 128, 256]]),
            up_conv=dict(up_conv_nn=[[1024 + 256, 256, 256], [256 + 128, 256, 128], [128 + feat, 128, 128, 128]],
                         up_k=[1, 3, 3], skip=True),
            innermost=dict(aggr="max", nn=[256 + 3, 256, 512, 1024]),
            mlp_cls=dict(nn=[128, 128, 128, 128, 128], dropout=0.5))
    if name == "pointnet2ms":
        return dict(
            down_conv=dict(ratios=[0.25, 0.25], radius=[[0.1, 0.2, 0.4], [0.4, 0.8]],
                           radius_num_points=[[32, 64, 128], [64, 128]],
                           down_conv_nn=[[feat + 3, 64, 96, 128], [128 * 3 + 3, 128, 196, 256]]),
            up_conv=dict(up_conv_nn=[[1024 + 256 * 2, 256, 256], [256 + 128 * 3, 128, 128], [128 + feat, 128, 128]],
                         up_k=[1, 3, 3], skip=True),
            innermost=dict(aggr="max", nn=[256 * 2 + 3, 256, 512, 1024]),
            mlp_cls=dict(nn=[128, 128, 128, 128, 128], dropout=0.5))
    raise ValueError("unknown message-passing PointNet++ config %r" % name)


class _UnetBlock(nn.Module):
    """UnetSkipConnectionBlock (models/base_architectures/unet.py:244-306): down -> submodule -> up over (result, input),
    or, innermost, inner -> up."""

    def __init__(self, up, down=None, submodule=None, inner=None):
        super().__init__()
        self.innermost = inner is not None
        if self.innermost:
            self.inner = inner
            self.up = up
        else:
            self.down = down
            self.submodule = submodule
            self.up = up

    def forward(self, data):
        if self.innermost:
            return self.up((self.inner(data), data))
        return self.up((self.submodule(self.down(data)), data))


class SegmentationMP(nn.Module):
    """The nested network of a message-passing U-Net: down module x n, GlobalBaseModule, FPModule x (n + 1), and the
    Segmentation_MP head.  cfg: the YAML's fields, numbers already resolved (down_conv: its down_conv_nn counts the
    levels; up_conv: up_conv_nn, up_k, skip; innermost: aggr, nn; mlp_cls: nn, dropout); make_down(i) builds the down
    module of level i.  forward(data) -> log-probabilities (N, num_classes); data carries pos (N,3), x and a sorted
    batch (N)."""

    def __init__(self, cfg, num_classes, make_down):
        super().__init__()
        up, inner, head = cfg["up_conv"], cfg["innermost"], cfg["mlp_cls"]
        n = len(cfg["down_conv"]["down_conv_nn"])
        if n + 1 != len(up["up_conv_nn"]):
            raise ValueError("up_conv_nn must list one module more than down_conv_nn (the innermost block's)")

        def fp(j):
            return FPModule(up_k=up["up_k"][j], up_conv_nn=up["up_conv_nn"][j], skip=up.get("skip", True), index=j)

        block = _UnetBlock(fp(0), inner=GlobalBaseModule(nn=inner["nn"], aggr=inner.get("aggr", "max")))
        for index in range(n - 1, -1, -1):  # the deepest level is nested first; the last one built is the input level
            block = _UnetBlock(fp(n - index), down=make_down(index), submodule=block)
        self.model = block
        widths = head["nn"]
        self.dropout = head.get("dropout")
        self.lin1 = nn.Linear(widths[0], widths[1])
        self.lin2 = nn.Linear(widths[2], widths[3])
        self.lin3 = nn.Linear(widths[4], num_classes)

    def forward(self, data):
        data = self.model(data)
        p = self.dropout or 0.0
        x = F.relu(self.lin1(data.x))
        x = F.dropout(x, p=p, training=bool(self.training))
        x = self.lin2(x)
        x = F.dropout(x, p=p, training=bool(self.training))
        x = self.lin3(x)
        return F.log_softmax(x, dim=-1)


class PointNet2MP(SegmentationMP):
    """PointNet2_MP segmentation network: SegmentationMP over SAModule.

    cfg: a config name of mp_config ("pointnet2", "pointnet2ms") or a dict with the YAML's fields (down_conv: ratios,
    radius, radius_num_points, down_conv_nn; the rest as SegmentationMP).  data.x is (N, input_nc)."""

    def __init__(self, cfg, input_nc, num_classes):
        if isinstance(cfg, str):
            cfg = mp_config(cfg, input_nc)
        down = cfg["down_conv"]
        super().__init__(cfg, num_classes, lambda i: SAModule(
            ratio=down["ratios"][i], radius=down["radius"][i], radius_num_point=down["radius_num_points"][i],
            down_conv_nn=down["down_conv_nn"][i], index=i))
