"""PointNet ("PointNet: Deep Learning on Point Sets for 3D Classification and Segmentation") on ragged batches.

Mirrors torch_points3d/modules/PointNet/modules.py (`MiniPointNet`, `PointNetSTN3D`, `PointNetSTNkD`, `PointNetSeg`),
core/common_modules/spatial_transform.py (`BaseLinearTransformSTNkD`) and the two models of
models/segmentation/pointnet.py over conf/models/segmentation/pointnet.yaml (`PointNet`, `PointNet_Features` =
`SegPointNetModel`): same constructor arguments, attribute names (hence state_dict keys) and defaults.  `batch_size` is
accepted and ignored: the identity is added for the number of clouds at hand.

Most of the network is shared MLPs over rows (`fused.rows_mlp`).  The three places where the reference builds a per-point
copy of a per-cloud tensor are one HIP kernel each way (csrc/segment_rows.hip, `torchpoints.segment_transform`,
`segment_broadcast_cat`, `segment_mean_rows`): the transform is applied from the cloud's matrix in LDS instead of
`bmm(x.view(N, 1, k), trans[batch])`, the global feature goes back to the points in the pass that concatenates it, and
the backward passes are fixed-order sums instead of `index_add`.  k <= 64.

What has one row per cloud -- `global_nn` and `fc_layer` -- runs as the torch modules on both paths, on purpose: it is a
few rows of work, and a training-mode BatchNorm over B rows divides by a B-sample deviation (0.03 .. 0.9 on a
three-cloud batch) and so multiplies whatever rounding the GEMM in front of it leaves.  Measured there at 3 rows,
64 -> 32: `fused.rows_seq` ends 1.1e-3 from the float64 block, torch's fp32 modules 4.5e-6 (the fused layer kernels are
built and tested for many rows, where this factor is near 1).

`fused=False` runs the plain-torch composition (`trans[batch]`, `g[batch]`, `torch.cat`, the modules themselves; the two
gathers written as `index_select`, whose backward is `index_add`: ATen's backward of advanced indexing reads past the end
of its index buffer on this ROCm build, DESIGN.md "The intermittent abort"); it
also runs on the CPU, which is how tests/test_pointnet_cpu.py pins this file to the reference's tensors.  The batch
vector must be sorted on both paths.  A dense input (B, n, C) is served on the fused path as B clouds of n rows.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused as _fused
from . import torchpoints as tp
from .kpconv_losses import internal_loss
from .partial_dense import MLP

IGNORE_LABEL = -1  # torch_points3d/datasets/segmentation/__init__.py


def _clouds(batch, seg=None):
    """(seg (B + 1,), B) of a sorted batch vector (cached per tensor; raises on an unsorted one)"""
    if seg is not None:
        return seg, seg.numel() - 1
    if batch is None:
        raise ValueError("a ragged input needs its batch vector")
    seg, B, _ = tp._segments(batch if batch.dtype == torch.int64 else batch.long())
    return seg, B


def _dense_seg(x):
    B, n = x.shape[:2]
    return torch.arange(B + 1, dtype=torch.int64, device=x.device) * n


def _pool_torch(x, batch, B, aggr):
    """global_max_pool / global_mean_pool in plain torch (empty clouds give zeros)"""
    if aggr == "max":
        return x.new_zeros((B, x.shape[1])).scatter_reduce(0, batch[:, None].expand_as(x), x, "amax", include_self=False)
    counts = torch.bincount(batch, minlength=B).clamp(min=1).to(x.dtype)
    return x.new_zeros((B, x.shape[1])).index_add(0, batch, x) / counts[:, None]


class MiniPointNet(nn.Module):
    """local_nn over the rows -> max / mean over each cloud -> global_nn (modules.py:9-36)."""

    def __init__(self, local_nn, global_nn, aggr="max", return_local_out=False, fused=True):
        super().__init__()
        self._local_nn = MLP(local_nn)
        self._global_nn = MLP(global_nn) if global_nn else None
        self._aggr = aggr
        self.return_local_out = return_local_out
        self.fused = fused

    def _mlp(self, mlp, x):
        return _fused.rows_mlp(mlp, x) if self.fused else mlp(x)

    def g_pool(self, x, batch, seg=None):
        seg, B = _clouds(batch, seg)
        if not self.fused:
            return _pool_torch(x, batch, B, self._aggr)
        return tp.segment_max(x, seg) if self._aggr == "max" else tp.segment_mean_rows(x, seg)

    def forward(self, x, batch, seg=None):
        if x.dim() == 3 and self.fused:
            B, n = x.shape[:2]
            out = self.forward(x.reshape(B * n, -1), None, seg=_dense_seg(x))
            return (out[0], out[1].view(B, n, -1)) if self.return_local_out else out
        y = x = self._mlp(self._local_nn, x)
        if x.dim() == 3:
            x = x.max(1)[0] if self._aggr == "max" else x.mean(1)
        else:
            x = self.g_pool(x, batch, seg)
        if self._global_nn:
            x = self._global_nn(x)  # one row per cloud: the modules themselves on both paths (module docstring)
        if self.return_local_out:
            return x, y
        return x

    def forward_embedding(self, pos, batch, seg=None):
        global_feat, local_feat = self.forward(pos, batch, seg=seg)
        if self.fused:
            return tp.segment_broadcast_cat(local_feat, global_feat, batch=batch, seg=seg)
        return torch.cat([local_feat, global_feat.index_select(0, batch)], -1)


class BaseLinearTransformSTNkD(nn.Module):
    """STN which learns a k-dimensional linear transformation (spatial_transform.py:5-65): `nn` regresses feat_x to a
    global feature per cloud, the zero-initialised `fc_layer` turns it into a k x k matrix, the identity is added, and the
    first k columns of trans_x are multiplied by their cloud's matrix.  `self.trans` (B, k, k) is kept for the loss."""

    def __init__(self, nn_, nn_feat_size, k=3, batch_size=1, fused=True):
        super().__init__()
        self.nn = nn_
        self.k = k
        self.batch_size = batch_size
        self.fused = fused
        self.fc_layer = nn.Linear(nn_feat_size, k * k)
        nn.init.constant_(self.fc_layer.weight, 0)
        nn.init.constant_(self.fc_layer.bias, 0)
        self.register_buffer("identity", torch.eye(k).view(1, k * k), persistent=False)

    def forward(self, feat_x, trans_x, batch, seg=None):
        if self.fused and self.k > tp.SEG_MAX_K:
            raise NotImplementedError("the fused spatial transformer serves k <= %d (the k x k matrix of a cloud is held in "
                                      "LDS), got k = %d; fused=False runs the plain-torch composition"
                                      % (tp.SEG_MAX_K, self.k))
        global_feature = self.nn(feat_x, batch) if seg is None else self.nn(feat_x, batch, seg=seg)
        trans = self.fc_layer(global_feature)
        trans = trans + self.identity.to(trans.dtype)  # needed so that the transform is initialised to the identity
        trans = trans.view(-1, self.k, self.k)
        self.trans = trans
        k = self.k
        if self.fused:
            if trans_x.dim() == 3:
                return tp.segment_transform(trans_x, trans)
            return tp.segment_transform(trans_x, trans, batch=None if seg is not None else batch, seg=seg)
        if trans_x.dim() == 2:
            x_transformed = torch.bmm(trans_x[:, None, :k], trans.index_select(0, batch))[:, 0]
        else:
            x_transformed = torch.bmm(trans_x[:, :, :k], trans)
        if trans_x.shape[-1] > k:
            x_transformed = torch.cat([x_transformed, trans_x[..., k:]], dim=-1)
        return x_transformed

    def get_orthogonal_regularization_loss(self):
        return torch.mean(torch.norm(
            torch.bmm(self.trans, self.trans.transpose(2, 1)) - self.identity.to(self.trans.dtype).view(-1, self.k, self.k),
            dim=(1, 2)))


class PointNetSTN3D(BaseLinearTransformSTNkD):
    def __init__(self, local_nn=[3, 64, 128, 1024], global_nn=[1024, 512, 256], batch_size=1, fused=True):
        super().__init__(MiniPointNet(local_nn, global_nn, fused=fused), global_nn[-1], 3, batch_size, fused=fused)

    def forward(self, x, batch, seg=None):
        return super().forward(x, x, batch, seg=seg)


class PointNetSTNkD(BaseLinearTransformSTNkD):
    def __init__(self, k=64, local_nn=[64, 64, 128, 1024], global_nn=[1024, 512, 256], batch_size=1, fused=True):
        super().__init__(MiniPointNet(local_nn, global_nn, fused=fused), global_nn[-1], k, batch_size, fused=fused)

    def forward(self, x, batch, seg=None):
        return super().forward(x, x, batch, seg=seg)

    def get_internal_losses(self):
        return {"orthogonal_regularization_loss": self.get_orthogonal_regularization_loss()}


class PointNetSeg(nn.Module):
    """input STN -> local_nn_1 -> feature STN -> local_nn_2 -> max over each cloud -> cat([features, global[batch]]) ->
    seg_nn (modules.py:58-114).  forward(x (N, input_nc), batch (N) sorted) -> (N, seg_nn[-1]) scores; x (B, n, input_nc)
    is the dense layout (batch is not read).  `record`: a dict that receives every stage's tensor."""

    def __init__(self, input_nc=3, input_stn_local_nn=[64, 128, 1024], input_stn_global_nn=[1024, 512, 256],
                 local_nn_1=[64, 64], feat_stn_k=64, feat_stn_local_nn=[64, 64, 128, 1024],
                 feat_stn_global_nn=[1024, 512, 256], local_nn_2=[64, 64, 128, 1024], seg_nn=[1088, 512, 256, 128, 4],
                 batch_size=1, *args, fused=True, **kwargs):
        super().__init__()
        self.batch_size = batch_size
        self.fused = fused
        self.input_stn = PointNetSTN3D([input_nc] + list(input_stn_local_nn), list(input_stn_global_nn), batch_size, fused=fused)
        self.local_nn_1 = MLP([input_nc] + list(local_nn_1))
        self.feat_stn = PointNetSTNkD(feat_stn_k, list(feat_stn_local_nn), list(feat_stn_global_nn), batch_size, fused=fused)
        self.local_nn_2 = MLP(list(local_nn_2))
        self.seg_nn = MLP(list(seg_nn))
        self._use_scatter_pooling = True

    def set_scatter_pooling(self, use_scatter_pooling):
        self._use_scatter_pooling = use_scatter_pooling

    def _mlp(self, mlp, x):
        return _fused.rows_mlp(mlp, x) if self.fused else mlp(x)

    def func_global_max_pooling(self, x, batch, seg=None):
        if x.dim() == 3:
            return x.max(1)[0]
        seg, B = _clouds(batch, seg)
        return tp.segment_max(x, seg) if self.fused else _pool_torch(x, batch, B, "max")

    def forward(self, x, batch, seg=None, record=None):
        rec = record if record is not None else {}
        if x.dim() == 3 and self.fused:
            B, n = x.shape[:2]
            out = self.forward(x.reshape(B * n, -1), None, seg=_dense_seg(x), record=record)
            return out.view(B, n, -1)
        if x.dim() == 2:
            seg, _ = _clouds(batch, seg)
        rec["x_input_stn"] = x = self.input_stn(x, batch, seg=seg)
        rec["x_local_nn_1"] = x = self._mlp(self.local_nn_1, x)
        rec["x_feat_stn"] = x_feat_trans = self.feat_stn(x, batch, seg=seg)
        rec["x_local_nn_2"] = x3 = self._mlp(self.local_nn_2, x_feat_trans)
        rec["global_feature"] = global_feature = self.func_global_max_pooling(x3, batch, seg)
        if x_feat_trans.dim() != 2:
            feat_concat = torch.cat([x_feat_trans, global_feature.unsqueeze(1).repeat((1, x_feat_trans.shape[1], 1))], dim=-1)
        elif self.fused:
            feat_concat = tp.segment_broadcast_cat(x_feat_trans, global_feature, seg=seg)
        else:
            feat_concat = torch.cat([x_feat_trans, global_feature.index_select(0, batch)], dim=1)
        rec["x_concat"] = feat_concat
        rec["out"] = out = self._mlp(self.seg_nn, feat_concat)
        return out


_YAML = dict(input_stn=dict(local_nn=[64, 128, 1024], global_nn=[1024, 512, 256]), local_nn_1=[64, 64],
             feat_stn=dict(k=64, local_nn=[64, 64, 128, 1024], global_nn=[1024, 512, 256]), local_nn_2=[64, 64, 128, 1024],
             seg_nn=[1024 + 64, 512, 256, 128])  # conf/models/segmentation/pointnet.yaml, `PointNet`


def _flatten(opts):
    """utils/model_building_utils/resolver_utils.flatten_dict: {"a": {"b": v}} -> {"a_b": v}"""
    out = {}
    for key, value in opts.items():
        if isinstance(value, dict):
            for sub, v in _flatten(value).items():
                out[key + "_" + sub] = v
        else:
            out[key] = value
    return out


class PointNet(nn.Module):
    """The `PointNet` model of models/segmentation/pointnet.py:15-67 without `BaseModel`: `pointnet_seg` over
    cat([pos, x]) (input_nc feature channels + 3), the YAML's widths unless overridden by keyword (nested as in the YAML or
    flattened: `feat_stn=dict(k=16, ...)` or `feat_stn_k=16`).  forward(data with pos, x or None, batch) -> (N, num_classes)
    scores; compute_loss(labels) = cross entropy (IGNORE_LABEL ignored) + 0.001 x the internal (orthogonality) loss."""

    def __init__(self, input_nc, num_classes, fused=True, **yaml_overrides):
        super().__init__()
        opts = _flatten(_YAML)
        opts["seg_nn"] = list(opts["seg_nn"]) + [num_classes]
        opts.update(_flatten(yaml_overrides))
        self.pointnet_seg = PointNetSeg(input_nc=input_nc + 3, fused=fused, **opts)
        self.loss_names = ["loss_seg", "loss_internal"]

    def forward(self, data):
        x = getattr(data, "x", None)
        self.input_features = torch.cat([data.pos, x], dim=-1) if x is not None else data.pos
        self.pointnet_seg.set_scatter_pooling(self.input_features.dim() == 2)
        self.output = self.pointnet_seg(self.input_features, getattr(data, "batch", None))
        return self.output

    def compute_loss(self, labels):
        self.loss_seg = F.cross_entropy(self.output, labels, ignore_index=IGNORE_LABEL)
        self.loss_internal = internal_loss(self) * 0.001
        self.loss = self.loss_seg + self.loss_internal
        return self.loss


class SegPointNetModel(nn.Module):
    """`PointNet_Features` (models/segmentation/pointnet.py:70-101): a MiniPointNet embedding, `seg_nn`, log-softmax.
    pointnet_opts: local_nn, global_nn, aggr, return_local_out (the YAML's `pointnet` block)."""

    def __init__(self, pointnet_opts, seg_nn, fused=True):
        super().__init__()
        self.fused = fused
        self.pointnet_seg = MiniPointNet(list(pointnet_opts["local_nn"]), list(pointnet_opts["global_nn"]),
                                         aggr=pointnet_opts.get("aggr", "max"),
                                         return_local_out=pointnet_opts.get("return_local_out", True), fused=fused)
        self.seg_nn = MLP(list(seg_nn))

    def forward(self, pos, batch):
        x = self.pointnet_seg.forward_embedding(pos, batch)
        x = _fused.rows_mlp(self.seg_nn, x) if self.fused else self.seg_nn(x)
        self.output = F.log_softmax(x, dim=-1)
        return self.output

    def compute_loss(self, labels):
        self.loss = F.nll_loss(self.output, labels)
        return self.loss
