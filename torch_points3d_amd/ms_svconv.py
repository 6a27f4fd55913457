"""MS-SVConv (reference torch_points3d/models/registration/ms_svconv3d.py and models/segmentation/ms_svconv3d.py, the 15 + 1
entries of conf/models/{registration,segmentation}/ms_svconv_base.yaml) on the device.

  voxelize              UnetMSparseConv3d._prepare_data over grid_sampling.voxel_cluster: coords = round(pos / grid_size) (half
                        to even), voxel ids ascending in (batch, z, y, x), the highest point index of every voxel -- what the
                        reference builds from torch.round, voxel_grid(coords, batch, 1) and consecutive_cluster
  UnetMSparseConv3d     pointnet / add_pos -> voxelize -> pre_mlp -> SparseConv3dUnet over the option dict (its first layer is
                        sparseconv.WideConv3d, kernel_size 5) -> torchpoints.gather_rows(x, cluster) -> post_mlp
  MS_SparseConv3d, MS_SparseConv3d_Shared, MS_SparseConv3d_Shared_Pool, MS_SparseConvModel
                        the multi-scale head on torchpoints.scale_fuse (one launch each way), FC_layer, final normalisation;
                        "match" mode loss in the style of registration.FragmentDescriptor
  ms_svconv_config      the resolved numbers of the 16 YAML entries
  build                 the model of one YAML entry with its loss

Constructors take plain Python arguments.  Attribute names are the reference's (`unet`, `pre_mlp`, `pointnet`, `post_mlp`,
`FC_layer`, `head`), hence the state_dict keys.  Not served: the `minkowski` backend, loss_mode other than "match", and the
miners of pytorch_metric_learning.
"""
import copy

import torch
import torch.nn.functional as F
from torch import nn

from . import grid_sampling
from . import torchpoints as tp
from .kpconv_blocks import FastBatchNorm1d
from .sparseconv import Seq, SparseConv3dUnet, SparseTensor

IGNORE_LABEL = -1  # torch_points3d/datasets/segmentation/__init__.py


def MLP(channels, activation=None, bn_momentum=0.1, bias=True):
    """core/common_modules/base_modules.py MLP: Linear (with bias) - FastBatchNorm1d - LeakyReLU(0.2) per step"""
    return nn.Sequential(*[nn.Sequential(nn.Linear(channels[i - 1], channels[i], bias=bias),
                                         FastBatchNorm1d(channels[i], momentum=bn_momentum),
                                         nn.LeakyReLU(0.2) if activation is None else activation)
                           for i in range(1, len(channels))])


class _ClusterMean(torch.autograd.Function):
    """scatter_mean over the voxels (grid_sampling.cluster_mean: members summed in ascending point order); the gradient of
    a point is its voxel's row over the voxel's size -- a gather, no atomics"""

    @staticmethod
    def forward(ctx, x, cluster, order, cluster_start):
        ctx.save_for_backward(cluster, cluster_start)
        return grid_sampling.cluster_mean(x, order, cluster_start)

    @staticmethod
    def backward(ctx, g):
        cluster, start = ctx.saved_tensors
        count = (start[1:] - start[:-1]).to(g.dtype).unsqueeze(1)
        return (g / count)[cluster], None, None, None


class Voxels(object):
    """one voxelisation: coords (K, 3) int64, batch (K,), pos (K, 3), x (K, C), cluster (N,), unique_pos_indices (K,)"""

    __slots__ = ("coords", "batch", "pos", "x", "cluster", "unique_pos_indices")

    def __init__(self, coords, batch, pos, x, cluster, unique_pos_indices):
        self.coords, self.batch, self.pos, self.x = coords, batch, pos, x
        self.cluster, self.unique_pos_indices = cluster, unique_pos_indices


def voxelize(pos, batch, grid_size, x, aggr=None):
    """UnetMSparseConv3d._prepare_data on the device.  aggr None: the features of the voxel's representative point
    (unique_pos_indices); "mean": cluster_mean; "max": segment_max over the voxel's members.  Differentiable wrt x."""
    cluster, upi, order, start = grid_sampling.voxel_cluster(pos, batch, grid_size)
    new_pos = pos[upi]
    coords = torch.round(new_pos / grid_size).long()
    if aggr is None:
        xv = tp.gather_rows(x, upi) if x.requires_grad else x[upi]
    elif aggr == "mean":
        xv = _ClusterMean.apply(x, cluster, order, start)
    elif aggr == "max":
        xv = tp.segment_max(tp.gather_rows(x, order) if x.requires_grad else x[order].contiguous(), start)
    else:
        raise NotImplementedError("voxelize: aggr %r (None, 'mean' or 'max')" % (aggr,))
    return Voxels(coords, batch[upi], new_pos, xv, cluster, upi)


def _backbone(down_nn, up_nn, bn_momentum=0.05):
    n = len(down_nn)
    return dict(down_conv=dict(module_name="ResNetDown", dimension=3, down_conv_nn=down_nn, kernel_size=[5] + [3] * (n - 1),
                               stride=[1] + [2] * (n - 1), dilation=[1] * n),
                up_conv=dict(module_name="ResNetUp", dimension=3, bn_momentum=bn_momentum, up_conv_nn=up_nn,
                             kernel_size=[3] * n, stride=[2] * (n - 1) + [1], dilation=[1] * n))


_BASE_GRID = {"B2cm": 0.02, "B4cm": 0.04, "B6cm": 0.06}
REGISTRATION_ENTRIES = ["MS_SVCONV_%s_X2_%s" % (b, h) for b in ("B2cm", "B4cm", "B6cm")
                        for h in ("1head", "2head", "3head", "3head_unshared", "4head")]
SEGMENTATION_ENTRY = "segmentation/MS_SVCONV_B4cm_X2_3head"


def ms_svconv_config(name, input_nc=1):
    """The resolved numbers of conf/models/registration/ms_svconv_base.yaml (15 entries, by their name) and of the one entry
    of conf/models/segmentation/ms_svconv_base.yaml ("segmentation/MS_SVCONV_B4cm_X2_3head"); FEAT = input_nc."""
    seg = name == SEGMENTATION_ENTRY
    short = name.split("/")[-1]
    if not seg and name not in REGISTRATION_ENTRIES:
        raise ValueError("unknown MS-SVConv configuration %r" % (name,))
    parts = short.split("_")  # MS, SVCONV, B<size>cm, X2, <scales>head[, unshared]
    base, heads = parts[2], "_".join(parts[4:])
    scales = int(heads[0])
    out_feat = 32
    cfg = dict(
        cls="MS_SparseConvModel" if seg else ("MS_SparseConv3d" if heads.endswith("unshared") else "MS_SparseConv3d_Shared"),
        backend="torchsparse", normalize_feature=True,
        option_unet=dict(input_nc=input_nc, num_scales=scales, grid_size=[_BASE_GRID[base] * 2 ** i for i in range(scales)],
                         post_mlp_nn=[64, out_feat],
                         backbone=_backbone([[input_nc, 32], [32, 64], [64, 128], [128, 256]],
                                            [[256, 64], [192, 64], [128, 64], [96, 64]])),
        mlp_cls=dict(nn=[scales * out_feat, out_feat, out_feat], bn_momentum=0.05))
    if seg:
        cfg["output_nc"] = out_feat
    else:
        cfg["loss_mode"] = "match"
        cfg["metric_loss"] = {"class": "ContrastiveHardestNegativeLoss",
                              "params": dict(num_pos=1024, num_hn_samples=256, pos_thresh=0.1, neg_thresh=1.4)}
    return cfg


class UnetMSparseConv3d(nn.Module):
    """forward(data) -> (N, post_mlp_nn[-1]) per-point features; data has pos (N, 3), batch (N,) and x (N, input_nc).
    `last` keeps the Voxels of the latest call."""

    def __init__(self, backbone, input_nc=1, grid_size=0.05, pointnet_nn=None, pre_mlp_nn=None, post_mlp_nn=[64, 64, 32],
                 add_pos=False, add_pre_x=False, backend="torchsparse", aggr=None):
        super().__init__()
        if backend != "torchsparse":
            raise NotImplementedError("UnetMSparseConv3d: backend %r is not served (only 'torchsparse')" % (backend,))
        if input_nc is None:
            input_nc = 1
        self.unet = SparseConv3dUnet(copy.deepcopy(backbone), input_nc=input_nc)
        self.pre_mlp = MLP(pre_mlp_nn) if pre_mlp_nn is not None else nn.Identity()
        self.pointnet = MLP(pointnet_nn) if pointnet_nn is not None else nn.Identity()
        self.post_mlp = MLP(post_mlp_nn)
        self._grid_size = grid_size
        self.add_pos = add_pos
        self.add_pre_x = add_pre_x
        self.aggr = aggr
        self.last = None

    def set_grid_size(self, grid_size):
        self._grid_size = grid_size

    def forward(self, data, **kwargs):
        pos, batch = data.pos, data.batch
        centred = pos - pos.mean(0) if self.add_pos else None
        x = self.pointnet(torch.cat([data.x, centred], 1) if self.add_pos else data.x)
        pre_x = x
        v = self.last = voxelize(pos, batch, self._grid_size, x, self.aggr)
        feats = self.pre_mlp(v.x)
        coords = torch.cat([v.coords.int(), v.batch.int().unsqueeze(1)], 1)
        out = tp.gather_rows(self.unet(SparseTensor(feats, coords)), v.cluster)
        if self.add_pos:
            out = torch.cat([out, centred], 1)
        if self.add_pre_x:
            out = torch.cat([out, pre_x], 1)
        return self.post_mlp(out)


def _fc_layer(widths, bn_momentum, dropout=None):
    fc = Seq()
    for i in range(1, len(widths)):
        fc.append(nn.Sequential(nn.Linear(widths[i - 1], widths[i], bias=False),
                                FastBatchNorm1d(widths[i], momentum=bn_momentum), nn.LeakyReLU(0.2)))
    if dropout is not None:
        fc.append(nn.Dropout(p=dropout))
    return fc


def _normalize(x, eps=1e-20):
    return tp.scale_fuse([x], "cat", eps=eps)


class _BaseMS(nn.Module):
    """shared by the registration classes: forward(data, data_target=None, match=None) as FragmentDescriptor"""

    pool_mode = "cat"

    def _init_head(self, option_unet, mlp_cls, normalize_feature, loss_mode, metric_loss, backend):
        if loss_mode != "match":
            raise NotImplementedError("MS-SVConv: loss_mode %r is not served (only 'match')" % (loss_mode,))
        if backend != "torchsparse":
            raise NotImplementedError("MS-SVConv: backend %r is not served (only 'torchsparse')" % (backend,))
        self.mode = loss_mode
        self.normalize_feature = normalize_feature
        self.grid_size = list(option_unet["grid_size"])
        self.FC_layer = _fc_layer(mlp_cls["nn"], mlp_cls["bn_momentum"], mlp_cls.get("dropout"))
        self.metric_loss_module = metric_loss
        self.output = self.output_target = self.loss = None

    @staticmethod
    def _unet(option_unet, grid_size):
        o = option_unet
        return UnetMSparseConv3d(o["backbone"], input_nc=o.get("input_nc", 1), grid_size=grid_size,
                                 pointnet_nn=o.get("pointnet_nn"), post_mlp_nn=o.get("post_mlp_nn", [64, 64, 32]),
                                 pre_mlp_nn=o.get("pre_mlp_nn"), add_pos=o.get("add_pos", False),
                                 add_pre_x=o.get("add_pre_x", False), aggr=o.get("aggr"))

    def _scale_features(self, data):
        raise NotImplementedError

    def apply_nn(self, data):
        """-> (descriptors (N, mlp_cls nn[-1]), the S normalised per-scale outputs)"""
        fused, scales = tp.scale_fuse(self._scale_features(data), self.pool_mode, eps=1e-20, return_scales=True)
        out = self.FC_layer(fused)
        if self.normalize_feature:
            out = _normalize(out)
        return out, scales

    def compute_intermediate_loss(self, outputs, outputs_target, data, data_target, match, loss_kwargs=None):
        pass

    def forward(self, data, data_target=None, match=None, loss_kwargs=None, int_loss_kwargs=None):
        """`output`; with a target and `match` (M, 2) also `output_target` and `loss`.  loss_kwargs: keyword arguments of the
        metric loss (the drawn selections of ContrastiveHardestNegativeLoss: sel0, sel1, pos_sel); int_loss_kwargs: one such
        dict per intermediate loss."""
        self.output, outputs = self.apply_nn(data)
        self.outputs, self.outputs_target = outputs, None
        self.output_target = self.loss = None
        if data_target is None or match is None:
            return self.output
        self.output_target, self.outputs_target = self.apply_nn(data_target)
        if self.metric_loss_module is None:
            raise ValueError("a target and matches were given but the model has no metric_loss")
        self.loss = self.metric_loss_module(self.output, self.output_target, match[:, :2], data.pos, data_target.pos,
                                            **(loss_kwargs or {}))
        self.compute_intermediate_loss(outputs, self.outputs_target, data, data_target, match, int_loss_kwargs)
        return self.output

    def get_output(self):
        return self.output, self.output_target


class MS_SparseConv3d(_BaseMS):
    """one UnetMSparseConv3d per scale (`unet.<i>`), their normalised outputs concatenated"""

    def __init__(self, option_unet, mlp_cls, normalize_feature=True, loss_mode="match", metric_loss=None, backend="torchsparse"):
        super().__init__()
        self._init_head(option_unet, mlp_cls, normalize_feature, loss_mode, metric_loss, backend)
        self.unet = nn.ModuleList(self._unet(option_unet, g) for g in self.grid_size)

    def _scale_features(self, data):
        return [net(data) for net in self.unet]


class MS_SparseConv3d_Shared(_BaseMS):
    """one UnetMSparseConv3d run at every grid size; intermediate_loss = dict(metric_loss=module, weights=[...]) adds
    weights[i] * metric_loss(scale i's outputs) to the loss (`loss_intermediate_loss_<i>`)"""

    def __init__(self, option_unet, mlp_cls, normalize_feature=True, loss_mode="match", metric_loss=None, intermediate_loss=None,
                 backend="torchsparse"):
        super().__init__()
        self._init_head(option_unet, mlp_cls, normalize_feature, loss_mode, metric_loss, backend)
        self.unet = self._unet(option_unet, self.grid_size[0])
        self.voxels = []
        if intermediate_loss is not None:
            self.int_metric_loss = intermediate_loss["metric_loss"]
            self.int_weights = list(intermediate_loss["weights"])
        else:
            self.int_metric_loss = None

    def _scale_features(self, data):
        outs, self.voxels = [], []
        for g in self.grid_size:
            self.unet.set_grid_size(g)
            outs.append(self.unet(data))
            self.voxels.append(self.unet.last)
        return outs

    def compute_intermediate_loss(self, outputs, outputs_target, data, data_target, match, loss_kwargs=None):
        assert len(outputs) == len(outputs_target)
        if self.int_metric_loss is None:
            return
        assert len(outputs) == len(self.int_weights)
        for i, w in enumerate(self.int_weights):
            kw = {} if loss_kwargs is None else loss_kwargs[i]
            loss_i = self.int_metric_loss(outputs[i], outputs_target[i], match[:, :2], data.pos, data_target.pos, **kw)
            self.loss = self.loss + w * loss_i
            setattr(self, "loss_intermediate_loss_{}".format(i), loss_i)


class MS_SparseConv3d_Shared_Pool(MS_SparseConv3d_Shared):
    """the normalised scales max- or mean-pooled instead of concatenated"""

    def __init__(self, option_unet, mlp_cls, pool_mode="max", **kwargs):
        super().__init__(option_unet, mlp_cls, **kwargs)
        if pool_mode not in ("max", "mean"):
            raise NotImplementedError("pool_mode %r ('max' or 'mean')" % (pool_mode,))
        self.pool_mode = pool_mode


class MS_SparseConvModel(nn.Module):
    """segmentation: the shared multi-scale descriptor, `head` = Sequential(Linear(output_nc, num_classes)), log_softmax,
    nll_loss with the ignore label.  forward(data, labels=None) -> log-probabilities (N, num_classes); `loss_seg`."""

    def __init__(self, option_unet, mlp_cls, output_nc, num_classes, normalize_feature=True, backend="torchsparse"):
        super().__init__()
        if backend != "torchsparse":
            raise NotImplementedError("MS-SVConv: backend %r is not served (only 'torchsparse')" % (backend,))
        self.normalize_feature = normalize_feature
        self.grid_size = list(option_unet["grid_size"])
        self.unet = _BaseMS._unet(option_unet, self.grid_size[0])
        if mlp_cls is not None:
            self.FC_layer = _fc_layer(mlp_cls["nn"], mlp_cls["bn_momentum"], mlp_cls.get("dropout"))
        else:
            self.FC_layer = nn.Identity()
        self.head = nn.Sequential(nn.Linear(output_nc, num_classes))
        self.output = self.loss_seg = None

    def apply_nn(self, data):
        outs = []
        for g in self.grid_size:
            self.unet.set_grid_size(g)
            outs.append(self.unet(data))
        fused, scales = tp.scale_fuse(outs, "cat", eps=1e-20, return_scales=True)
        out = self.FC_layer(fused)
        if self.normalize_feature:
            out = _normalize(out)
        return self.head(out), scales

    def forward(self, data, labels=None):
        logits, _ = self.apply_nn(data)
        self.output = F.log_softmax(logits, dim=-1)
        self.loss_seg = None
        if labels is not None:
            self.loss_seg = F.nll_loss(self.output, labels, ignore_index=IGNORE_LABEL)
        return self.output


def build(name, input_nc=1, num_classes=None, metric_loss=None, **kwargs):
    """the model of one YAML entry (ms_svconv_config(name)); metric_loss defaults to the entry's
    ContrastiveHardestNegativeLoss"""
    cfg = ms_svconv_config(name, input_nc)
    if cfg["cls"] == "MS_SparseConvModel":
        return MS_SparseConvModel(cfg["option_unet"], cfg["mlp_cls"], cfg["output_nc"], num_classes, cfg["normalize_feature"])
    if metric_loss is None:
        from .registration import ContrastiveHardestNegativeLoss
        p = cfg["metric_loss"]["params"]
        metric_loss = ContrastiveHardestNegativeLoss(p["pos_thresh"], p["neg_thresh"], p["num_pos"], p["num_hn_samples"])
    cls = MS_SparseConv3d if cfg["cls"] == "MS_SparseConv3d" else MS_SparseConv3d_Shared
    return cls(cfg["option_unet"], cfg["mlp_cls"], cfg["normalize_feature"], cfg["loss_mode"], metric_loss, **kwargs)
