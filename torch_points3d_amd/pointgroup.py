"""PointGroup (reference torch_points3d/models/panoptic/pointgroup.py, structures.py, core/losses/panoptic_losses.py) on
the device, from the backbone to the scored proposals.

Everything after the heads works on the CSR form of the clusters (torchpoints.ClusterSet): there is no per-cluster Python
loop and no dense (clusters, N) mask.
  region_grow          the reference's signature and list result, through torchpoints.region_grow_csr (HIP region growing)
  cluster              the two region_grow calls of PointGroup._cluster as one ClusterSet plus cluster_type
  instance_iou_csr     torch_points_kernels.instance_iou on the CSR
  offset_loss, instance_iou_loss   restatements of core/losses/panoptic_losses.py
  PanopticResults, PanopticLabels  the reference's structures; `clusters` may be a ClusterSet
  PointGroup           backbone -> Semantic / Offset heads -> clusters -> a scorer -> ScorerHead (or the semantic certainty)
  pointgroup_config    the resolved numbers of the two entries of conf/models/panoptic/pointgroup.yaml

Served: every scorer_type -- "MLP" and None as they stand, "unet" and "encoder" (a sparse network over one cloud per cluster:
torchpoints.cluster_voxelize builds the tensor, SparseTensor(clouds=K) holds more than 2^9 clouds) when the scorer's config
is handed in (`scorer_unet=` / `scorer_encoder=`, e.g. from pointgroup_config); a call without one is refused as before.  The
sparse scorers are assembled from this library's SparseConv3d family, as the backbone is.  The panoptic tracker is served
by panoptic_metrics.PanopticEvaluator (suppression, instance matching and AP on the device);
PanopticResults.get_instances below stays the host path it was.  Not served: the MinkowskiEngine backends.
"""
from typing import Any, NamedTuple

import numpy as np
import torch
from torch import nn

from . import torchpoints as tp
from .partial_dense import MLP
from .sparseconv import Seq, SparseConv3dEncoder, SparseConv3dUnet
from .torchpoints import ClusterSet

IGNORE_LABEL = -1  # datasets/segmentation/__init__.py:1


def region_grow(pos, labels, batch, ignore_labels=[], radius=0.03, nsample=300, min_cluster_size=10):
    """torch_points_kernels.region_grow for device tensors: a list of LongTensors of point indices, one per cluster, in
    the host path's list order.  Members come in ascending index (the host path lists them in discovery order; the
    reference reads clusters as index sets)."""
    return tp.region_grow_csr(pos, labels, batch, ignore_labels=ignore_labels, radius=radius, nsample=nsample,
                              min_cluster_size=min_cluster_size).to_list()


def cluster(pos, votes, labels, batch, stuff, radius):
    """PointGroup._cluster (pointgroup.py:98-121): the clusters of the positions `pos` (nsample 300) followed by those of
    the voted positions `votes` = pos + predicted offsets (nsample 200), as one ClusterSet, and cluster_type (K,) uint8:
    0 -> original positions, 1 -> votes.  `stuff`: the ignored labels (IGNORE_LABEL and the stuff classes)."""
    on_pos = tp.region_grow_csr(pos, labels, batch, ignore_labels=stuff, radius=radius)
    on_votes = tp.region_grow_csr(votes, labels, batch, ignore_labels=stuff, radius=radius, nsample=200)
    both = ClusterSet.cat([on_pos, on_votes])
    cluster_type = torch.zeros(len(both), dtype=torch.uint8, device=pos.device)
    cluster_type[len(on_pos):] = 1
    return both, cluster_type


def _as_set(clusters, device):
    return clusters if isinstance(clusters, ClusterSet) else ClusterSet.from_list(clusters, device=device)


def instance_iou_csr(clusters, instance_labels, batch):
    """(K, G) intersection over union of every cluster with every ground-truth instance: torch_points_kernels.instance_iou
    on clusters.to_list(), column layout included (instances 1..g_s of cloud s, cloud after cloud), from one bincount over
    the (cluster, instance) pairs of the member slots."""
    dev = instance_labels.device
    gt = instance_labels.long()
    b = batch.long().to(dev)
    nb = int(b.max()) + 1 if b.numel() else 0
    per_cloud = torch.zeros(nb, dtype=torch.long, device=dev)
    if gt.numel():
        per_cloud.scatter_reduce_(0, b, gt, reduce="amax", include_self=True)
    offsets = torch.cumsum(per_cloud, 0) - per_cloud
    G = int(per_cloud.sum()) if nb else 0
    K = len(clusters)
    if K == 0 or G == 0:
        return torch.zeros((K, G), dtype=torch.float32, device=dev)
    column = torch.where(gt > 0, offsets[b] + gt - 1, torch.full_like(gt, -1))
    gt_size = torch.bincount(column[column >= 0], minlength=G).float()
    col = column[clusters.members.to(dev)]
    keep = col >= 0
    inter = torch.bincount(clusters.member_cluster.to(dev)[keep] * G + col[keep], minlength=K * G).view(K, G).float()
    union = clusters.sizes().to(dev).float().unsqueeze(1) + gt_size.unsqueeze(0) - inter
    return inter / union.clamp(min=1.0)


def offset_loss(pred_offsets, gt_offsets, total_instance_points):
    """the two offset terms of PointGroup (equations 2 and 3; core/losses/panoptic_losses.py:6-22): the L1 distance
    between predicted and true offsets, and minus the cosine between them (each vector divided by its norm + 1e-8),
    both summed over the rows and divided by total_instance_points + 1e-6"""
    denom = total_instance_points + 1e-6

    def unit(v):
        return v / (v.norm(p=2, dim=1, keepdim=True) + 1e-8)

    return {"offset_norm_loss": (pred_offsets - gt_offsets).abs().sum() / denom,
            "offset_dir_loss": -(unit(gt_offsets) * unit(pred_offsets)).sum() / denom}


def instance_iou_loss(predicted_clusters, cluster_scores, instance_labels, batch, min_iou_threshold=0.25,
                      max_iou_threshold=0.75):
    """binary cross entropy of the scores against a target made from each cluster's best IoU with an instance
    (PointGroup equation 7; panoptic_losses.py:25-46): 0 below min_iou_threshold, 1 above max_iou_threshold, linear in
    between -- one clamp.  predicted_clusters: a ClusterSet or the reference's list."""
    clusters = _as_set(predicted_clusters, instance_labels.device)
    if len(clusters) != cluster_scores.shape[0]:
        raise ValueError("one score per cluster is needed")
    best = instance_iou_csr(clusters, instance_labels, batch).max(1)[0]
    target = ((best - min_iou_threshold) / (max_iou_threshold - min_iou_threshold)).clamp(0.0, 1.0)
    return torch.nn.functional.binary_cross_entropy(cluster_scores, target)


def non_max_suppression(ious, scores, threshold):
    """greedy suppression over the (K, K) numpy matrix, on the host as in the reference (structures.py:6-16): clusters
    are visited by descending score; one that is still alive is picked and takes out every other whose IoU with it
    exceeds the threshold.  Returns the picked indices in visiting order."""
    alive = np.ones(len(scores), dtype=bool)
    picked = []
    for i in np.argsort(scores)[::-1]:
        if alive[i]:
            picked.append(i)
            alive &= ~(ious[i] > threshold)
    return picked


def cross_iou(clusters):
    """(K, K) IoU of every pair of clusters (structures.py:32-41) from the (point, cluster) pairs: the member slots are
    sorted by point, every run of one point contributes its cluster pairs, one bincount counts them."""
    K = len(clusters)
    dev = clusters.members.device
    point, order = torch.sort(clusters.members, stable=True)
    owner = clusters.member_cluster[order]
    _, run_len = torch.unique_consecutive(point, return_counts=True)
    run_start = torch.cumsum(run_len, 0) - run_len
    slot_len = torch.repeat_interleave(run_len, run_len)       # per slot: the length of its run ...
    slot_start = torch.repeat_interleave(run_start, run_len)   # ... and where the run begins
    left = torch.repeat_interleave(torch.arange(point.numel(), device=dev), slot_len)
    first_pair = torch.cumsum(slot_len, 0) - slot_len
    right = slot_start[left] + (torch.arange(left.numel(), device=dev) - first_pair[left])
    intersection = torch.bincount(owner[left] * K + owner[right], minlength=K * K).view(K, K).float()
    pointnum = clusters.sizes().float()
    return intersection / (pointnum.unsqueeze(-1) + pointnum.unsqueeze(0) - intersection)


class PanopticResults(NamedTuple):
    semantic_logits: torch.Tensor
    offset_logits: torch.Tensor
    cluster_scores: torch.Tensor  # one float value per cluster
    clusters: Any  # ClusterSet, or the reference's list of index tensors
    cluster_type: torch.Tensor  # 0 -> cluster of the original positions, 1 -> of the votes

    def get_instances(self, nms_threshold=0.3, min_cluster_points=100, min_score=0.2):
        """indices of the clusters that pass the suppression, the size test and the score test (structures.py:26-49)"""
        if self.clusters is None or len(self.clusters) == 0:
            return []
        clusters = _as_set(self.clusters, self.semantic_logits.device)
        scores = self.cluster_scores.detach().cpu()
        picked = non_max_suppression(cross_iou(clusters).cpu().numpy(), scores.numpy(), nms_threshold)
        # structures.py:46-47 is kept as the reference behaves: its size test compares the NUMBER OF CLUSTERS, not the
        # size of the picked cluster, with min_cluster_points
        enough = len(self.clusters) > min_cluster_points
        return [i for i in picked if enough and scores[i] > min_score]


class PanopticLabels(NamedTuple):
    center_label: torch.Tensor
    y: torch.Tensor
    num_instances: torch.Tensor
    instance_labels: torch.Tensor
    instance_mask: torch.Tensor
    vote_label: torch.Tensor


def _scorer_config(kind, in_feat, n_blocks):
    """scorer_unet / scorer_encoder of pointgroup.yaml with `in_feat` and `N` filled in (both entries share the shape)"""
    f = in_feat
    cfg = dict(down_conv=dict(module_name="ResNetDown", dimension=3, down_conv_nn=[[f, 2 * f], [2 * f, 4 * f]], kernel_size=3,
                              stride=2, N=n_blocks))
    if kind == "unet":
        cfg["up_conv"] = dict(module_name="ResNetUp", dimension=3, up_conv_nn=[[4 * f, 2 * f], [2 * f + 2 * f, f]], kernel_size=3,
                              stride=2, N=n_blocks)
    else:
        cfg["innermost"] = dict(module_name="GlobalBaseModule", activation=dict(name="LeakyReLU", negative_slope=0.2), aggr="max",
                                nn=[4 * f, f])
    return cfg


def pointgroup_config(name, feat):
    """The resolved numbers of conf/models/panoptic/pointgroup.yaml: `PointGroup` (the default backbone, scorers at in_feat
    96 with one block per stage) or `PointGroup-PAPER` (feat_size 16, two blocks per stage, a 7-level backbone with strides
    [1, 2, 2, 2, 2, 2, 2]); `feat` = FEAT, the dataset's feature dimension.  The `backbone`, `scorer_unet` and
    `scorer_encoder` values are the dicts sparseconv's networks take as `config`; `backbone` is None for the default
    ("unet" without a config: SparseConv3dUnet("unet_4") here, the MinkowskiEngine U-Net in the reference)."""
    common = dict(scorer_type="unet", prepare_epoch=120, min_iou_threshold=0.25, max_iou_threshold=0.75,
                  loss_weights=dict(semantic=1, offset_norm_loss=1, offset_dir_loss=1, score_loss=1))
    if name == "PointGroup":
        return dict(common, backbone=None, scorer_unet=_scorer_config("unet", 96, 1), scorer_encoder=_scorer_config("encoder", 96, 1))
    if name == "PointGroup-PAPER":
        f = 16
        backbone = dict(
            down_conv=dict(module_name="ResNetDown", dimension=3, kernel_size=3, stride=[1, 2, 2, 2, 2, 2, 2], N=2,
                           down_conv_nn=[[feat, f]] + [[i * f, (i + 1) * f] for i in range(1, 7)]),
            up_conv=dict(module_name="ResNetUp", dimension=3, kernel_size=3, stride=[2, 2, 2, 2, 2, 2, 1], N=2,
                         up_conv_nn=[[7 * f, 6 * f]] + [[2 * i * f, (i - 1) * f] for i in range(6, 1, -1)] + [[2 * f, f]]))
        return dict(common, feat_size=f, backbone=backbone, scorer_unet=_scorer_config("unet", f, 2),
                    scorer_encoder=_scorer_config("encoder", f, 2))
    raise ValueError("unknown PointGroup configuration %r (\"PointGroup\" or \"PointGroup-PAPER\")" % (name,))


class PointGroup(nn.Module):
    """PointGroup on the CSR.  `backbone`: any module mapping the batch (x, coords, batch, pos) to (N, C) features with an
    `output_nc` attribute; default SparseConv3dUnet("unet_4", input_nc).  Semantic, Offset, ScorerUnet, ScorerEncoder,
    ScorerMLP and ScorerHead carry the reference's attribute names and layer order (pointgroup.py:41-56).

    scorer_type (the default here stays "MLP"; the reference's is "encoder", its YAML says "unet"):
      "unet"     cluster_voxelize -> ScorerUnet (a SparseConv3dUnet) -> max per cluster (segment_max over the voxel
                 offsets) -> ScorerHead
      "encoder"  cluster_voxelize -> ScorerEncoder (a SparseConv3dEncoder whose innermost max gives one row per cluster) ->
                 ScorerHead
      "MLP"      ScorerMLP on backbone_features[members], max per cluster (segment_max over `starts`), ScorerHead
      None       the mean semantic row per cluster, then its maximum (no gradient, as in the reference)
    scorer_unet / scorer_encoder: the config dict of that network (pointgroup_config(...)["scorer_unet"]).  The sparse
    scorers are opt-in: scorer_type "unet" / "encoder" WITHOUT its config raises NotImplementedError, as every call did
    before these arguments existed -- a sparse tensor holds 2^9 clouds unless it is built with clouds=K, and handing in the
    scorer's config is what asks for that.  Only the scorer that scorer_type names is built
    (the reference builds all three), so a model's state_dict holds no parameter its loss cannot reach except ScorerMLP's.
    ScorerHead takes the scorer's output_nc.  cluster_voxel_size: the voxel edge of the clusters' tensor (0.05; None or 0:
    the data's `coords` unchanged).

    The sparse scorers score every cluster as one cloud of ONE sparse tensor with clouds = the number of clusters: no
    per-cluster loop, no trip through the host (the reference moves the batch to the CPU and back), the score loss
    reaches the backbone through the voxel mean's gradient.  Device-to-host reads of one scoring: two in cluster_voxelize
    and one per coordinate set the scorer visits (three for the YAML's two strided stages)."""

    loss_names = ["loss", "offset_norm_loss", "offset_dir_loss", "semantic_loss", "score_loss"]

    def __init__(self, input_nc, num_classes, stuff_classes=(), backbone=None, scorer_type="MLP", scorer_nc=None,
                 cluster_radius_search=0.03, prepare_epoch=120, loss_weights=None, min_iou_threshold=0.25,
                 max_iou_threshold=0.75, scorer_unet=None, scorer_encoder=None, cluster_voxel_size=0.05):
        super().__init__()
        if scorer_type not in ("unet", "encoder", "MLP", None):
            raise ValueError("unknown scorer_type %r" % (scorer_type,))
        if scorer_type in ("unet", "encoder") and (scorer_unet if scorer_type == "unet" else scorer_encoder) is None:
            raise NotImplementedError(
                "PointGroup scorer_type %r is not served without its network: it scores every cluster as one cloud of a "
                "sparse network, and by default the sparse coordinate keys hold 2^9 clouds while a scene has more clusters "
                "than that.  Pass scorer_%s=<config> (pointgroup_config(name, feat)[\"scorer_%s\"], or any dict "
                "SparseConv3d%s takes) to score on a tensor built with clouds = the number of clusters, or use \"MLP\" or "
                "None.  The MinkowskiEngine backends are out of scope."
                % (scorer_type, scorer_type, scorer_type, "Unet" if scorer_type == "unet" else "Encoder"))
        self.Backbone = backbone if backbone is not None else SparseConv3dUnet("unet_4", input_nc)
        nc = self.Backbone.output_nc
        self._scorer_type = scorer_type
        self.cluster_voxel_size = cluster_voxel_size
        self._scorer_cfg = None
        if scorer_type in ("unet", "encoder"):
            cfg = scorer_unet if scorer_type == "unet" else scorer_encoder
            if cfg["down_conv"]["down_conv_nn"][0][0] != nc:
                raise ValueError("the %s scorer takes %d channels, the backbone gives %d"
                                 % (scorer_type, cfg["down_conv"]["down_conv_nn"][0][0], nc))
            self._scorer_cfg = cfg
            if scorer_type == "unet":
                self.ScorerUnet = SparseConv3dUnet(cfg, nc)
            else:
                self.ScorerEncoder = SparseConv3dEncoder(cfg, nc)
            sparse_nc = (self.ScorerUnet if scorer_type == "unet" else self.ScorerEncoder).output_nc
            if scorer_nc is not None and scorer_nc != sparse_nc:
                raise ValueError("scorer_nc %d is not the %s scorer's output width %d" % (scorer_nc, scorer_type, sparse_nc))
            scorer_nc = sparse_nc
        scorer_nc = nc if scorer_nc is None else scorer_nc
        self.ScorerMLP = MLP([nc, nc, scorer_nc])
        self.ScorerHead = Seq().append(nn.Linear(scorer_nc, 1)).append(nn.Sigmoid())
        self.Offset = Seq().append(MLP([nc, nc], bias=False))
        self.Offset.append(nn.Linear(nc, 3))
        self.Semantic = (Seq().append(MLP([nc, nc], bias=False)).append(nn.Linear(nc, num_classes))
                         .append(nn.LogSoftmax(dim=-1)))
        stuff = torch.as_tensor(list(stuff_classes), dtype=torch.long).reshape(-1)
        self.register_buffer("_stuff_classes", torch.cat([torch.tensor([IGNORE_LABEL]), stuff]), persistent=False)
        self.cluster_radius_search = cluster_radius_search
        self.prepare_epoch = prepare_epoch
        self.loss_weights = dict(semantic=1, offset_norm_loss=1, offset_dir_loss=1, score_loss=1)
        self.loss_weights.update(loss_weights or {})
        self.min_iou_threshold, self.max_iou_threshold = min_iou_threshold, max_iou_threshold

    def forward(self, data, epoch=-1):
        self.input = data
        backbone_features = self.Backbone(data)
        semantic_logits = self.Semantic(backbone_features)
        offset_logits = self.Offset(backbone_features)
        cluster_scores = all_clusters = cluster_type = None
        if epoch == -1 or epoch > self.prepare_epoch:  # active by default
            predicted_labels = torch.max(semantic_logits, 1)[1]
            all_clusters, cluster_type = cluster(data.pos, data.pos + offset_logits.detach(), predicted_labels, data.batch,
                                                 self._stuff_classes, self.cluster_radius_search)
            if len(all_clusters):
                cluster_scores = self._compute_score(all_clusters, backbone_features, semantic_logits)
        self.output = PanopticResults(semantic_logits=semantic_logits, offset_logits=offset_logits, clusters=all_clusters,
                                      cluster_scores=cluster_scores, cluster_type=cluster_type)
        return self.output

    def _compute_score(self, clusters, backbone_features, semantic_logits):
        if self._scorer_type in ("unet", "encoder"):
            data = self.input
            voxels, voxel_starts = tp.cluster_voxelize(clusters, backbone_features, data.pos, self.cluster_voxel_size,
                                                       getattr(data, "coords", None))
            if self._scorer_type == "unet":
                cluster_feats = tp.segment_max(self.ScorerUnet(voxels), voxel_starts)
            else:
                cluster_feats = self.ScorerEncoder(voxels, clouds=len(clusters))
            return self.ScorerHead(cluster_feats).squeeze(-1)
        if self._scorer_type:
            rows = self.ScorerMLP(backbone_features[clusters.members])
            cluster_feats = tp.segment_max(rows, clusters.starts)
            return self.ScorerHead(cluster_feats).squeeze(-1)
        with torch.no_grad():  # the semantic certainty as the cluster's confidence
            mean = tp.segment_mean(semantic_logits, clusters.starts, clusters.members)
            return torch.max(mean, 1)[0]

    def compute_loss(self, labels):
        """labels: PanopticLabels (y, instance_labels, instance_mask, vote_label are read).  Sets and returns the
        reference's losses (pointgroup.py:174-203): a dict over `loss_names`."""
        out = self.output
        self.semantic_loss = torch.nn.functional.nll_loss(out.semantic_logits, labels.y, ignore_index=IGNORE_LABEL)
        self.loss = self.loss_weights["semantic"] * self.semantic_loss
        mask = labels.instance_mask
        offset_losses = offset_loss(out.offset_logits[mask], labels.vote_label[mask], torch.sum(mask))
        for name, value in offset_losses.items():
            setattr(self, name, value)
            self.loss = self.loss + self.loss_weights[name] * value
        self.score_loss = None
        if out.cluster_scores is not None and self._scorer_type:
            self.score_loss = instance_iou_loss(out.clusters, out.cluster_scores, labels.instance_labels, self.input.batch,
                                                min_iou_threshold=self.min_iou_threshold,
                                                max_iou_threshold=self.max_iou_threshold)
            self.loss = self.loss + self.score_loss * self.loss_weights["score_loss"]
        return {name: getattr(self, name) for name in self.loss_names}
