"""VoteNet object detection on the dense PointNet++ modules, with the box post-processing on the device.

Mirrors, with the reference's class names, attribute names and state_dict keys,
  modules/VoteNet/voting_module.py:13-82        VotingModule
  modules/VoteNet/proposal_module.py:14-77      ProposalModule
  modules/VoteNet/votenet_results.py:11-255     VoteNetResults (from_logits, assign_objects, get_boxes)
  modules/VoteNet/loss_helper.py                compute_*_loss, to_dense_labels, get_loss
  models/object_detection/votenet2.py:15-194    VoteNet2 -> VoteNet (no BaseModel; the `VoteNetPaper` layout of
                                                conf/models/object_detection/votenet2.yaml:2-89)
  metrics/box_detection/ap.py                   eval_detection -> DetectionEvaluator
The three steps the reference walks box by box on the host -- the NMS sweep, the rotated IoU and the greedy AP
matching -- are HIP kernels (csrc/detection.hip, torchpoints.box_nms / box3d_iou / ap_match).  CPU tensors take the numpy
form of the same definitions (detection_cpu.py); device tensors never do.

Three things the reference's code does and its paper does not say; they are kept:
 1. ProposalModule computes furthest_point_sample(seed_pos, num_proposal) and hands it to the aggregation as
    `sampled_idx=`, which BaseDenseConvolutionDown.forward (core/base_conv/dense.py:60, argument `sample_idx`) swallows in
    **kwargs: the aggregation samples the VOTE positions itself.  Here that unused sampling is not computed at all.
 2. VoteNet2._select_seeds returns seed_inds = sampling_id_0[:, :num_seeds]: indices of the FIRST level's samples, not the
    composed indices of the level the seed features live on.  compute_vote_loss gathers the vote labels through them.
    (With furthest point sampling at every level both name the same points: sampling an FPS-ordered set again returns
    its prefix.  A backbone that samples otherwise gets the reference's behaviour, not a correction of it.)
 3. Order of equal scores, which neither np.argsort call of the reference defines: the NMS visits boxes by descending
    score and among equal scores the higher index first; AP matching visits detections by descending score and equal
    scores keep their input order.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import detection_cpu as _cpu
from . import fused as _fused
from . import torchpoints as _tp
from .dense import Data, DenseFPModule, PointNetMSGDown, Seq
from .losses import huber_loss, nn_distance

FAR_THRESHOLD = 0.6
NEAR_THRESHOLD = 0.3
GT_VOTE_FACTOR = 3
OBJECTNESS_CLS_WEIGHTS = [0.2, 0.8]


# ===================================================================================================== boxes
class BoxData(object):
    """One box (datasets/object_detection/box_data.py): a prediction when it has a score, a ground-truth box otherwise."""

    def __init__(self, classname, corners3d, score=None):
        assert tuple(corners3d.shape) == (8, 3)
        self.classname = classname.item() if torch.is_tensor(classname) else classname
        self.corners3d = corners3d.cpu().numpy() if torch.is_tensor(corners3d) else np.asarray(corners3d)
        self.score = score.item() if torch.is_tensor(score) else score

    @property
    def is_gt(self):
        return self.score is None

    def __repr__(self):
        return "{}: (score={})".format(self.__class__.__name__, self.score)


def box_corners_from_param(box_size, heading_angle, center):
    """utils/box_utils.py:8-25 for any number of boxes: box_size (..., 3), heading_angle (...), center (..., 3) ->
    (..., 8, 3) fp32.  Rows 0-3 are the bottom face counter-clockwise seen from +z, rows 4-7 the top face; the rotation
    is euler_angles_to_rotation_matrix([0, 0, heading]): x' = cos x - sin y, y' = sin x + cos y."""
    box_size = torch.as_tensor(box_size).float()
    dev = box_size.device
    center = torch.as_tensor(center, device=dev).float()
    if torch.is_tensor(heading_angle):
        heading = heading_angle.to(device=dev, dtype=torch.float32).expand(box_size.shape[:-1])
    else:
        heading = torch.full(box_size.shape[:-1], float(heading_angle), dtype=torch.float32, device=dev)
    k = torch.arange(8, device=dev)  # corner k: x sign from bit 0 xor bit 1, y sign bit 1, z sign bit 2 (made on the device)
    half = lambda bit: (bit.float() - 0.5)  # noqa: E731
    x = box_size[..., 0:1] * half((k ^ (k >> 1)) & 1)
    y = box_size[..., 1:2] * half((k >> 1) & 1)
    z = box_size[..., 2:3] * half((k >> 2) & 1)
    c, s = torch.cos(heading).unsqueeze(-1), torch.sin(heading).unsqueeze(-1)
    out = torch.stack([c * x - s * y, s * x + c * y, z], -1)
    return out + center.unsqueeze(-2)


class BoxSet(object):
    """The boxes of a batch of scenes as tensors on one device.

    Public fields, all over the n boxes that exist, ordered by scene: `corners` (n, 8, 3) fp32, `score` (n,) fp32 (None
    for ground truth), `classname` (n,) int64, `scene` (n,) int64 and `scene_start` (B + 1,) int64, the offsets of the
    scenes.  Internally the set is kept at its padded size with a `valid` mask, as get_boxes produces it: nothing is
    read back to the host until one of corners / score / classname / scene or to_list() is asked for (the boxes are
    compacted then, once).  `scene_start` and `num_scenes` never need the host."""

    def __init__(self, corners, classname, scene, valid, num_scenes, score=None, class_names=None):
        self._corners, self._classname, self._scene, self._score = corners, classname, scene, score
        self.valid = valid
        self.num_scenes = int(num_scenes)
        self.class_names = class_names  # optional: names for to_list() / the dict adaptor
        self._index = None

    # ---- construction
    @classmethod
    def from_padded(cls, corners, classname, mask, score=None, class_names=None):
        """corners (B, K, 8, 3), classname (B, K), mask (B, K) bool (, score (B, K)): e.g. the padded ground-truth labels
        `instance_box_corners`, `sem_cls_label`, `box_label_mask` of a batch"""
        B, K = mask.shape
        scene = torch.arange(B, device=corners.device).repeat_interleave(K)
        return cls(corners.reshape(B * K, 8, 3).float(), classname.reshape(-1).long(), scene, mask.reshape(-1).bool(), B,
                   None if score is None else score.reshape(-1).float(), class_names)

    @classmethod
    def from_list(cls, scenes, device=None, class_names=None):
        """the reference's List[List[BoxData]] (one list per scene).  Class names that are not integers are numbered by
        `class_names` (grown as needed)."""
        names = class_names
        flat, scene, cls_id, score = [], [], [], []
        for s, boxes in enumerate(scenes):
            for b in boxes:
                c = b.classname
                if not isinstance(c, (int, np.integer)):
                    names = [] if names is None else names
                    if c not in names:
                        names.append(c)
                    c = names.index(c)
                flat.append(np.asarray(b.corners3d, dtype=np.float32))
                scene.append(s)
                cls_id.append(int(c))
                score.append(b.score)
        n = len(flat)
        corners = torch.from_numpy(np.stack(flat)) if n else torch.zeros((0, 8, 3))
        has_score = n > 0 and score[0] is not None
        out = cls(corners.to(device), torch.tensor(cls_id, dtype=torch.int64, device=device),
                  torch.tensor(scene, dtype=torch.int64, device=device), torch.ones(n, dtype=torch.bool, device=device),
                  len(scenes), torch.tensor(score, dtype=torch.float32, device=device) if has_score else None, names)
        return out

    # ---- fields
    def _idx(self):
        if self._index is None:
            self._index = torch.nonzero(self.valid, as_tuple=False).squeeze(1)  # the one host read
        return self._index

    @property
    def corners(self):
        return self._corners[self._idx()]

    @property
    def classname(self):
        return self._classname[self._idx()]

    @property
    def scene(self):
        return self._scene[self._idx()]

    @property
    def score(self):
        return None if self._score is None else self._score[self._idx()]

    @property
    def scene_start(self):
        counts = torch.zeros(self.num_scenes + 1, dtype=torch.int64, device=self.valid.device)
        counts.index_add_(0, self._scene + 1, self.valid.long())
        return counts.cumsum(0)

    def __len__(self):
        return int(self._idx().shape[0])

    def to_list(self):
        """List[List[BoxData]], one list per scene, in the reference's order"""
        corners = self.corners.cpu().numpy()
        cls = self.classname.cpu().tolist()
        scene = self.scene.cpu().tolist()
        score = None if self._score is None else self.score.cpu().tolist()
        out = [[] for _ in range(self.num_scenes)]
        for k in range(len(cls)):
            name = cls[k] if self.class_names is None else self.class_names[cls[k]]
            out[scene[k]].append(BoxData(name, corners[k], None if score is None else score[k]))
        return out


def box_nms(boxes, scores, classes, overlap_threshold=0.25):
    """nms_samecls per scene: (B, P, 6), (B, P), (B, P) -> keep (B, P) bool; HIP on a device, numpy otherwise"""
    if boxes.is_cuda:
        return _tp.box_nms(boxes, scores, classes, overlap_threshold)
    if boxes.shape[1] > _tp.BOX_NMS_MAX_BOXES:
        raise ValueError("box_nms serves at most %d boxes per scene" % _tp.BOX_NMS_MAX_BOXES)
    return torch.from_numpy(_cpu.box_nms(boxes.detach().numpy(), scores.detach().numpy(), classes.numpy(), overlap_threshold))


def box3d_iou(corners1, corners2):
    """box3d_iou of every pair: (n, 8, 3), (m, 8, 3) -> (n, m) float64; HIP on a device, numpy otherwise"""
    if corners1.is_cuda:
        return _tp.box3d_iou(corners1, corners2)
    return torch.from_numpy(_cpu.box3d_iou(corners1.detach().numpy(), corners2.detach().numpy()))


def box3d_vol(corners):
    """utils/box_utils.py:112-118: the product of three edge lengths, (..., 8, 3) -> (...) float64"""
    c = torch.as_tensor(corners).double()
    edge = lambda i, j: (c[..., i, :] - c[..., j, :]).pow(2).sum(-1).sqrt()  # noqa: E731
    return edge(0, 1) * edge(1, 2) * edge(0, 4)


def ap_match(det, gt, thresholds=(0.25, 0.5)):
    """(tp (D, T) bool, ovmax (D,) float64, jmax (D,) int64) of the detections `det` against the ground truth `gt` (two
    BoxSets over the same scenes); see torchpoints.ap_match"""
    args = (det.corners, det.score, det.classname, det.scene, gt.corners, gt.classname, gt.scene_start)
    if det.valid.is_cuda:
        return _tp.ap_match(*args, thresholds=thresholds)
    tp, ov, j = _cpu.ap_match(*[a.detach().numpy() for a in args], thresholds=list(thresholds))
    return torch.from_numpy(tp), torch.from_numpy(ov), torch.from_numpy(j)


# ===================================================================================================== results
class VoteNetResults(Data):
    """The structured output of the proposal network (modules/VoteNet/votenet_results.py); fields as documented there."""

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, value):
        setattr(self, key, value)

    @classmethod
    def from_logits(cls, seed_inds, seed_votes, seed_pos, sampled_votes, features, num_classes, num_heading_bin,
                    mean_size_arr):
        """features (B, 2 + 3 + 2 * num_heading_bin + 4 * num_size_cluster + num_classes, num_proposal), split in that
        order into objectness, centre offset, heading scores and residuals, size scores and residuals, class scores."""
        nsc = len(mean_size_arr)
        nhb = num_heading_bin
        assert features.dim() == 3
        assert features.shape[1] == 2 + 3 + nhb * 2 + nsc * 4 + num_classes
        data = cls(sampled_votes=sampled_votes, seed_inds=seed_inds, seed_votes=seed_votes, seed_pos=seed_pos)
        data.has_class = num_classes != 0
        xt = features.transpose(2, 1)  # (B, num_proposal, features)
        B, P = xt.shape[0], xt.shape[1]
        data.objectness_scores = xt[:, :, 0:2]
        data.center = sampled_votes + xt[:, :, 2:5]
        data.heading_scores = xt[:, :, 5:5 + nhb]
        data.heading_residuals_normalized = xt[:, :, 5 + nhb:5 + 2 * nhb]
        data.heading_residuals = data.heading_residuals_normalized * (np.pi / nhb)
        o = 5 + 2 * nhb
        data.size_scores = xt[:, :, o:o + nsc]
        data.size_residuals_normalized = xt[:, :, o + nsc:o + 4 * nsc].reshape(B, P, nsc, 3)
        if nsc > 0:
            data.size_residuals = data.size_residuals_normalized * mean_size_arr.unsqueeze(0).unsqueeze(0)
        data.sem_cls_scores = xt[:, :, o + 4 * nsc:] if num_classes else None
        return data

    def assign_objects(self, gt_center, gt_object_mask, near_threshold, far_threshold):
        """objectness_label (B, K) int64: 1 when the vote lies within near_threshold of a ground-truth centre;
        objectness_mask (B, K) fp32: 0 in the grey zone between the thresholds; object_assignment (B, K): the nearest
        ground-truth slot.  All three are 0 where that slot is masked out."""
        dist1, ind1, _, _ = nn_distance(self.sampled_votes, gt_center)
        dist = torch.sqrt(dist1 + 1e-6)
        gt_mask = torch.gather(gt_object_mask, 1, ind1)
        near, far = dist < near_threshold, dist > far_threshold
        self.objectness_label = near.long() * gt_mask.long()
        self.objectness_mask = (near | far).float() * gt_mask.float()
        self.object_assignment = ind1

    @property
    def batch_size(self):
        return self.center.shape[0]

    @property
    def num_proposal(self):
        return self.center.shape[1]

    def decode_corners(self, dataset):
        """(B, P, 8, 3) corners of every proposal: arg-max heading and size class, their residuals, the rotation"""
        hc = torch.argmax(self.heading_scores, -1)
        hr = torch.gather(self.heading_residuals, 2, hc.unsqueeze(-1)).squeeze(-1)
        sc = torch.argmax(self.size_scores, -1)
        sr = torch.gather(self.size_residuals, 2, sc.unsqueeze(-1).unsqueeze(-1).expand(-1, -1, 1, 3)).squeeze(2)
        if hasattr(dataset, "class2angle"):
            angle = dataset.class2angle(hc, hr)  # vectorised, or a scalar (ScanNet: 0) that is broadcast
        else:
            angle = hc.to(hr.dtype) * (2 * np.pi / float(self.heading_scores.shape[-1])) + hr
        mean_size = dataset.mean_size_arr
        if torch.is_tensor(mean_size):  # a tensor already on the device is used as is: no copy, nothing to wait for
            mean_size = mean_size.to(device=sr.device, dtype=torch.float32)
        else:
            mean_size = torch.as_tensor(np.asarray(mean_size), dtype=torch.float32).to(sr.device)
        return box_corners_from_param(mean_size[sc] + sr, angle, self.center)

    def get_boxes(self, dataset, apply_nms=False, objectness_threshold=0.05, duplicate_boxes=False):
        """The predicted boxes of the batch as a BoxSet (to_list() gives the reference's List[List[BoxData]] in its order:
        per scene the proposals ascending, and with duplicate_boxes every kept proposal once per class, classes ascending,
        scored objectness * class probability).  `dataset` supplies `mean_size_arr` and optionally a vectorised
        `class2angle(heading_class (B, P), residual (B, P))`; without it the angle is
        class * 2 pi / num_heading_bin + residual.  NMS (threshold 0.25, per class of the arg-max) runs on the axis-aligned
        hulls of the corners.  No loop over boxes and no host read: the set stays padded with a validity mask."""
        corners = self.decode_corners(dataset)  # (B, P, 8, 3)
        B, P = corners.shape[:2]
        dev = corners.device
        pred_obj = torch.softmax(self.objectness_scores, -1)[:, :, 1]
        pred_cls = torch.argmax(self.sem_cls_scores, -1)
        keep = pred_obj > objectness_threshold
        if apply_nms:
            hull = torch.cat([corners.min(2)[0], corners.max(2)[0]], -1)
            keep = keep & box_nms(hull, pred_obj, pred_cls, 0.25)
        has_class = getattr(self, "has_class", self.sem_cls_scores is not None)
        if duplicate_boxes and has_class:
            proba = torch.softmax(self.sem_cls_scores, -1)
            C = proba.shape[-1]
            score = (pred_obj.unsqueeze(-1) * proba).reshape(-1)
            cls = torch.arange(C, device=dev).expand(B, P, C).reshape(-1)
            corners = corners.unsqueeze(2).expand(B, P, C, 8, 3).reshape(-1, 8, 3)
            valid = keep.unsqueeze(-1).expand(B, P, C).reshape(-1)
            per_scene = P * C
        else:
            score, cls, corners, valid, per_scene = pred_obj.reshape(-1), pred_cls.reshape(-1), corners.reshape(-1, 8, 3), \
                keep.reshape(-1), P
        scene = torch.arange(B, device=dev).repeat_interleave(per_scene)
        return BoxSet(corners, cls, scene, valid, B, score)


# ===================================================================================================== modules
def _pointwise(layer, x):
    """a kernel-size-1 Conv1d on (B, C, N) as one batched GEMM with the layer's own weight and bias"""
    return torch.baddbmm(layer.bias.view(1, -1, 1), layer.weight.squeeze(-1).unsqueeze(0).expand(x.shape[0], -1, -1), x)


class VotingModule(nn.Module):
    """Each seed votes `vote_factor` times: an offset to its position and a residual to its features."""

    def __init__(self, vote_factor, seed_feature_dim, conv_type="DENSE"):
        super().__init__()
        self.vote_factor = vote_factor
        self.in_dim = seed_feature_dim
        self.out_dim = self.in_dim  # the features are residual
        self._conv_type = conv_type
        make = (lambda i, o: nn.Conv1d(i, o, 1)) if conv_type == "DENSE" else nn.Linear
        self.conv1 = make(self.in_dim, self.in_dim)
        self.conv2 = make(self.in_dim, self.in_dim)
        self.conv3 = make(self.in_dim, (3 + self.out_dim) * self.vote_factor)
        self.bn1 = nn.BatchNorm1d(self.in_dim)
        self.bn2 = nn.BatchNorm1d(self.in_dim)

    def forward(self, data):
        """DENSE: data.pos (B, N, 3), data.x (B, C, N) -> Data(pos (B, N * vote_factor, 3), x (B, C, N * vote_factor),
        seed_pos).  Otherwise rows: pos (N, 3), x (N, C), batch."""
        if self._conv_type == "DENSE":
            B, N = data.pos.shape[0], data.pos.shape[1]
            x = F.relu(self.bn1(_pointwise(self.conv1, data.x)))
            x = F.relu(self.bn2(_pointwise(self.conv2, x)))
            x = _pointwise(self.conv3, x)
            x = x.transpose(2, 1).reshape(B, N, self.vote_factor, 3 + self.out_dim)
            vote_pos = (data.pos.unsqueeze(2) + x[..., 0:3]).reshape(B, N * self.vote_factor, 3)
            vote_x = (data.x.transpose(2, 1).unsqueeze(2) + x[..., 3:]).reshape(B, N * self.vote_factor, self.out_dim)
            return Data(pos=vote_pos, x=vote_x.transpose(2, 1).contiguous(), seed_pos=data.pos)
        x = F.relu(self.bn1(self.conv1(data.x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = self.conv3(x)
        return Data(pos=data.pos + x[:, 0:3], x=data.x + x[:, 3:], seed_pos=data.pos, batch=getattr(data, "batch", None))


class VoteAggregation(PointNetMSGDown):
    """PointNetMSGDown over the votes.  The set abstraction's fused path treats positions as data (in a backbone they
    are), but vote positions are outputs of the voting module: the grouped, centred coordinates carry a gradient back
    to it.  When the positions require a gradient, the rows get the same coordinates once more through differentiable
    torch gathers as `rel - rel.detach()` -- exactly zero in value, so the forward pass is unchanged bit for bit -- and
    the MLP chain is asked for the gradient of every input column instead of the feature columns only."""

    def _conv_fused(self, parts, x, pos, new_pos, radius_idx, scale_idx, table=None):
        if not (torch.is_grad_enabled() and pos.requires_grad):
            return super()._conv_fused(parts, x, pos, new_pos, radius_idx, scale_idx, table)
        if x is None or not self.use_xyz:
            return None
        B, npnt, ns = radius_idx.shape
        rows = _fused.group_concat(pos, new_pos, _fused._cl(x), radius_idx, self.radii[scale_idx], self.normalize_xyz, table)
        idx = radius_idx.long().reshape(B, npnt * ns, 1).expand(-1, -1, 3)
        rel = pos.gather(1, idx).view(B, npnt, ns, 3) - new_pos.unsqueeze(2)
        if self.normalize_xyz:
            rel = rel / self.radii[scale_idx]
        rel = rel.reshape(B * npnt * ns, 3)
        rows = rows + F.pad(rel - rel.detach(), (0, rows.shape[1] - 3))
        pooled = _fused.run_mlp(rows, parts, pool_ns=ns)
        return pooled.view(B, npnt, -1).transpose(1, 2)


class ProposalModule(nn.Module):
    """Vote aggregation (one PointNet++ set abstraction over the votes) and the three-layer proposal head.

    The aggregation samples the vote positions with its own furthest point sampling: the reference computes a sampling
    of the SEED positions first and passes it under a keyword the aggregation does not read (see the module docstring,
    point 1), so that sampling has no effect and is not computed here.  The head's layers carry a bias, which the fused
    row kernels (fused.mlp_parts) do not take, so they run as plain GEMMs."""

    def __init__(self, num_class, vote_aggregation_config, num_heading_bin, mean_size_arr, num_proposal, sampling,
                 kernels=None, fused=True):
        super().__init__()
        self.num_class = num_class
        self.num_heading_bin = num_heading_bin
        self.num_size_cluster = len(mean_size_arr)
        self.mean_size_arr = nn.Parameter(torch.as_tensor(np.asarray(mean_size_arr), dtype=torch.float32), requires_grad=False)
        self.num_proposal = num_proposal
        self.sampling = sampling
        params = dict(vote_aggregation_config)
        assert params.get("module_name", "PointNetMSGDown") == "PointNetMSGDown", "Proposal Module support only PointNet2 for now"
        self.vote_aggregation = VoteAggregation(kernels=kernels, fused=fused, **params)
        nc = params["down_conv_nn"][-1][-1]
        output_feat = 2 + 3 + num_heading_bin * 2 + self.num_size_cluster * 4 + self.num_class
        mid_feat = (nc + output_feat) // 2
        self.conv1 = nn.Conv1d(nc, nc, 1)
        self.conv2 = nn.Conv1d(nc, mid_feat, 1)
        self.conv3 = nn.Conv1d(mid_feat, output_feat, 1)
        self.bn1 = nn.BatchNorm1d(nc)
        self.bn2 = nn.BatchNorm1d(mid_feat)

    def head(self, x):
        x = F.relu(self.bn1(_pointwise(self.conv1, x)))
        x = F.relu(self.bn2(_pointwise(self.conv2, x)))
        return _pointwise(self.conv3, x)

    def forward(self, data):
        """data.pos (B, N, 3) votes, data.x (B, C, N), data.seed_pos, data.seed_inds -> VoteNetResults"""
        if data.pos.dim() != 3:
            raise ValueError("This method only supports dense convolutions for now")
        if self.sampling != "seed_fps":
            raise ValueError("Unknown sampling strategy: %s. Exiting!" % (self.sampling))
        feats = self.vote_aggregation(Data(pos=data.pos, x=data.x))
        x = self.head(feats.x)
        return VoteNetResults.from_logits(data.seed_inds, data.pos, data.seed_pos, feats.pos, x, self.num_class,
                                          self.num_heading_bin, self.mean_size_arr)


# ===================================================================================================== losses
def _field(obj, key):
    return obj[key] if isinstance(obj, dict) else getattr(obj, key)


def _set_field(obj, key, value):
    if isinstance(obj, dict):
        obj[key] = value
    else:
        setattr(obj, key, value)


def _masked_mean(values, mask):
    return torch.sum(values * mask) / (torch.sum(mask) + 1e-6)


def compute_vote_loss(input, output):
    """For every seed inside an object (vote_label_mask), the smallest l1 distance between one of its votes and one of
    its GT_VOTE_FACTOR ground-truth votes, averaged over those seeds.  The labels are gathered through output.seed_inds
    (see the module docstring, point 2)."""
    seed_pos = output["seed_pos"]
    B, num_seed = seed_pos.shape[0], seed_pos.shape[1]
    seed_inds = output["seed_inds"].long()
    mask = torch.gather(_field(input, "vote_label_mask"), 1, seed_inds).float()
    gt_votes = torch.gather(_field(input, "vote_label"), 1, seed_inds.unsqueeze(-1).expand(-1, -1, 3 * GT_VOTE_FACTOR))
    gt_votes = gt_votes + seed_pos.repeat(1, 1, GT_VOTE_FACTOR)
    votes = output["seed_votes"].reshape(B * num_seed, -1, 3)
    _, _, dist2, _ = nn_distance(votes, gt_votes.reshape(B * num_seed, GT_VOTE_FACTOR, 3), l1=True)
    votes_dist = torch.min(dist2, dim=1)[0].view(B, num_seed)
    return _masked_mean(votes_dist, mask)


def compute_objectness_loss(inputs, outputs, loss_params):
    scores = outputs["objectness_scores"]
    weights = torch.tensor(_field(loss_params, "objectness_cls_weights"), dtype=scores.dtype, device=scores.device)
    loss = F.cross_entropy(scores.transpose(2, 1), outputs.objectness_label, weight=weights, reduction="none")
    return _masked_mean(loss, outputs.objectness_mask)


def compute_box_and_sem_cls_loss(inputs, outputs, loss_params, weight_classes=None):
    """(center, heading class, heading residual, size class, size residual, semantic class) losses over the proposals
    labelled as objects, each against the ground-truth slot of its object_assignment"""
    num_heading_bin = _field(loss_params, "num_heading_bin")
    dev = outputs["center"].device
    mean_size_arr = torch.as_tensor(np.asarray(_field(loss_params, "mean_size_arr"), dtype=np.float32)).to(dev)
    num_size_cluster = mean_size_arr.shape[0]
    assignment = outputs.object_assignment
    obj = outputs["objectness_label"].float()

    dist1, _, dist2, _ = nn_distance(outputs["center"], _field(inputs, "gt_center"))
    box_label_mask = _field(inputs, "box_label_mask")
    center_loss = _masked_mean(dist1, obj) + _masked_mean(dist2, box_label_mask)

    heading_class_label = torch.gather(_field(inputs, "heading_class_label"), 1, assignment).long()
    heading_class_loss = F.cross_entropy(outputs["heading_scores"].transpose(2, 1), heading_class_label, reduction="none")
    heading_class_loss = _masked_mean(heading_class_loss, obj)
    heading_residual_label = torch.gather(_field(inputs, "heading_residual_label"), 1, assignment)
    heading_residual_normalized_label = heading_residual_label / (np.pi / num_heading_bin)
    one_hot = F.one_hot(heading_class_label, num_heading_bin).to(obj.dtype)
    heading_reg_loss = huber_loss(
        torch.sum(outputs["heading_residuals_normalized"] * one_hot, -1) - heading_residual_normalized_label, delta=1.0)
    heading_reg_loss = _masked_mean(heading_reg_loss, obj)

    if num_size_cluster != 0:
        size_class_label = torch.gather(_field(inputs, "size_class_label"), 1, assignment).long()
        size_class_loss = F.cross_entropy(outputs["size_scores"].transpose(2, 1), size_class_label, reduction="none")
        size_class_loss = _masked_mean(size_class_loss, obj)
        size_residual_label = torch.gather(_field(inputs, "size_residual_label"), 1, assignment.unsqueeze(-1).expand(-1, -1, 3))
        tiled = F.one_hot(size_class_label, num_size_cluster).to(obj.dtype).unsqueeze(-1).expand(-1, -1, -1, 3)
        predicted = torch.sum(outputs["size_residuals_normalized"] * tiled, 2)
        mean_size_label = torch.sum(tiled * mean_size_arr.unsqueeze(0).unsqueeze(0), 2)
        size_reg_loss = torch.mean(huber_loss(predicted - size_residual_label / mean_size_label, delta=1.0), -1)
        size_reg_loss = _masked_mean(size_reg_loss, obj)
    else:
        size_class_loss = 0
        size_reg_loss = 0

    sem_cls_label = torch.gather(_field(inputs, "sem_cls_label"), 1, assignment).long()
    sem_cls_loss = F.cross_entropy(outputs["sem_cls_scores"].transpose(2, 1), sem_cls_label, weight=weight_classes,
                                   reduction="none")
    sem_cls_loss = _masked_mean(sem_cls_loss, obj)
    return center_loss, heading_class_loss, heading_reg_loss, size_class_loss, size_reg_loss, sem_cls_loss


def to_dense_labels(data):
    """the label fields reshaped to (B, K, ...), and gt_center = center_label[..., 0:3]"""
    get = data.get if isinstance(data, dict) else (lambda k: getattr(data, k, None))
    if get("batch") is not None:
        B = len(torch.unique(get("batch")))
    elif get("pos") is not None:
        B = get("pos").shape[0]
    else:
        B = _field(data, "center_label").shape[0]  # dense labels (B, K, 3)
    for key in ("heading_class_label", "heading_residual_label", "size_class_label", "sem_cls_label", "box_label_mask"):
        _set_field(data, key, _field(data, key).view((B, -1)))
    _set_field(data, "size_residual_label", _field(data, "size_residual_label").view((B, -1, 3)))
    _set_field(data, "instance_box_corners", _field(data, "instance_box_corners").view((B, -1, 8, 3)))
    center = _field(data, "center_label")
    _set_field(data, "gt_center", center[:, :, 0:3] if center.dim() == 3 else center[:, 0:3].view((B, -1, 3)))
    return data


def get_loss(inputs, outputs, loss_params, weight_classes=None):
    """{name: loss}: the reference's weights -- box = center + 0.1 heading_cls + heading_reg + 0.1 size_cls + size_reg,
    loss = 10 * (vote + 0.5 objectness + box + 0.1 sem_cls)"""
    losses = {}
    inputs = to_dense_labels(inputs)
    losses["vote_loss"] = vote_loss = compute_vote_loss(inputs, outputs)
    losses["objectness_loss"] = objectness_loss = compute_objectness_loss(inputs, outputs, loss_params)
    center, heading_cls, heading_reg, size_cls, size_reg, sem_cls = compute_box_and_sem_cls_loss(
        inputs, outputs, loss_params, weight_classes=weight_classes)
    losses["center_loss"] = center
    losses["heading_cls_loss"] = heading_cls
    losses["heading_reg_loss"] = heading_reg
    losses["size_cls_loss"] = size_cls
    losses["size_reg_loss"] = size_reg
    losses["sem_cls_loss"] = sem_cls
    losses["box_loss"] = box_loss = center + 0.1 * heading_cls + heading_reg + 0.1 * size_cls + size_reg
    losses["loss"] = (vote_loss + 0.5 * objectness_loss + box_loss + 0.1 * sem_cls) * 10
    return losses


# ===================================================================================================== network
def votenet_config(name, feat, num_classes, mean_size_arr, in_feat=64, num_features=256, num_proposal=256, num_seeds=1024,
                   npoint=(2048, 1024, 512, 256), nsamples=((64,), (32,), (16,), (16,)), agg_nsample=16):
    """conf/models/object_detection/votenet2.yaml resolved for FEAT = feat.  The keyword arguments are the file's
    constants (and its point counts), for reduced networks; the defaults are the file's.  The aggregation's widths are
    the ones VoteNet2.__init__ (votenet2.py:75-77) puts in place of the file's:
    [num_features + 3, num_features, num_features]."""
    if name != "VoteNetPaper":
        raise ValueError("unknown VoteNet config %r (only the dense PointNet++ layout VoteNetPaper is built)" % name)
    f = in_feat
    backbone = dict(
        npoint=list(npoint), radii=[[0.2], [0.4], [0.8], [1.2]], nsample=[list(n) for n in nsamples],
        down_conv_nn=[[[feat + 3, f, f, f * 2]], [[f * 2 + 3, f * 2, f * 2, f * 4]], [[f * 4 + 3, f * 2, f * 2, f * 4]],
                      [[f * 4 + 3, f * 2, f * 2, f * 4]]],
        save_sampling_id=[True, False, False, False], normalize_xyz=[True, True, True, True],
        up_conv_nn=[[f * 4 + f * 4, f * 4, f * 4], [f * 4 + f * 4, f * 4, num_features]], skip=True)
    return dict(
        conv_type="DENSE", backbone=backbone,
        voting=dict(module_name="VotingModule", vote_factor=1, feat_dim=num_features, num_points_to_sample=num_seeds),
        proposal=dict(module_name="ProposalModule",
                      vote_aggregation=dict(module_name="PointNetMSGDown", npoint=num_proposal, radii=[0.3],
                                            nsample=[agg_nsample],
                                            down_conv_nn=[[num_features + 3, num_features, num_features]],
                                            normalize_xyz=True),
                      num_class=num_classes, num_heading_bin=1, num_proposal=num_proposal, sampling="seed_fps"),
        loss_params=dict(far_threshold=FAR_THRESHOLD, near_threshold=NEAR_THRESHOLD, gt_vote_factor=GT_VOTE_FACTOR,
                         objectness_cls_weights=list(OBJECTNESS_CLS_WEIGHTS), num_heading_bin=1,
                         mean_size_arr=np.asarray(mean_size_arr, dtype=np.float32).tolist()))


class VoteNetBackbone(nn.Module):
    """The truncated dense PointNet++ U-Net of VoteNetPaper: four set abstractions, no innermost module, two feature
    propagations, so the features come out on the SECOND level's points.  Module names as the reference's
    UnwrappedUnetBasedModel (`down_modules`, `inner_modules` = [Identity], `up_modules`); the first level's
    `sampling_id_0` is handed through to the output (unet.py:501-530, applications/pointnet2.py:153-191)."""

    def __init__(self, input_nc, config, kernels=None, fused=True):
        super().__init__()
        cfg = config
        self.config = cfg
        self.fused = fused
        self._kernels_are_hip = kernels is None
        self.down_modules = nn.ModuleList(
            PointNetMSGDown(npoint=cfg["npoint"][i], radii=cfg["radii"][i], nsample=cfg["nsample"][i],
                            down_conv_nn=cfg["down_conv_nn"][i], normalize_xyz=cfg["normalize_xyz"][i],
                            save_sampling_id=cfg["save_sampling_id"][i], index=i, kernels=kernels, fused=fused)
            for i in range(len(cfg["down_conv_nn"])))
        self.inner_modules = nn.ModuleList([nn.Identity()])
        self.up_modules = nn.ModuleList(DenseFPModule(up_conv_nn=c, index=i, kernels=kernels, fused=fused)
                                        for i, c in enumerate(cfg["up_conv_nn"]))
        self._output_nc = cfg["up_conv_nn"][-1][-1]

    @property
    def output_nc(self):
        return self._output_nc

    def forward(self, data):
        """data.pos (B, N, 3), data.x (B, N, C) or None -> Data(pos (B, n, 3), x (B, output_nc, n), sampling_id_0)"""
        x = None
        if data.x is not None:
            x = data.x.transpose(1, 2)
            if not (self.fused and self._kernels_are_hip and x.is_cuda):
                x = x.contiguous()
        cur = Data(pos=data.pos, x=x)
        stack_down = [cur]
        for i in range(len(self.down_modules) - 1):
            cur = self.down_modules[i](cur)
            stack_down.append(cur)
        cur = self.down_modules[-1](cur)
        sampling_ids = {}
        for d in stack_down:
            for k, v in d.__dict__.items():
                if k.startswith("sampling_id"):
                    sampling_ids[k] = v
        for up in self.up_modules:
            cur = up((cur, stack_down.pop()))
        for k, v in sampling_ids.items():
            setattr(cur, k, v)
        return cur


class VoteNet(nn.Module):
    """VoteNet2 (models/object_detection/votenet2.py) without the BaseModel plumbing: backbone -> optional dropout ->
    seed selection -> voting -> proposal -> VoteNetResults; with labels, the object assignment and the losses.

    Sub-module names are the reference's (`backbone_model`, `voting_module`, `proposal_cls_module`, `Semantic`,
    `dropout`), so its state_dict loads with strict=True.  `backbone` may be any module with `output_nc` and a dense
    forward(Data(pos (B, N, 3), x (B, N, C))) -> Data(pos (B, n, 3), x (B, output_nc, n)[, sampling_id_0])."""

    def __init__(self, config="VoteNetPaper", feat=0, num_classes=18, mean_size_arr=None, backbone=None, dropout=None,
                 semantic_supervision=False, weight_classes=None, kernels=None, fused=True):
        super().__init__()
        cfg = votenet_config(config, feat, num_classes, mean_size_arr) if isinstance(config, str) else config
        self.config = cfg
        self._kernels = kernels or _tp
        self._weight_classes = weight_classes
        self.backbone_model = backbone if backbone is not None else VoteNetBackbone(feat, cfg["backbone"], kernels=kernels,
                                                                                    fused=fused)
        nc = self.backbone_model.output_nc
        self.dropout = nn.Dropout(dropout) if dropout is not None else None
        if semantic_supervision:
            from .partial_dense import MLP
            self.Semantic = Seq().append(MLP([nc, nc], bias=False)).append(nn.Linear(nc, num_classes)).append(nn.LogSoftmax(-1))
        else:
            self.Semantic = None
        voting = cfg["voting"]
        self._num_seeds = voting["num_points_to_sample"]
        self.voting_module = VotingModule(vote_factor=voting["vote_factor"], seed_feature_dim=nc)
        prop = cfg["proposal"]
        agg = dict(prop["vote_aggregation"], down_conv_nn=[[nc + 3, nc, nc]])  # votenet2.py:75-77
        self.proposal_cls_module = ProposalModule(
            num_class=prop["num_class"], vote_aggregation_config=agg, num_heading_bin=prop["num_heading_bin"],
            mean_size_arr=cfg["loss_params"]["mean_size_arr"], num_proposal=prop["num_proposal"], sampling=prop["sampling"],
            kernels=kernels, fused=fused)
        self.loss_params = dict(cfg["loss_params"], num_heading_bin=prop["num_heading_bin"])
        self.semantic_logits = None
        self.losses = None

    def _select_seeds(self, data_features):
        """(Data(pos, x) of num_seeds seeds, seed_inds).  With `sampling_id_0` from the backbone, seed_inds are its first
        num_seeds columns -- indices of the FIRST level's samples in the input cloud, also when the features live on a
        deeper level (module docstring, point 2) -- and when the feature level has another size than num_seeds they also
        gather pos and x.  Without it: furthest point sampling of the feature positions."""
        ids = getattr(data_features, "sampling_id_0", None)
        pos, x = data_features.pos, data_features.x
        if ids is not None:
            seed_inds = ids[:, :self._num_seeds]
            if pos.shape[1] == self._num_seeds:
                return Data(pos=pos, x=x), seed_inds
        else:
            if self._num_seeds > pos.shape[1]:
                raise ValueError("num_to_sample %d should be smaller than num_pos %d" % (self._num_seeds, pos.shape[1]))
            seed_inds = self._kernels.furthest_point_sample(pos, self._num_seeds).long()
        pos = torch.gather(pos, 1, seed_inds.unsqueeze(-1).expand(-1, -1, pos.shape[-1]))
        x = torch.gather(x, 2, seed_inds.unsqueeze(1).expand(-1, x.shape[1], -1))
        return Data(pos=pos, x=x), seed_inds

    def forward(self, data, labels=None, semantic_labels=None):
        """data.pos (B, N, 3), data.x (B, N, C) or None -> VoteNetResults.  `labels` (an object or dict with the label
        fields of the reference's __REQUIRED_LABELS__, and `pos`): the objects are assigned and self.losses is filled
        (self.losses["loss"] is the total, the semantic head's 10 * nll_loss included when it ran)."""
        feats = self.backbone_model(data)
        if self.dropout is not None:
            feats.x = self.dropout(feats.x)
        seeds, seed_inds = self._select_seeds(feats)
        self.semantic_logits = None
        if self.Semantic is not None and semantic_labels is not None:
            rows = feats.x.transpose(2, 1).reshape(-1, feats.x.shape[1])
            if rows.shape[0] == semantic_labels.shape[0]:
                self.semantic_logits = self.Semantic(rows)
        votes = self.voting_module(seeds)
        votes.seed_inds = seed_inds
        outputs = self.proposal_cls_module(votes)
        self.losses = None
        if labels is not None:
            center = _field(labels, "center_label")
            mask = _field(labels, "box_label_mask")
            B = outputs.batch_size
            gt_center = center[:, :, 0:3] if center.dim() == 3 else center[:, 0:3].view((B, -1, 3))
            outputs.assign_objects(gt_center, mask.view((B, -1)), self.loss_params["near_threshold"],
                                   self.loss_params["far_threshold"])
            self.losses = get_loss(labels, outputs, self.loss_params, weight_classes=self._weight_classes)
            if self.semantic_logits is not None:
                self.losses["semantic_loss"] = F.nll_loss(self.semantic_logits, semantic_labels, ignore_index=-1)
                self.losses["loss"] = self.losses["loss"] + 10 * self.losses["semantic_loss"]
        return outputs


# ===================================================================================================== evaluation
def voc_ap(rec, prec):
    """PASCAL VOC average precision (metrics/box_detection/ap.py:10-32), float64"""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


class DetectionEvaluator(object):
    """Average precision of 3-D detections over a whole validation pass.  add() keeps the BoxSets of a batch (nothing
    is computed and nothing read back); finalise() matches every detection of every scene in one pass of the HIP
    kernels (numpy for CPU BoxSets) and forms the per-class precision / recall curves in float64 on the host."""

    def __init__(self):
        self._pred, self._gt = [], []

    def add(self, boxes, gt):
        if boxes.num_scenes != gt.num_scenes:
            raise ValueError("predictions cover %d scenes, ground truth %d" % (boxes.num_scenes, gt.num_scenes))
        self._pred.append(boxes)
        self._gt.append(gt)

    @staticmethod
    def _merge(sets):
        off, parts = 0, []
        for s in sets:
            parts.append((s.corners, s.classname, s.scene + off, s.score))
            off += s.num_scenes
        cat = lambda k: torch.cat([p[k] for p in parts])  # noqa: E731
        score = None if parts[0][3] is None else cat(3)
        n = sum(p[0].shape[0] for p in parts)
        dev = parts[0][0].device
        return BoxSet(cat(0), cat(1), cat(2), torch.ones(n, dtype=torch.bool, device=dev), off, score, sets[0].class_names)

    def match(self, overlap_thresholds=(0.25, 0.5)):
        """(det, gt, tp (D, T) bool, ovmax (D,), jmax (D,)) over everything added so far"""
        det, gt = self._merge(self._pred), self._merge(self._gt)
        tp, ovmax, jmax = ap_match(det, gt, overlap_thresholds)
        return det, gt, tp, ovmax, jmax

    def finalise(self, overlap_thresholds=(0.25, 0.5)):
        """(rec, prec, ap): each {threshold: {classname: value}} as eval_detection returns them per threshold -- rec and
        prec arrays over the class's detections by descending score, ap a float; 0 for a ground-truth class without a
        detection."""
        overlap_thresholds = list(overlap_thresholds)
        det, gt, tp, _, _ = self.match(overlap_thresholds)
        tp = tp.cpu().numpy()
        score = det.score.double().cpu().numpy()
        dcls, gcls = det.classname.cpu().numpy(), gt.classname.cpu().numpy()
        names = det.class_names or gt.class_names
        name = (lambda c: c) if names is None else (lambda c: names[c])
        rec, prec, ap = {}, {}, {}
        for t, thr in enumerate(overlap_thresholds):
            rec[thr], prec[thr], ap[thr] = {}, {}, {}
            for c in sorted(set(gcls.tolist()) | set(dcls.tolist())):
                sel = np.where(dcls == c)[0]
                if len(sel) == 0:
                    rec[thr][name(c)], prec[thr][name(c)], ap[thr][name(c)] = 0, 0, 0
                    continue
                sel = sel[np.argsort(-score[sel], kind="stable")]
                hits = np.cumsum(tp[sel, t].astype(np.float64))
                misses = np.cumsum((~tp[sel, t]).astype(np.float64))
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = hits / float((gcls == c).sum())
                p = hits / np.maximum(hits + misses, np.finfo(np.float64).eps)
                rec[thr][name(c)], prec[thr][name(c)], ap[thr][name(c)] = r, p, voc_ap(r, p)
        return rec, prec, ap


def eval_detection(pred_all, gt_all, ovthresh=0.25, processes=4, device=None):
    """The reference's signature (metrics/box_detection/ap.py:127-178): pred_all, gt_all {img_id: [BoxData]} ->
    (rec, prec, ap), each {classname: value}.  `processes` is accepted and unused; `device` moves the boxes there."""
    ids = list(dict.fromkeys(list(pred_all.keys()) + list(gt_all.keys())))
    names = []
    pred = BoxSet.from_list([pred_all.get(i, []) for i in ids], device=device, class_names=names)
    gt = BoxSet.from_list([gt_all.get(i, []) for i in ids], device=device, class_names=names)
    pred.class_names = gt.class_names = names if names else None
    ev = DetectionEvaluator()
    ev.add(pred, gt)
    rec, prec, ap = ev.finalise([ovthresh])
    return rec[ovthresh], prec[ovthresh], ap[ovthresh]
