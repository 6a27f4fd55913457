"""Panoptic evaluation: cluster suppression, instance matching and instance AP.

Mirrors (metric keys, thresholds, host arithmetic):
  * `instances_device`    PanopticResults.get_instances, models/panoptic/structures.py:6-49
  * `PanopticEvaluator`   PanopticTracker and InstanceAPMeter, metrics/panoptic_tracker.py:16-294

The reference builds a (K, N) mask and a (K, K) matrix for the suppression, copies every cluster to numpy, walks every
ground-truth instance with torch.where and intersects every (prediction, instance) pair with np.intersect1d.  Here GPU
tensors go through the kernels of csrc/panoptic_metrics.hip (`torchpoints.cluster_best_instance`, `cluster_overlaps`,
`cluster_nms`, `instance_ap_match`): `track` only enqueues work and reads nothing back, the sums and the per-prediction
records stay on the device, `finalise` / `get_metrics` read them once.  CPU tensors take the numpy restatements of the
same rules kept in this file (`*_numpy`), so the host arithmetic can be pinned without a GPU.

The evaluator takes tensors, not the reference's model / data objects: `track(model.get_output(), model.get_labels(),
data.batch)` is the substitution.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import torchpoints as _tp
from .pointgroup import _as_set
from .seg_metrics import SegmentationEvaluator, _is_gpu, _np
from .votenet import voc_ap

__all__ = ["instances_device", "PanopticEvaluator", "cluster_best_instance_numpy", "cluster_overlaps_numpy",
           "cluster_nms_numpy", "instance_ap_match_numpy"]

CLUSTER_BEST_WINDOW = _tp.CLUSTER_BEST_WINDOW


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of the rules of include/tp3d_hip.h ("Panoptic metrics"); they return CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def cluster_best_instance_numpy(clusters, column, gt_size, gt_class, cluster_class, col_lo, col_hi):
    """`torchpoints.cluster_best_instance` on the host: (inter_all, col_all, inter_cls, col_cls), (K,) int64 each"""
    members, starts = _np(clusters.members, np.int64), _np(clusters.starts, np.int64)
    column, gt_size, gt_class = _np(column, np.int64), _np(gt_size, np.int64), _np(gt_class, np.int64)
    cluster_class, col_lo, col_hi = _np(cluster_class, np.int64), _np(col_lo, np.int64), _np(col_hi, np.int64)
    K = starts.shape[0] - 1
    out = np.zeros((4, K), dtype=np.int64)
    out[1], out[3] = -1, -1
    for k in range(K):
        n = int(starts[k + 1] - starts[k])
        cols = column[members[starts[k]:starts[k + 1]]]
        cols = cols[(cols >= max(int(col_lo[k]), 0)) & (cols < min(int(col_hi[k]), gt_size.shape[0]))]
        if cols.shape[0] == 0:
            continue
        u, inter = np.unique(cols, return_counts=True)  # ascending columns: argmax names the first maximum
        fi = inter.astype(np.float32)
        iou32 = fi / np.maximum((np.float32(n) + gt_size[u].astype(np.float32)) - fi, np.float32(1.0))
        j = int(np.argmax(iou32))
        out[0, k], out[1, k] = inter[j], u[j]
        same = gt_class[u] == cluster_class[k]
        if same.any():
            iou64 = inter[same].astype(np.float64) / (n + gt_size[u[same]] - inter[same]).astype(np.float64)
            j = int(np.argmax(iou64))
            out[2, k], out[3, k] = inter[same][j], u[same][j]
    return tuple(torch.from_numpy(o.copy()) for o in out)


def cluster_overlaps_numpy(clusters):
    """`torchpoints.cluster_overlaps` on the host: (ov_start (K + 1,), ov_other (P,), ov_inter (P,)); a point that one
    cluster lists twice is counted once"""
    members, owner = _np(clusters.members, np.int64), _np(clusters.member_cluster, np.int64)
    K = len(clusters)
    if members.shape[0] > _tp.CLUSTER_MAX_PAIRS or K > _tp.CLUSTER_MAX_PAIRS:
        raise ValueError("cluster_overlaps indexes at most 2^31 - 1 slots, clusters and pairs")
    slots = np.unique(members * max(K, 1) + owner) if members.shape[0] else np.zeros(0, dtype=np.int64)
    point, cl = slots // max(K, 1), slots % max(K, 1)
    cut = np.flatnonzero(np.concatenate([[True], point[1:] != point[:-1], [True]])) if slots.shape[0] else np.zeros(1, int)
    keys = []
    for a, b in zip(cut[:-1], cut[1:]):
        if b - a > 1:
            c = cl[a:b]
            pair = c[:, None] * K + c[None, :]
            keys.append(pair[c[:, None] != c[None, :]])
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    if keys.shape[0] > _tp.CLUSTER_MAX_PAIRS:
        raise ValueError("cluster_overlaps: %d overlapping pairs are more than 2^31 - 1" % keys.shape[0])
    u, inter = np.unique(keys, return_counts=True)
    ov_start = np.searchsorted(u // max(K, 1), np.arange(K + 1)).astype(np.int64)
    return torch.from_numpy(ov_start), torch.from_numpy((u % max(K, 1)).astype(np.int64)), torch.from_numpy(inter.astype(np.int64))


def cluster_nms_numpy(clusters, scores, threshold, overlaps=None):
    """`torchpoints.cluster_nms` on the host: (keep (K,) bool, order (K,) int64); equal scores are visited higher index
    first (a stable ascending sort read from the back)"""
    K = len(clusters)
    scores = _np(scores).reshape(-1)
    if scores.shape[0] != K:
        raise ValueError("one score per cluster is needed")
    if overlaps is None:
        overlaps = cluster_overlaps_numpy(clusters)
    ov_start, ov_other, ov_inter = (_np(t, np.int64) for t in overlaps[:3])
    size = _np(clusters.sizes(), np.int64).astype(np.float32)
    thr = np.float32(threshold)
    order = np.argsort(scores, kind="stable")[::-1].astype(np.int64)
    alive = np.ones(K, dtype=bool)
    keep = np.zeros(K, dtype=bool)
    for i in order:
        if not alive[i]:
            continue
        keep[i] = True
        other = ov_other[ov_start[i]:ov_start[i + 1]]
        fi = ov_inter[ov_start[i]:ov_start[i + 1]].astype(np.float32)
        alive[other[fi / ((size[i] + size[other]) - fi) > thr]] = False
    return torch.from_numpy(keep), torch.from_numpy(order.copy())


def instance_ap_match_numpy(order, cls, cloud, valid, size, inter_cls, col_cls, gt_size, threshold):
    """`torchpoints.instance_ap_match` on the host: tp (K,) bool"""
    order, cls, cloud, size = (_np(t, np.int64) for t in (order, cls, cloud, size))
    inter_cls, col_cls, gt_size, valid = _np(inter_cls, np.int64), _np(col_cls, np.int64), _np(gt_size, np.int64), _np(valid)
    tp = np.zeros(order.shape[0], dtype=bool)
    taken = set()  # an instance belongs to one (cloud, class) group: its column alone names it
    for d in order:
        j = int(col_cls[d])
        if not valid[d] or j < 0:
            continue
        iou = float(inter_cls[d]) / float(size[d] + gt_size[j] - inter_cls[d])
        if iou >= threshold and j not in taken:
            taken.add(j)
            tp[d] = True
    return torch.from_numpy(tp)


# ---------------------------------------------------------------------------------------------------------------------
def instances_device(results, nms_threshold=0.3, min_cluster_points=100, min_score=0.2, pair_capacity=None, stats=None):
    """PanopticResults.get_instances on the device of the results: (valid (K,) bool, order (K,) int64).  `order` is the
    visiting order of the suppression (`torchpoints.cluster_nms`: descending score, equal scores higher index first);
    the valid clusters taken in that order -- order[valid[order]] -- are get_instances' list.  The reference's quirk is
    kept as get_instances documents it: the size test compares the NUMBER of clusters with min_cluster_points.

    pair_capacity (GPU only): room for the overlapping cluster pairs; None asks `cluster_overlaps` for the exact size,
    which reads two integers back, a number reads nothing; `stats` (a list) then receives the overlap statistics."""
    clusters = results.clusters
    if clusters is None or len(clusters) == 0:
        dev = results.semantic_logits.device
        return torch.zeros(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    clusters = _as_set(clusters, results.semantic_logits.device)
    scores = results.cluster_scores.detach()
    if _is_gpu(scores.device):
        ov = _tp.cluster_overlaps(clusters, capacity=pair_capacity, return_stats=True)
        if stats is not None:
            stats.append(ov[3])
        keep, order = _tp.cluster_nms(clusters, scores, nms_threshold, overlaps=ov)
    else:
        keep, order = cluster_nms_numpy(clusters, scores, nms_threshold)
    enough = len(clusters) > min_cluster_points
    valid = keep & (scores > min_score) if enough else torch.zeros_like(keep)
    return valid, order


class PanopticEvaluator(SegmentationEvaluator):
    """PanopticTracker on tensors: `track(outputs, labels, batch)` per batch, `finalise()` and `get_metrics()` at the
    end of the epoch.  Keys: the semantic ones of SegmentationEvaluator, `{stage}_pos`, `_neg`, `_Iacc`, `_map`, and
    under `verbose` `_iou_per_class`, `_class_rec`, `_class_ap`.

    What `track` computes per batch (metrics/panoptic_tracker.py, line for line):
      _compute_acc (191-221)  every valid cluster (instances_device) takes its best instance over all columns; fp32
          IoU < iou_threshold is a false positive; otherwise a true positive when the majority label of the instance's
          points (first maximum of the label histogram, lowest label on ties) is the cluster's predicted label.
          acc = tp / clusters, pos = tp / num_instances.sum(), neg = fp / num_instances.sum(), each averaged over the
          track calls that had at least one valid cluster.
      AP (49-104, 230-269)    a prediction is a true positive when its best instance AMONG THOSE OF ITS CLASS has float64
          IoU >= iou_threshold (not strict) and has not been taken by an earlier prediction of its cloud and class;
          earlier = higher score, equal scores in visiting order.  An instance belongs to one (cloud, class) group and
          every prediction of a cloud arrives in the same `track` call, so the flags are final at `track` time: only
          (class, score, flag) per prediction and the instance count per class survive the batch.  `finalise` reads
          them back once and forms recall, precision and votenet.voc_ap per class in float64; a class with ground truth
          and no prediction scores 0; mAP is the mean over the classes with ground truth; `_class_rec` the last recall.
          The class of an instance is the label of its lowest-index point.  One quirk of the reference is kept, as
          get_instances' size test is: _pred_instances_per_scan pairs the i-th VALID cluster (in visiting order) with
          cluster_scores[i], the score of the i-th cluster of the batch, and that is the score the AP sorts by.

    Differences from the reference, all on inputs it does not serve:
      * an instance id without points is skipped (the reference raises IndexError);
      * iou_threshold must be > 0 (ValueError): at 0 the reference's result depends on columns of other clouds;
      * a batch with valid clusters and num_instances.sum() == 0 is skipped (the reference raises ZeroDivisionError);
      * the flags are formed with the threshold of their own `track` call (the reference evaluates every record with
        the threshold of the last call);
      * cloud s owns labels.num_instances[s] columns, as the reference's own offsets assume (instance_iou derives the
        count from the largest id instead); an instance id above it is reported as ValueError at the end.
    On a GPU `track` reads nothing back.  Two sizes are therefore bounds, checked on the device and reported by
    `finalise` / `get_metrics` as ValueError: the instance columns of a batch must not outnumber its points, and the
    overlapping cluster pairs must fit `pair_capacity` (default: the member slots of the batch, which holds any set of
    clusters in which a point belongs to at most two -- PointGroup's two partitions)."""

    def __init__(self, num_classes, stage="train", ignore_label=-1, pair_capacity=None):
        self._pair_capacity = pair_capacity
        super().__init__(num_classes, stage=stage, ignore_label=ignore_label)

    def reset(self, stage="train"):
        super().reset(stage)
        self._sums = None       # (4,) float64 on the device: pos, neg, acc, calls
        self._ngt = None        # (C + 1,) int64: instances per class, index label + 1 (label -1: the ignored label)
        self._errors = None     # (3,) int64 batches with: pairs beyond capacity, columns > points, ids > num_instances
        self._records = []      # per batch (class or -9, score, flag) in visiting order, on the device
        self._scan_id_offset = 0
        self._iou_threshold = None
        self._rec, self._ap = {}, {}
        self._iou_per_class = {}

    # -- one batch ----------------------------------------------------------------------------------------------------
    def track(self, outputs, labels, batch=None, iou_threshold=0.25, track_instances=True, min_cluster_points=10):
        if not iou_threshold > 0:
            raise ValueError("iou_threshold must be > 0, got %r" % (iou_threshold,))
        self._iou_threshold = iou_threshold
        logits = outputs.semantic_logits.detach()
        super().track(logits, labels.y)
        if batch is None or outputs.clusters is None or len(outputs.clusters) == 0:
            return
        dev = logits.device
        gpu = _is_gpu(dev)
        clusters = _as_set(outputs.clusters, dev)
        if clusters.members.numel() == 0:
            return
        K, M, N, C = len(clusters), clusters.members.numel(), logits.shape[0], self._num_classes
        if self._sums is None:
            self._sums = torch.zeros(4, dtype=torch.float64, device=dev)
            self._ngt = torch.zeros(C + 1, dtype=torch.int64, device=dev)
            self._errors = torch.zeros(3, dtype=torch.int64, device=dev)
        stats = []
        capacity = (self._pair_capacity if self._pair_capacity is not None else M) if gpu else None
        valid, order = instances_device(outputs, min_cluster_points=min_cluster_points, pair_capacity=capacity, stats=stats)

        # ground-truth columns, in the layout of torch_points_kernels.instance_iou (cloud s owns num_instances[s] columns).
        # The tables come from sorts and binary searches, not from scatters: thousands of points of one instance (or of
        # none) would queue on one atomic.
        gt = labels.instance_labels.long()
        b = batch.long()
        y = labels.y.long()
        nb = labels.num_instances.shape[0]
        per_cloud = labels.num_instances.long()
        offsets = torch.cumsum(per_cloud, 0) - per_cloud
        beyond = gt > per_cloud[b]
        column = torch.where((gt > 0) & ~beyond, offsets[b] + gt - 1, torch.full_like(gt, -1))
        self._errors[2] += beyond.any().long()
        if gpu:
            G = N  # a bound instead of a read; more columns than points is reported at the end
            self._errors[1] += (per_cloud.sum() > G).long()
            column = torch.where(column < G, column, torch.full_like(column, -1))
        else:
            G = int(per_cloud.sum())
            if G == 0:
                return  # no instance at all: num_instances.sum() == 0, the skipped batch
        width = C + 1  # label bins: -1 (the ignored label) .. C - 1
        bins = torch.arange(width, dtype=torch.long, device=dev)
        by_column, point = torch.sort(torch.where(column >= 0, column, torch.full_like(column, G)), stable=True)
        edge = torch.searchsorted(by_column, torch.arange(G + 1, dtype=torch.long, device=dev))
        gt_size = edge[1:] - edge[:-1]
        present = gt_size > 0
        first = point[edge[:-1].clamp(max=N - 1)]  # stable sort: the lowest point of the column
        gt_class = torch.where(present, y[first], torch.full_like(first, -2))
        label_key = torch.sort(torch.where(column >= 0, column * width + y.clamp(min=-1, max=C - 1) + 1,
                                           torch.full_like(column, G * width))).values

        # per cluster
        head = clusters.members[clusters.starts[:-1].clamp(max=M - 1)]
        predicted = logits.argmax(1)
        cluster_class, cloud = predicted[head], b[head]
        col_lo = offsets[cloud]
        col_hi = col_lo + per_cloud[cloud]
        size = clusters.sizes().long()
        best = (_tp.cluster_best_instance if gpu else cluster_best_instance_numpy)(
            clusters, column, gt_size, gt_class, cluster_class, col_lo, col_hi)
        inter_all, col_all, inter_cls, col_cls = best

        # _compute_acc
        at = col_all.clamp(min=0)
        fi = inter_all.float()
        iou = torch.where(col_all >= 0, fi / ((size.float() + gt_size[at].float()) - fi).clamp(min=1.0), torch.zeros_like(fi))
        matched = valid & ~(iou < float(np.float32(iou_threshold))) & (col_all >= 0)
        # the majority label of the matched instance: first maximum of its label histogram, lowest label on ties
        probe = (at * width).unsqueeze(1) + bins
        votes = torch.searchsorted(label_key, probe + 1) - torch.searchsorted(label_key, probe)
        majority = torch.where(votes == votes.max(1, keepdim=True).values, bins, torch.full_like(bins, width)).min(1).values - 1
        tp = (matched & (majority == cluster_class)).sum().double()
        n_valid = valid.sum().double()
        n_inst = labels.num_instances.sum().double()
        counted = ((n_valid > 0) & (n_inst > 0)).double()
        denom = n_inst.clamp(min=1.0)
        self._sums += counted * torch.stack([tp / denom, (n_valid - tp) / denom, tp / n_valid.clamp(min=1.0),
                                             torch.ones_like(tp)])
        if stats:
            self._errors[0] += stats[0][2]

        if track_instances:
            # _pred_instances_per_scan (230-247) reads scores[i] with i the position in the list of VALID clusters: the
            # i-th valid cluster in visiting order carries the score of cluster i.  Kept as the reference behaves.
            taken_in_order = valid[order]
            rank = torch.cumsum(taken_in_order.long(), 0) - 1
            ap_score = outputs.cluster_scores.detach().double()[rank.clamp(min=0)]
            ap_score = torch.where(taken_in_order, ap_score, torch.full_like(ap_score, float("-inf")))
            walk = order[torch.sort(ap_score, descending=True, stable=True).indices]  # equal scores: insertion order
            match = _tp.instance_ap_match if gpu else instance_ap_match_numpy
            flag = match(walk, cluster_class, cloud, valid, size, inter_cls, col_cls, gt_size, float(iou_threshold))
            live = valid & (counted > 0)
            rec_class = torch.where(live, cluster_class, torch.full_like(cluster_class, -9))
            self._records.append((rec_class[order], ap_score, flag[order]))
            class_bin = torch.where(present, gt_class.clamp(min=-1, max=C - 1) + 1, torch.full_like(gt_class, -1))
            self._ngt += (class_bin.unsqueeze(1) == bins).sum(0) * (counted > 0).long()
            self._scan_id_offset += nb

    # -- the end of the epoch -------------------------------------------------------------------------------------------
    def _check(self):
        if self._errors is None:
            return
        pairs, columns, beyond = (int(v) for v in self._errors.cpu())
        if beyond:
            raise ValueError("%d batches held an instance id above num_instances of its cloud" % beyond)
        if pairs:
            raise ValueError("%d batches had more overlapping cluster pairs than pair_capacity holds: their suppression "
                             "was not computed; construct the evaluator with a larger pair_capacity" % pairs)
        if columns:
            raise ValueError("%d batches had more instance columns than points: number the instances of a cloud "
                             "consecutively from 1" % columns)

    def prediction_records(self):
        """(class (P,) int64, score (P,) float64, flag (P,) bool) of the predicted instances tracked so far, in
        insertion order (batch after batch, inside a batch in visiting order), on the host: the one read of the records"""
        if not self._records:
            return np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0, dtype=bool)
        cls = torch.cat([r[0] for r in self._records]).cpu().numpy()
        score = torch.cat([r[1] for r in self._records]).cpu().numpy()
        flag = torch.cat([r[2] for r in self._records]).cpu().numpy().astype(bool)
        live = cls != -9
        return cls[live], score[live], flag[live]

    def finalise(self, track_instances=True):
        per_class_iou = self._matrix(None).get_intersection_union_per_class()[0]
        self._iou_per_class = {k: v for k, v in enumerate(per_class_iou)}
        self._check()
        if not track_instances:
            return
        ngt = self._ngt.cpu().numpy() if self._ngt is not None else np.zeros(self._num_classes + 1, dtype=np.int64)
        cls, score, flag = self.prediction_records()
        rec, ap = {}, {}
        for c in range(-1, self._num_classes):
            if ngt[c + 1] == 0:
                continue
            mine = np.flatnonzero(cls == c)
            if mine.shape[0] == 0:
                rec[c], ap[c] = 0, 0
                continue
            mine = mine[np.argsort(-score[mine], kind="stable")]  # descending score, equal scores in insertion order
            tp = np.cumsum(flag[mine].astype(np.float64))
            fp = np.cumsum((~flag[mine]).astype(np.float64))
            recall = tp / float(ngt[c + 1])
            precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            rec[c], ap[c] = recall[-1], voc_ap(recall, precision)
        self._ap = OrderedDict(sorted(ap.items()))
        self._rec = OrderedDict(sorted(rec.items()))

    @property
    def _has_instance_data(self):
        return len(self._rec)

    @staticmethod
    def _dict_to_str(dictionnary):
        string = "{"
        for key, value in dictionnary.items():
            string += "%s: %.2f," % (str(key), value)
        string += "}"
        return string

    def get_metrics(self, verbose=False):
        metrics = super().get_metrics(verbose)
        self._check()
        sums = self._sums.cpu().numpy() if self._sums is not None else np.zeros(4)
        for key, total in zip(("pos", "neg", "Iacc"), sums[:3]):
            metrics["{}_{}".format(self._stage, key)] = float(total / sums[3]) if sums[3] > 0 else 0.0
        if self._has_instance_data:
            metrics["{}_map".format(self._stage)] = sum(self._ap.values()) / len(self._ap)
        if verbose:
            metrics["{}_iou_per_class".format(self._stage)] = self._iou_per_class
        if verbose and self._has_instance_data:
            metrics["{}_class_rec".format(self._stage)] = self._dict_to_str(self._rec)
            metrics["{}_class_ap".format(self._stage)] = self._dict_to_str(self._ap)
        return metrics
