"""Segmentation metrics: confusion matrix, ShapeNet part IoU, full-resolution votes.

Mirrors (method names, metric keys, scaling and host arithmetic):
  * `ConfusionMatrix`          torch_points3d/metrics/confusion_matrix.py:6-104
  * `SegmentationEvaluator`    torch_points3d/metrics/segmentation_tracker.py:13-102   (SegmentationTracker)
  * `ShapenetPartEvaluator`    torch_points3d/metrics/shapenet_part_tracker.py:11-156  (ShapenetPartTracker)
  * `SegmentationVoter`        torch_points3d/metrics/segmentation_helpers.py:7-87
  * `S3DISEvaluator`           torch_points3d/metrics/s3dis_tracker.py:17-122          (S3DISTracker)

The reference copies every (N, C) score matrix to the host and counts there.  Here GPU tensors are counted by the
kernels of csrc/seg_metrics.hip (`torchpoints.confusion_count`, `part_iou_counts`, `vote_add`): `track` only enqueues
work, the counters stay on the device, and a getter reads them back once.  CPU tensors go to the numpy restatement of
the same counting rules in this file (`*_numpy`), so the host arithmetic of the metrics can be pinned without a GPU.
The means and ratios are the reference's float64 numpy expressions, term for term.

The evaluators take tensors, not the reference's model / dataset objects: `track(model.get_output(),
model.get_labels())` is the substitution.  Not served: the ScanNet, classification and panoptic
trackers, `APMeter`, the loss meters, wandb and TensorBoard publishing.
"""
import numpy as np
import torch

from . import torchpoints as _tp

__all__ = ["ConfusionMatrix", "SegmentationEvaluator", "ShapenetPartEvaluator", "SegmentationVoter", "S3DISEvaluator"]

PART_IOU_MAX_PARTS = _tp.PART_IOU_MAX_PARTS


def _is_gpu(device):
    return device is not None and torch.device(device).type == "cuda"


def _np(t, dtype=None):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    return t if dtype is None else t.astype(dtype, copy=False)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of the counting rules of include/tp3d_hip.h ("Segmentation metrics")
# ---------------------------------------------------------------------------------------------------------------------
def confusion_count_numpy(cm, labels, scores=None, pred=None, ignore_label=None, row_index=None, columns=None):
    """`torchpoints.confusion_count` on the host: cm (C * C + 1) int64 numpy, accumulated in place."""
    C = int(round((cm.shape[0] - 1) ** 0.5))
    labels = _np(labels, np.int64).reshape(-1)
    N = labels.shape[0]
    keep = np.ones(N, dtype=bool) if ignore_label is None else labels != int(ignore_label)
    bad = (labels < 0) | (labels >= C)
    if pred is not None:
        p = _np(pred, np.int64).reshape(-1)
        bad |= (p < 0) | (p >= C)
        valid = keep & ~bad
        p = p[valid]
    else:
        scores = _np(scores, np.float32)
        lo, hi = (0, C) if columns is None else (int(columns[0]), int(columns[1]))
        rows = np.arange(N, dtype=np.int64)
        if row_index is not None:
            rows = _np(row_index, np.int64).reshape(-1)
            keep &= rows != -1
        bad |= (rows < 0) | (rows >= scores.shape[0])
        valid = keep & ~bad
        p = lo + np.argmax(scores[rows[valid], lo:hi], axis=1) if valid.any() else np.zeros(0, dtype=np.int64)
    cm[:C * C] += np.bincount(C * labels[valid] + p, minlength=C * C)
    cm[C * C] += int((keep & bad).sum())
    return cm


def part_iou_counts_numpy(scores, labels, seg, part_lo, part_hi):
    """`torchpoints.part_iou_counts` on the host: (counts (B, PART_IOU_MAX_PARTS, 2) int32, cat_lo (B) int32)."""
    scores, labels, seg = _np(scores, np.float32), _np(labels, np.int64), _np(seg, np.int64)
    B, C = seg.shape[0] - 1, scores.shape[1]
    counts = np.zeros((B, PART_IOU_MAX_PARTS, 2), dtype=np.int32)
    cat_lo = np.full(B, -1, dtype=np.int32)
    for b in range(B):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        if s1 == s0:
            continue
        first = int(labels[s0])
        lo, hi = (int(part_lo[first]), int(part_hi[first])) if 0 <= first < C else (-2, -2)
        if lo < 0 or hi <= lo or hi > C or hi - lo > PART_IOU_MAX_PARTS:
            cat_lo[b] = -2
            continue
        cat_lo[b] = lo
        segl = labels[s0:s1]
        segp = np.argmax(scores[s0:s1, lo:hi], axis=1) + lo
        for part in range(lo, hi):
            counts[b, part - lo, 0] = np.sum((segl == part) & (segp == part))
            counts[b, part - lo, 1] = np.sum((segl == part) | (segp == part))
    return counts, cat_lo


def vote_add_numpy(votes, counts, ids, out):
    """`torchpoints.vote_add` on the host (votes (T, C) fp32 and counts (T) int32 torch tensors, changed in place);
    returns the number of ids outside [0, T).  Of equal ids the highest row wins."""
    ids = _np(ids, np.int64).reshape(-1)
    n, T = ids.shape[0], votes.shape[0]
    ok = (ids >= 0) & (ids < T)
    rows = np.nonzero(ok)[0]
    # last occurrence of every id: first occurrence in the reversed list
    _, first_rev = np.unique(ids[rows][::-1], return_index=True)
    win = torch.from_numpy(np.sort(rows[::-1][first_rev]))
    target = torch.from_numpy(ids)[win]
    votes[target] += out.detach().float()[win]
    counts[target] += 1
    return int(n - rows.shape[0])


def knn_host(k, support, query):
    """(idx (Nq, k) int64, d2 (Nq, k) fp32 squared distances) of the k nearest support rows, closest first: the host
    search of `torch_points_kernels.points_cpu` (libtp3d_cpu.so)"""
    from torch_points_kernels import points_cpu
    idx, d2 = points_cpu.dense_knn(support.detach().cpu().unsqueeze(0), query.detach().cpu().unsqueeze(0), k)
    return idx[0], d2[0]


def knn_interpolate_numpy(x, pos_x, pos_y, k):
    """torch_geometric's knn_interpolate on the host: weights 1 / max(d2, 1e-16), sums in neighbour order."""
    idx, d2 = knn_host(k, pos_x, pos_y)
    x = x.detach().float()
    w = 1.0 / torch.clamp(d2, min=1e-16)
    num = torch.zeros((idx.shape[0], x.shape[1]), dtype=torch.float32)
    den = torch.zeros((idx.shape[0], 1), dtype=torch.float32)
    for j in range(k):
        num += x[idx[:, j]] * w[:, j:j + 1]
        den += w[:, j:j + 1]
    return num / den


# ---------------------------------------------------------------------------------------------------------------------
class ConfusionMatrix(object):
    """The reference's streaming confusion matrix with the counters kept where the predictions are.

    `device=None` (or a CPU device) counts with numpy; a ROCm device counts with `torchpoints.confusion_count`, and the
    matrix is read back once by the first getter after a count and cached until the next count.  A label outside
    [0, number_of_labels) that is not the ignore label raises ValueError at that read (the reference's bincount would
    raise, or silently grow the matrix, at count time)."""

    def __init__(self, number_of_labels=2, device=None):
        self.number_of_labels = int(number_of_labels)
        self.device = torch.device("cpu" if device is None else device)
        C = self.number_of_labels
        if _is_gpu(self.device):
            self._cm = torch.zeros(C * C + 1, dtype=torch.int64, device=self.device)
        else:
            self._cm = np.zeros(C * C + 1, dtype=np.int64)
        self._host = None

    @staticmethod
    def create_from_matrix(confusion_matrix, device=None):
        m = _np(confusion_matrix, np.int64)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        out = ConfusionMatrix(m.shape[0], device)
        flat = np.concatenate([m.reshape(-1), np.zeros(1, dtype=np.int64)])
        out._cm = torch.from_numpy(flat).to(out.device) if _is_gpu(out.device) else flat
        return out

    # -- counting -----------------------------------------------------------------------------------------------------
    def _count(self, labels, **kw):
        self._host = None
        if _is_gpu(self.device):
            _tp.confusion_count(self._cm, labels, **kw)
        else:
            confusion_count_numpy(self._cm, labels, **kw)

    def count_predicted_batch(self, ground_truth_vec, predicted):
        """ground truth and predicted labels of one batch (the reference's entry point)"""
        if _is_gpu(self.device):
            ground_truth_vec, predicted = (torch.as_tensor(v).to(self.device) for v in (ground_truth_vec, predicted))
        self._count(ground_truth_vec, pred=predicted)

    def count_scores(self, ground_truth_vec, scores, ignore_label=None, row_index=None, columns=None):
        """ground truth and the (n, C) score matrix of one batch: the prediction of a row is the first maximum over
        `columns` = (lo, hi), default every class; row i reads scores[row_index[i]] (-1 skips it) when given; rows whose
        label is `ignore_label` are skipped.  On a device nothing is read back."""
        self._count(ground_truth_vec, scores=scores, ignore_label=ignore_label, row_index=row_index, columns=columns)

    # -- reading ------------------------------------------------------------------------------------------------------
    @property
    def confusion_matrix(self):
        if self._host is None:
            C = self.number_of_labels
            flat = self._cm.cpu().numpy() if torch.is_tensor(self._cm) else self._cm.copy()
            if flat[C * C]:
                raise ValueError("%d rows carried a label (or prediction) outside [0, %d) that is not the ignore label"
                                 % (int(flat[C * C]), C))
            self._host = flat[:C * C].reshape(C, C)
        return self._host

    def get_count(self, ground_truth, predicted):
        return self.confusion_matrix[ground_truth][predicted]

    def get_confusion_matrix(self):
        return self.confusion_matrix

    def count_gt(self, ground_truth):
        return self.confusion_matrix[ground_truth, :].sum()

    def get_intersection_union_per_class(self):
        cm = self.confusion_matrix
        TP_plus_FN = np.sum(cm, axis=0)
        TP_plus_FP = np.sum(cm, axis=1)
        TP = np.diagonal(cm)
        union = TP_plus_FN + TP_plus_FP - TP
        iou = 1e-8 + TP / (union + 1e-8)
        existing_class_mask = union > 1e-3
        return iou, existing_class_mask

    def get_overall_accuracy(self):
        cm = self.confusion_matrix
        matrix_diagonal = int(np.trace(cm))  # the reference's double loop sums the same integers
        all_values = int(cm.sum())
        if all_values == 0:
            all_values = 1
        return float(matrix_diagonal) / all_values

    def get_average_intersection_union(self, missing_as_one=False):
        values, existing_classes_mask = self.get_intersection_union_per_class()
        if np.sum(existing_classes_mask) == 0:
            return 0
        if missing_as_one:
            values[~existing_classes_mask] = 1
            existing_classes_mask[:] = True
        return np.sum(values[existing_classes_mask]) / np.sum(existing_classes_mask)

    def get_mean_class_accuracy(self):
        cm = self.confusion_matrix
        re = 0
        label_presents = 0
        for i in range(self.number_of_labels):
            total_gt = np.sum(cm[i, :])
            if total_gt:
                label_presents += 1
                re = re + cm[i][i] / max(1, total_gt)
        if label_presents == 0:
            return 0
        return re / label_presents


# ---------------------------------------------------------------------------------------------------------------------
class SegmentationEvaluator(object):
    """SegmentationTracker on tensors: `track(outputs, labels)` per batch, `get_metrics()` at the end of the epoch.
    The matrix lives on the device of the first tracked outputs; `track` reads nothing back."""

    def __init__(self, num_classes, stage="train", ignore_label=-1):
        self._num_classes = int(num_classes)
        self._ignore_label = ignore_label
        self.reset(stage)

    def reset(self, stage="train"):
        self._stage = stage
        self._confusion_matrix = None

    def _matrix(self, device):
        """the matrix, created on the device of the first tracked outputs; a read before that sees an empty one"""
        if self._confusion_matrix is None:
            if device is None:
                return ConfusionMatrix(self._num_classes)
            self._confusion_matrix = ConfusionMatrix(self._num_classes, device)
        elif device is not None and torch.device(device).type != self._confusion_matrix.device.type:
            raise ValueError("outputs on %s, but the matrix of this epoch lives on %s"
                             % (device, self._confusion_matrix.device))
        return self._confusion_matrix

    @property
    def confusion_matrix(self):
        return self._matrix(None).confusion_matrix

    def track(self, outputs, labels):
        """outputs (N, C) or (B, N, C) scores, labels (N) or (B, N)"""
        outputs = outputs.detach()
        if outputs.dim() != 2:
            outputs = outputs.reshape(-1, outputs.shape[-1])
        if outputs.shape[1] != self._num_classes:
            raise ValueError("outputs have %d columns for %d classes" % (outputs.shape[1], self._num_classes))
        self._matrix(outputs.device).count_scores(labels.reshape(-1), outputs, ignore_label=self._ignore_label)

    def get_metrics(self, verbose=False):
        cm = self._matrix(None)
        metrics = {}
        metrics["{}_acc".format(self._stage)] = 100 * cm.get_overall_accuracy()
        metrics["{}_macc".format(self._stage)] = 100 * cm.get_mean_class_accuracy()
        metrics["{}_miou".format(self._stage)] = 100 * cm.get_average_intersection_union()
        if verbose:
            metrics["{}_iou_per_class".format(self._stage)] = {
                i: "{:.2f}".format(100 * v) for i, v in enumerate(cm.get_intersection_union_per_class()[0])}
        return metrics


# ---------------------------------------------------------------------------------------------------------------------
class ShapenetPartEvaluator(object):
    """ShapenetPartTracker on tensors.  `class_to_segments`: {category: [labels]}, every list a contiguous ascending
    range (the kernel restricts the argmax to a column range), at most PART_IOU_MAX_PARTS labels each.  Per-cloud
    (intersection, union) counts stay on the device until `get_metrics`, which forms the part IoUs (an absent part
    counts as 1), the per-shape means and Cmiou / Imiou in float64 as `_compute_part_ious` and
    `_get_metrics_per_class` do."""

    def __init__(self, class_to_segments, stage="train"):
        self._class_seg_map = {cat: [int(v) for v in segs] for cat, segs in class_to_segments.items()}
        labels = [v for segs in self._class_seg_map.values() for v in segs]
        if not labels or min(labels) < 0 or len(set(labels)) != len(labels):
            raise ValueError("class_to_segments must list every label once")
        self._num_classes = max(labels) + 1
        self._part_lo = np.zeros(self._num_classes, dtype=np.int32)
        self._part_hi = np.zeros(self._num_classes, dtype=np.int32)
        self._lo_to_cat = {}
        for cat, segs in self._class_seg_map.items():
            if segs != list(range(segs[0], segs[0] + len(segs))):
                raise ValueError("category %r lists non-contiguous labels %r" % (cat, segs))
            if len(segs) > PART_IOU_MAX_PARTS:
                raise ValueError("category %r has %d parts, at most %d are served" % (cat, len(segs), PART_IOU_MAX_PARTS))
            self._part_lo[segs] = segs[0]
            self._part_hi[segs] = segs[-1] + 1
            self._lo_to_cat[segs[0]] = cat
        self._max_parts = max(len(s) for s in self._class_seg_map.values())
        self._tables = {}
        self.reset(stage)

    def reset(self, stage="train"):
        self._stage = stage
        self._pending = []  # (counts, cat_lo) per tracked batch, on the device of that batch

    def track(self, outputs, labels, batch=None, seg=None):
        """outputs (N, C) with a sorted batch vector (or cloud offsets `seg` (B + 1), which saves the host read that the
        batch vector's cloud count costs), or dense outputs (B, N, C) and labels (B, N)"""
        outputs = outputs.detach()
        if outputs.dim() == 3:
            B, n, C = outputs.shape
            outputs, labels = outputs.reshape(B * n, C), labels.reshape(B * n)
            seg = torch.arange(B + 1, dtype=torch.int64, device=outputs.device) * n
        if outputs.dim() != 2 or outputs.shape[1] != self._num_classes:
            raise ValueError("outputs must have %d columns, got %s" % (self._num_classes, tuple(outputs.shape)))
        if labels.dim() != 1 or labels.shape[0] != outputs.shape[0]:
            raise ValueError("labels must have one entry per row")
        if _is_gpu(outputs.device):
            seg, _ = _tp._cloud_rows(batch, seg, outputs.shape[0])
            dev = outputs.device
            if dev not in self._tables:
                self._tables[dev] = (torch.from_numpy(self._part_lo).to(dev), torch.from_numpy(self._part_hi).to(dev))
            lo, hi = self._tables[dev]
            self._pending.append(_tp.part_iou_counts(outputs, labels, seg, lo, hi, self._max_parts))
        else:
            if seg is None:
                b = _np(batch, np.int64)
                if b.shape[0] > 1 and (b[1:] < b[:-1]).any():
                    raise ValueError("batch must be sorted")
                seg = np.concatenate([[0], np.cumsum(np.bincount(b))]) if b.shape[0] else np.zeros(1, dtype=np.int64)
            self._pending.append(part_iou_counts_numpy(outputs, labels, seg, self._part_lo, self._part_hi))

    def cloud_counts(self):
        """(counts (clouds, PART_IOU_MAX_PARTS, 2), cat_lo (clouds)) of everything tracked, on the host (one read)"""
        if not self._pending:
            return np.zeros((0, PART_IOU_MAX_PARTS, 2), dtype=np.int32), np.zeros(0, dtype=np.int32)
        if torch.is_tensor(self._pending[0][0]):
            counts = torch.cat([c for c, _ in self._pending]).cpu().numpy()
            cat_lo = torch.cat([l for _, l in self._pending]).cpu().numpy()
        else:
            counts = np.concatenate([c for c, _ in self._pending])
            cat_lo = np.concatenate([l for _, l in self._pending])
        return counts, cat_lo

    def shape_ious(self):
        counts, cat_lo = self.cloud_counts()
        if (cat_lo == -2).any():
            raise ValueError("%d clouds start with a label that belongs to no category" % int((cat_lo == -2).sum()))
        shape_ious = {cat: [] for cat in self._class_seg_map.keys()}
        for b in range(cat_lo.shape[0]):
            if cat_lo[b] < 0:
                continue  # empty cloud
            cat = self._lo_to_cat[int(cat_lo[b])]
            part_ious = np.zeros(len(self._class_seg_map[cat]))
            for p in range(part_ious.shape[0]):
                if counts[b, p, 1] == 0:
                    part_ious[p] = 1  # part is not present in this shape
                else:
                    part_ious[p] = float(counts[b, p, 0]) / float(counts[b, p, 1])
            shape_ious[cat].append(np.mean(part_ious))
        return shape_ious

    @staticmethod
    def _get_metrics_per_class(shape_ious):
        instance_ious = []
        cat_ious = {}
        for cat in shape_ious.keys():
            for iou in shape_ious[cat]:
                instance_ious.append(iou)
            if len(shape_ious[cat]):
                cat_ious[cat] = np.mean(shape_ious[cat])
        mean_class_ious = np.mean(list(cat_ious.values()))
        return cat_ious, mean_class_ious, np.mean(instance_ious)

    def get_metrics(self, verbose=False):
        shape_ious = self.shape_ious()
        metrics = {}
        if not any(len(v) for v in shape_ious.values()):
            miou_per_class, Cmiou, Imiou = {}, 0, 0  # the tracker's values before the first batch
        else:
            miou_per_class, Cmiou, Imiou = self._get_metrics_per_class(shape_ious)
        metrics["{}_Cmiou".format(self._stage)] = Cmiou * 100
        metrics["{}_Imiou".format(self._stage)] = Imiou * 100
        if verbose:
            metrics["{}_Imiou_per_class".format(self._stage)] = miou_per_class
        return metrics


# ---------------------------------------------------------------------------------------------------------------------
class _Votes(object):
    """votes (T, C) fp32 and counts (T) int32 on `device`, with the workspace, epoch and error counter of vote_add"""

    def __init__(self, T, C, device):
        self.device = torch.device(device)
        self.votes = torch.zeros((T, C), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros(T, dtype=torch.int32, device=self.device)
        self.gpu = _is_gpu(self.device)
        self.epoch = 0
        if self.gpu:
            self.workspace = torch.zeros(T, dtype=torch.int64, device=self.device)
            self.errors = torch.zeros(1, dtype=torch.int64, device=self.device)
        else:
            self.errors = 0

    def add(self, ids, out):
        ids = ids.reshape(-1)
        out = out.detach().reshape(-1, out.shape[-1])
        if ids.shape[0] != out.shape[0] or out.shape[1] != self.votes.shape[1]:
            raise ValueError("ids %s do not match outputs %s" % (tuple(ids.shape), tuple(out.shape)))
        if self.gpu:
            self.epoch += 1
            _tp.vote_add(self.votes, self.counts, self.workspace, self.errors, self.epoch, ids.to(self.device), out)
        else:
            self.errors += vote_add_numpy(self.votes, self.counts, ids, out)

    def check(self):
        bad = int(self.errors) if not self.gpu else int(self.errors.item())
        if bad:
            raise ValueError("Origin ids are larger than the number of points in the original point cloud "
                             "(%d ids outside [0, %d))" % (bad, self.votes.shape[0]))


class SegmentationVoter(object):
    """Full-cloud prediction from votes interpolated with kNN (segmentation_helpers.py).  Takes the raw cloud's
    positions and labels instead of a Data object, and origin ids instead of (data, batch_mask); the state lives on
    raw_pos's device.  An id repeated inside one `add_vote` is counted once, with its last row (`torchpoints.vote_add`).
    An id out of range raises at the next read (`coverage`, `full_res_preds`), not in `add_vote`, which reads nothing."""

    def __init__(self, raw_pos, raw_y, num_classes, class_seg_map=None, k=1):
        assert k > 0
        self._pos, self._y = raw_pos, raw_y
        self._num_pos = raw_pos.shape[0]
        self._state = _Votes(self._num_pos, num_classes, raw_pos.device)
        self._class_seg_map = list(class_seg_map) if class_seg_map else None
        self._k = k
        self._num_votes = 0

    @property
    def k(self):
        return self._k

    @k.setter
    def k(self, k):
        if isinstance(k, int):
            if k > 0:
                self._k = k
            else:
                raise Exception("k should be >= 1")
        else:
            raise Exception("k used for knn_interpolate should be an int")

    @property
    def num_votes(self):
        return self._num_votes

    @property
    def votes(self):
        return self._state.votes

    @property
    def vote_counts(self):
        return self._state.counts

    @property
    def coverage(self):
        self._state.check()
        return float(int((self._state.counts > 0).sum())) / self._num_pos

    @property
    def full_res_labels(self):
        return self._y

    def add_vote(self, origin_ids, output):
        self._state.add(origin_ids, output)
        self._num_votes += 1

    def _predict_full_res(self):
        st = self._state
        st.check()
        has_prediction = st.counts > 0
        votes = st.votes[has_prediction].div(st.counts[has_prediction].float().unsqueeze(-1))
        if st.gpu:
            from .partial_dense import knn_interpolate
            return knn_interpolate(votes, self._pos[has_prediction], self._pos, k=self._k)
        return knn_interpolate_numpy(votes, self._pos[has_prediction], self._pos, self._k)

    @property
    def full_res_preds(self):
        full = self._predict_full_res()
        if self._class_seg_map:
            return full[:, self._class_seg_map].argmax(1) + self._class_seg_map[0]
        return full.argmax(-1)

    def __repr__(self):
        return "{}(num_pos={})".format(self.__class__.__name__, self._num_pos)


# ---------------------------------------------------------------------------------------------------------------------
class S3DISEvaluator(SegmentationEvaluator):
    """S3DISTracker on tensors: the test area's `pos` (T, 3) and `y` (T) are given at construction and the votes live on
    their device.  `track(outputs, labels, origin_ids)` adds votes; `finalise` scores them:
      vote_miou       confusion of y against argmax(votes) on the rows that have a prediction;
      full_vote_miou  every raw point takes the votes of its nearest predicted point (the reference's
                      knn_interpolate with k = 1 copies that row up to one rounding of (x w) / w): `torchpoints.knn(1)`
                      gives the row, `count_scores(row_index=...)` reads it; the (T, C) interpolated matrix is not formed.
    Deviation: an origin id out of range raises ValueError at `finalise`, not at `track`, which reads nothing back.
    `label_names` ({class: name}) stands for the dataset's INV_OBJECT_LABEL in the per-class keys."""

    def __init__(self, num_classes, pos, y, stage="test", ignore_label=-1, label_names=None):
        self._pos, self._y = pos, y
        self._label_names = label_names
        super().__init__(num_classes, stage=stage, ignore_label=ignore_label)

    def reset(self, stage="train"):
        super().reset(stage)
        self._test_area = None
        self._full_vote_miou = None
        self._vote_miou = None
        self._full_confusion = None
        self._iou_per_class = {}

    @property
    def votes(self):
        return None if self._test_area is None else self._test_area.votes

    @property
    def prediction_count(self):
        return None if self._test_area is None else self._test_area.counts

    def track(self, outputs, labels, origin_ids=None):
        super().track(outputs, labels)
        if origin_ids is None or self._stage == "train":
            return
        if self._test_area is None:
            self._test_area = _Votes(self._y.shape[0], self._num_classes, self._pos.device)
        self._test_area.add(origin_ids, outputs)

    def finalise(self, full_res=False, vote_miou=True):
        per_class_iou = self._matrix(None).get_intersection_union_per_class()[0]
        names = self._label_names
        self._iou_per_class = {(names[k] if names else k): v for k, v in enumerate(per_class_iou)}
        area = self._test_area
        if area is None:
            return
        area.check()
        has_prediction = area.counts > 0
        rows = torch.arange(has_prediction.shape[0], device=area.device)
        if vote_miou:
            c = ConfusionMatrix(self._num_classes, area.device)
            c.count_scores(self._y, area.votes, row_index=torch.where(has_prediction, rows, torch.full_like(rows, -1)))
            self._vote_miou = c.get_average_intersection_union() * 100
        if full_res and self._full_vote_miou is None:
            predicted = rows[has_prediction]
            if area.gpu:
                nearest = _tp.knn(1, self._pos[predicted], self._pos)[0][:, 0]
            else:
                nearest = knn_host(1, self._pos[predicted], self._pos)[0][:, 0]
            self._full_confusion = ConfusionMatrix(self._num_classes, area.device)
            self._full_confusion.count_scores(self._y, area.votes, row_index=predicted[nearest])
            self._full_vote_miou = self._full_confusion.get_average_intersection_union() * 100

    @property
    def full_confusion_matrix(self):
        return self._full_confusion

    def get_metrics(self, verbose=False):
        metrics = super().get_metrics(verbose)
        if verbose:
            metrics["{}_iou_per_class".format(self._stage)] = self._iou_per_class
            if self._vote_miou:
                metrics["{}_full_vote_miou".format(self._stage)] = self._full_vote_miou
                metrics["{}_vote_miou".format(self._stage)] = self._vote_miou
        return metrics
