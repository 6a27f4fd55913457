"""Generator of tests/golden/seg_metrics.npz: the REFERENCE's segmentation trackers on the CPU (data only).

Runs the reference's own classes, loaded from the reference tree:
  * `ConfusionMatrix` (metrics/confusion_matrix.py), loaded by file path;
  * `SegmentationTracker`, `ShapenetPartTracker`, `S3DISTracker` (metrics/segmentation_tracker.py,
    shapenet_part_tracker.py, s3dis_tracker.py) and `SegmentationVoter` (metrics/segmentation_helpers.py), imported from
    the tree behind `sys.modules` stand-ins for what is not installed or not needed: torchnet, wandb,
    torch.utils.tensorboard, torch_geometric (make_golden.py's stubs plus `nn.unpool`), and two one-name modules,
    `torch_points3d.datasets.segmentation` (IGNORE_LABEL = -1, read from the reference's file) and
    `torch_points3d.core.data_transform` (SaveOriginalPosId.KEY = "origin_id", grid_transform.py:149), whose real
    packages import every dataset and transform;
  * `knn_interpolate` is make_golden_mp.py's binding (oracle kNN + the published inverse-squared-distance blend);
  * ShapeNet's `seg_classes` table is parsed out of datasets/segmentation/shapenet.py (the module itself imports the
    dataset stack) and stored as JSON text.
The trackers are driven through their public `track(model, ...)` with a minimal model / dataset object that only hands
over the tensors; no line of the trackers is restated.

Fixtures (inputs are rounded to 10 mantissa bits before anything runs; the rounded values ARE the inputs):
  (a) 13 classes, three batches of log-softmax scores, ~10 % labels -1, rows with tied maxima, class 12 absent from
      labels and predictions; the matrix and every metric after each batch.
  (b) ShapeNet's 16 categories / 50 labels, 8 ragged clouds of 1, 63, 64, 65, 300, 257, 128 and 40 points with a Motorbike
      (6 parts), one part absent from labels and predictions alike, labels of another category inside a cloud, rows whose
      unrestricted argmax lies outside the category (asserted); and 4 dense clouds of 64 points.
  (c) a 3000-point area, four vote calls with ids unique inside a call and overlapping between calls, coverage < 100 %.
  (d) two voters with `class_seg_map`, k = 1 and k = 3.
For (c) and (d) it is asserted that no two predicted positions coincide, that the squared distances of every raw point
to its k + 1 nearest predicted points differ (relative gap > 1e-5), that every voted row's top-two gap is at least 1e-3
of its maximum and (d) that every interpolated row's top-two gap inside the map is at least 1e-4 of its maximum: rounding
in (x w) / w or in the interpolation weights can then flip no argmax.

    python tests/golden/make_golden_seg_metrics.py
"""
import ast
import importlib.util
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_mp as mgmp  # noqa: E402

C13 = 13


def quantise(t):
    """keep 10 mantissa bits (the archive compresses; the rounded values are the inputs of every pass)"""
    return (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def load_reference():
    mg.install_stubs()
    mg._stub("torchnet", meter=mg._stub("torchnet.meter", AverageValueMeter=object))
    mg._stub("wandb")
    mg._stub("torch.utils.tensorboard", SummaryWriter=object)
    mg._stub("torch_geometric.nn.unpool", knn_interpolate=mgmp.knn_interpolate)
    text = open(os.path.join(mg.REF, "torch_points3d/datasets/segmentation/__init__.py")).read()
    mg._stub("torch_points3d.datasets.segmentation", IGNORE_LABEL=int(re.search(r"IGNORE_LABEL: int = (-?\d+)", text).group(1)))
    text = open(os.path.join(mg.REF, "torch_points3d/core/data_transform/grid_transform.py")).read()
    key = re.search(r"class SaveOriginalPosId:.*?KEY = \"(\w+)\"", text, flags=re.S).group(1)
    mg._stub("torch_points3d.core.data_transform", SaveOriginalPosId=type("SaveOriginalPosId", (), {"KEY": key}))
    spec = importlib.util.spec_from_file_location(
        "_ref_confusion_matrix", os.path.join(mg.REF, "torch_points3d/metrics/confusion_matrix.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    from torch_points3d.metrics.s3dis_tracker import S3DISTracker
    from torch_points3d.metrics.segmentation_helpers import SegmentationVoter
    from torch_points3d.metrics.segmentation_tracker import SegmentationTracker
    from torch_points3d.metrics.shapenet_part_tracker import ShapenetPartTracker
    return cm.ConfusionMatrix, SegmentationTracker, ShapenetPartTracker, S3DISTracker, SegmentationVoter, key


def shapenet_seg_classes():
    text = open(os.path.join(mg.REF, "torch_points3d/datasets/segmentation/shapenet.py")).read()
    return ast.literal_eval(re.search(r"seg_classes = (\{.*?\})", text, flags=re.S).group(1))


class Model(object):
    """what a tracker asks of a model: the tensors of one batch"""
    conv_type = "PARTIAL_DENSE"
    device = "cpu"

    def __init__(self, output, labels, batch=None):
        self._o, self._l, self._b = output, labels, batch

    def get_output(self):
        return self._o

    def get_labels(self):
        return self._l

    def get_batch(self):
        return self._b

    def get_current_losses(self):
        return {}


class Area(dict):
    """the test area / a batch: attribute and item access, `clone` and `to` as the S3DIS tracker uses them"""
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__

    def clone(self):
        return Area(self)

    def to(self, device):
        return self


class Dataset(object):
    def __init__(self, num_classes, **kw):
        self.num_classes = num_classes
        self.__dict__.update(kw)

    def has_labels(self, stage):
        return True


def scores_for(labels, C, gen, hit=0.7, boost=4.0):
    """log-softmax of noise with the label's column raised for a share `hit` of the rows"""
    n = labels.shape[0]
    s = 2.0 * torch.randn(n, C, generator=gen)
    raised = (torch.rand(n, generator=gen) < hit) & (labels >= 0) & (labels < C)
    s[raised, labels[raised]] += boost
    return quantise(torch.log_softmax(s, 1))


def case_a(out, ConfusionMatrix, SegmentationTracker):
    gen = torch.Generator().manual_seed(101)
    tracker = SegmentationTracker(Dataset(C13), stage="val", ignore_label=-1)
    sizes = [500, 777, 1024]
    for b, n in enumerate(sizes):
        labels = torch.randint(0, C13 - 1, (n,), generator=gen)  # class 12 never labelled ...
        labels[torch.rand(n, generator=gen) < 0.1] = -1
        scores = scores_for(labels, C13, gen)
        scores[:, C13 - 1] = -30.0  # ... and never predicted
        tied = torch.randperm(n, generator=gen)[:n // 16]
        top = scores[tied].max(1)
        other = (top.indices + 1 + torch.randint(0, C13 - 2, (tied.shape[0],), generator=gen)) % (C13 - 1)
        scores[tied, other] = top.values  # two columns hold the maximum
        if b == 1:
            scores[:5] = scores[0, 0]  # all-equal rows
        tracker.track(Model(scores, labels))
        m = tracker.get_metrics(verbose=True)
        out["a_scores_%d" % b], out["a_labels_%d" % b] = scores.numpy(), labels.numpy()
        out["a_cm_%d" % b] = np.array(tracker.confusion_matrix)
        out["a_metrics_%d" % b] = np.array([m["val_acc"], m["val_macc"], m["val_miou"]], dtype=np.float64)
        out["a_iou_strings_%d" % b] = np.array([m["val_iou_per_class"][i] for i in range(C13)])
        c = ConfusionMatrix.create_from_matrix(np.array(tracker.confusion_matrix))
        iou, mask = c.get_intersection_union_per_class()
        out["a_iou_%d" % b], out["a_mask_%d" % b] = iou, mask
        out["a_miou_missing_as_one_%d" % b] = np.float64(c.get_average_intersection_union(missing_as_one=True))
        out["a_count_gt_%d" % b] = np.array([c.count_gt(i) for i in range(C13)])
        assert c.get_overall_accuracy() * 100 == m["val_acc"] and not mask[C13 - 1] and mask[:C13 - 1].all()


def part_clouds(seg_classes, sizes, cats, gen, foreign=None, absent=None):
    """(scores, labels, batch): cloud i of sizes[i] points of category cats[i]; `absent` = (cloud, part) never labelled
    nor predicted; `foreign` = cloud with some labels of another category (not in its first row)"""
    scores, labels, batch = [], [], []
    for i, (n, cat) in enumerate(zip(sizes, cats)):
        segs = seg_classes[cat]
        parts = [p for p in segs if not (absent and absent[0] == i and p == absent[1])]
        l = torch.tensor(parts)[torch.randint(0, len(parts), (n,), generator=gen)]
        s = scores_for(l, 50, gen, hit=0.6, boost=3.0)
        if absent and absent[0] == i:
            s[:, absent[1]] = -40.0
        if foreign == i:
            l[1::7] = (segs[-1] + 3) % 50
        if n >= 64:  # ties inside the category
            s[5, segs[0]:segs[-1] + 1] = s[5, segs[0]]
        scores.append(s), labels.append(l), batch.append(torch.full((n,), i, dtype=torch.long))
    return torch.cat(scores), torch.cat(labels), torch.cat(batch)


def case_b(out, ShapenetPartTracker):
    seg_classes = shapenet_seg_classes()
    assert len(seg_classes) == 16 and sum(len(v) for v in seg_classes.values()) == 50
    out["b_seg_classes_json"] = np.array(json.dumps(seg_classes))
    gen = torch.Generator().manual_seed(202)
    dataset = Dataset(50, class_to_segments=seg_classes)
    sizes = [1, 63, 64, 65, 300, 257, 128, 40]
    cats = ["Bag", "Airplane", "Chair", "Motorbike", "Motorbike", "Table", "Airplane", "Lamp"]
    scores, labels, batch = part_clouds(seg_classes, sizes, cats, gen, foreign=5, absent=(4, 33))
    lo = torch.tensor([seg_classes[cats[b]][0] for b in batch.tolist()])
    hi = torch.tensor([seg_classes[cats[b]][-1] + 1 for b in batch.tolist()])
    free = scores.argmax(1)
    assert int(((free < lo) | (free >= hi)).sum()) > 0  # unrestricted argmax outside the category
    assert int((labels[batch == 4] == 33).sum()) == 0
    tracker = ShapenetPartTracker(dataset, stage="test")
    tracker.track(Model(scores, labels, batch))
    m = tracker.get_metrics(verbose=True)
    out["b_scores"], out["b_labels"], out["b_batch"] = scores.numpy(), labels.numpy(), batch.numpy()
    out["b_cats"] = np.array(cats)
    out["b_metrics"] = np.array([m["test_Cmiou"], m["test_Imiou"]], dtype=np.float64)
    out["b_per_class_names"] = np.array(list(m["test_Imiou_per_class"].keys()))
    out["b_per_class"] = np.array(list(m["test_Imiou_per_class"].values()), dtype=np.float64)
    # dense: 4 clouds of 64 points, tracked after the ragged batch by a fresh tracker
    dsizes, dcats = [64] * 4, ["Car", "Mug", "Motorbike", "Car"]
    scores, labels, batch = part_clouds(seg_classes, dsizes, dcats, gen)
    tracker = ShapenetPartTracker(dataset, stage="test")
    tracker.track(Model(scores, labels, batch))
    m = tracker.get_metrics(verbose=True)
    out["b_dense_scores"], out["b_dense_labels"] = scores.reshape(4, 64, 50).numpy(), labels.reshape(4, 64).numpy()
    out["b_dense_metrics"] = np.array([m["test_Cmiou"], m["test_Imiou"]], dtype=np.float64)
    out["b_dense_per_class_names"] = np.array(list(m["test_Imiou_per_class"].keys()))
    out["b_dense_per_class"] = np.array(list(m["test_Imiou_per_class"].values()), dtype=np.float64)


def check_geometry(pos, has, k):
    """no two predicted positions coincide; the k + 1 nearest predicted squared distances of every raw point differ"""
    p = pos[has].double()
    d = ((pos.double()[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    pp = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    pp.fill_diagonal_(1.0)
    assert float(pp.min()) > 0.0
    near = d.sort(1).values[:, :k + 1]
    gap = (near[:, 1:] - near[:, :-1]) / near[:, 1:]
    assert float(gap.min()) > 1e-5, float(gap.min())


def check_votes(votes, rows, cols=None, rel=1e-3):
    v = votes[rows] if cols is None else votes[rows][:, cols]
    top = v.double().topk(2, dim=1).values
    assert float(((top[:, 0] - top[:, 1]) / v.double().abs().max(1).values).min()) >= rel


def vote_calls(T, C, y, calls, rows, pool, gen, hit=0.8):
    """`calls` x (ids (rows) unique inside the call, drawn from the first `pool` entries of one permutation; outputs)"""
    perm = torch.randperm(T, generator=gen)[:pool]
    out = []
    for _ in range(calls):
        ids = perm[torch.randperm(pool, generator=gen)[:rows]]
        out.append((ids, scores_for(y[ids], C, gen, hit=hit, boost=5.0)))
    return settle(out, T, C)


def settle(calls, T, C, rel=2e-3):
    """raise the leading column of every voted row whose top-two gap is below `rel` of its maximum by 1 (in the last
    call that names the row) until none is left: the inputs are arbitrary, the gap is what the exact tests need"""
    while True:
        votes = torch.zeros(T, C)
        for ids, o in calls:
            votes[ids] += o
        top = votes.double().topk(2, dim=1)
        close = (top.values[:, 0] - top.values[:, 1]) < rel * votes.double().abs().max(1).values
        close &= votes.abs().sum(1) > 0
        if not bool(close.any()):
            return calls
        for t in close.nonzero().flatten().tolist():
            for ids, o in reversed(calls):
                row = (ids == t).nonzero().flatten()
                if row.numel():
                    o[row[0], top.indices[t, 0]] += 1.0
                    break


def case_c(out, S3DISTracker, key):
    T = 3000
    for seed in range(303, 403):
        gen = torch.Generator().manual_seed(seed)
        pos = quantise(10.0 * torch.rand(T, 3, generator=gen))
        y = torch.randint(0, C13, (T,), generator=gen)
        calls = vote_calls(T, C13, y, 4, 700, 2200, gen)
        votes = torch.zeros(T, C13)
        for ids, o in calls:
            votes[ids] += o
        has = torch.zeros(T, dtype=torch.bool)
        has[torch.cat([ids for ids, _ in calls])] = True
        try:
            check_geometry(pos, has, 1)
            check_votes(votes, has)
            break
        except AssertionError:
            continue
    else:
        raise RuntimeError("no seed met the conditions")
    dataset = Dataset(C13, test_data=Area(pos=pos, y=y), INV_OBJECT_LABEL={i: "class%d" % i for i in range(C13)})
    tracker = S3DISTracker(dataset, stage="test", ignore_label=-1)
    for j, (ids, o) in enumerate(calls):
        labels = y[ids].clone()
        labels[::19] = -1
        ids_in = ids.reshape(2, -1) if j == 1 else ids  # 2-D ids are flattened by the tracker
        tracker.track(Model(o, labels), full_res=True, data=Area({key: ids_in}))
        out["c_ids_%d" % j], out["c_out_%d" % j], out["c_labels_%d" % j] = ids.numpy(), o.numpy(), labels.numpy()
    tracker.finalise(full_res=True, vote_miou=True)
    m = tracker.get_metrics(verbose=True)
    area = tracker._test_area
    assert torch.equal(area.votes, votes) and 0 < int((area.prediction_count > 0).sum()) < T
    out["c_seed"], out["c_pos"], out["c_y"] = np.int64(seed), pos.numpy(), y.numpy()
    out["c_votes"], out["c_counts"] = area.votes.numpy(), area.prediction_count.numpy()
    out["c_cm"] = np.array(tracker.confusion_matrix)
    out["c_metrics"] = np.array([m["test_acc"], m["test_macc"], m["test_miou"]], dtype=np.float64)
    out["c_vote_miou"], out["c_full_vote_miou"] = np.float64(m["test_vote_miou"]), np.float64(m["test_full_vote_miou"])
    out["c_full_cm"] = np.array(tracker.full_confusion_matrix.get_confusion_matrix())
    out["c_iou_per_class"] = np.array([m["test_iou_per_class"]["class%d" % i] for i in range(C13)], dtype=np.float64)


def case_d(out, SegmentationVoter, key):
    T, C = 600, 50
    seg_classes = shapenet_seg_classes()
    for name, cat, k, seed0 in (("d1", "Motorbike", 1, 404), ("d3", "Chair", 3, 505)):
        segs = seg_classes[cat]
        for seed in range(seed0, seed0 + 100):
            gen = torch.Generator().manual_seed(seed)
            pos = quantise(torch.rand(T, 3, generator=gen))
            y = torch.tensor(segs)[torch.randint(0, len(segs), (T,), generator=gen)]
            calls = vote_calls(T, C, y, 3, 200, 420, gen)
            voter = SegmentationVoter(Area(pos=pos, y=y), C, "PARTIAL_DENSE", class_seg_map=segs, k=k)
            for ids, o in calls:
                voter.add_vote(Area({key: ids}), o, slice(None))
            has = voter._vote_counts > 0
            try:
                check_geometry(pos, has, k)
                check_votes(voter._votes, has)
                preds = voter.full_res_preds
                check_votes(voter._full_res_preds, slice(None), cols=segs, rel=1e-4)
                break
            except AssertionError:
                continue
        else:
            raise RuntimeError("no seed met the conditions")
        for j, (ids, o) in enumerate(calls):
            out["%s_ids_%d" % (name, j)], out["%s_out_%d" % (name, j)] = ids.numpy(), o.numpy()
        out[name + "_seed"], out[name + "_pos"], out[name + "_y"] = np.int64(seed), pos.numpy(), y.numpy()
        out[name + "_map"], out[name + "_k"] = np.array(segs), np.int64(k)
        out[name + "_counts"] = voter._vote_counts.numpy()
        out[name + "_coverage"], out[name + "_num_votes"] = np.float64(voter.coverage), np.int64(voter.num_votes)
        out[name + "_preds"] = preds.numpy()
        assert torch.equal(voter.full_res_labels, y) and 0.0 < voter.coverage < 1.0


def main():
    ConfusionMatrix, SegmentationTracker, ShapenetPartTracker, S3DISTracker, SegmentationVoter, key = load_reference()
    out = {}
    case_a(out, ConfusionMatrix, SegmentationTracker)
    case_b(out, ShapenetPartTracker)
    case_c(out, S3DISTracker, key)
    case_d(out, SegmentationVoter, key)
    path = os.path.join(HERE, "seg_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
