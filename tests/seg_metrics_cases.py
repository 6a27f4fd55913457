"""Checks shared by tests/test_seg_metrics_cpu.py and tests/test_gpu_seg_metrics.py: the four evaluators of
torch_points3d_amd/seg_metrics.py on a device against tests/golden/seg_metrics.npz (the reference's own trackers).

Bars: counters and matrices np.array_equal; metrics == as float64 (the host arithmetic is the reference's, on equal
integers); votes torch.equal; full-resolution predictions equal on every row (the generator asserts the gaps that make
them rounding-proof)."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN
from torch_points3d_amd import seg_metrics as SM

_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(os.path.join(GOLDEN, "seg_metrics.npz")) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def seg_classes():
    return json.loads(str(golden()["b_seg_classes_json"]))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_fixture_a(dev):
    g = golden()
    ev = SM.SegmentationEvaluator(13, stage="val", ignore_label=-1)
    seen = []
    for b in range(3):
        ev.track(T(g["a_scores_%d" % b], dev), T(g["a_labels_%d" % b], dev))
        m = ev.get_metrics(verbose=True)
        assert np.array_equal(ev.confusion_matrix, g["a_cm_%d" % b])
        got = np.array([m["val_acc"], m["val_macc"], m["val_miou"]], dtype=np.float64)
        assert np.array_equal(got, g["a_metrics_%d" % b]), (got, g["a_metrics_%d" % b])
        assert [m["val_iou_per_class"][i] for i in range(13)] == list(g["a_iou_strings_%d" % b])
        c = ev._confusion_matrix
        iou, mask = c.get_intersection_union_per_class()
        assert np.array_equal(iou, g["a_iou_%d" % b]) and np.array_equal(mask, g["a_mask_%d" % b])
        assert np.float64(c.get_average_intersection_union(missing_as_one=True)) == g["a_miou_missing_as_one_%d" % b]
        assert np.array_equal(np.array([c.count_gt(i) for i in range(13)]), g["a_count_gt_%d" % b])
        assert c.get_count(3, 3) == g["a_cm_%d" % b][3][3]
        seen.append(got)
    ev.reset("val")
    assert ev.get_metrics() == {"val_acc": 0.0, "val_macc": 0, "val_miou": 0}
    return seen


def check_fixture_b(dev):
    g = golden()
    ev = SM.ShapenetPartEvaluator(seg_classes(), stage="test")
    ev.track(T(g["b_scores"], dev), T(g["b_labels"], dev), T(g["b_batch"], dev))
    m = ev.get_metrics(verbose=True)
    got = np.array([m["test_Cmiou"], m["test_Imiou"]], dtype=np.float64)
    assert np.array_equal(got, g["b_metrics"]), (got, g["b_metrics"])
    assert list(m["test_Imiou_per_class"].keys()) == list(g["b_per_class_names"])
    assert np.array_equal(np.array(list(m["test_Imiou_per_class"].values()), dtype=np.float64), g["b_per_class"])
    counts, cat_lo = ev.cloud_counts()
    classes = seg_classes()
    assert [int(v) for v in cat_lo] == [classes[c][0] for c in g["b_cats"]]
    assert counts[4, 3].tolist() == [0, 0]  # part 33 of the second Motorbike: absent from labels and predictions
    dense = SM.ShapenetPartEvaluator(classes, stage="test")
    dense.track(T(g["b_dense_scores"], dev), T(g["b_dense_labels"], dev))
    md = dense.get_metrics(verbose=True)
    gotd = np.array([md["test_Cmiou"], md["test_Imiou"]], dtype=np.float64)
    assert np.array_equal(gotd, g["b_dense_metrics"])
    assert list(md["test_Imiou_per_class"].keys()) == list(g["b_dense_per_class_names"])
    assert np.array_equal(np.array(list(md["test_Imiou_per_class"].values()), dtype=np.float64), g["b_dense_per_class"])
    return got, gotd, counts


def check_fixture_c(dev):
    g = golden()
    names = {i: "class%d" % i for i in range(13)}
    ev = SM.S3DISEvaluator(13, T(g["c_pos"], dev), T(g["c_y"], dev), stage="test", ignore_label=-1, label_names=names)
    for j in range(4):
        ids = T(g["c_ids_%d" % j], dev)
        ev.track(T(g["c_out_%d" % j], dev), T(g["c_labels_%d" % j], dev), ids.reshape(2, -1) if j == 1 else ids)
    ev.finalise(full_res=True, vote_miou=True)
    m = ev.get_metrics(verbose=True)
    assert torch.equal(ev.votes.cpu(), torch.from_numpy(g["c_votes"]))
    assert np.array_equal(ev.prediction_count.cpu().numpy(), g["c_counts"])
    assert np.array_equal(ev.confusion_matrix, g["c_cm"])
    got = np.array([m["test_acc"], m["test_macc"], m["test_miou"], m["test_vote_miou"], m["test_full_vote_miou"]],
                   dtype=np.float64)
    want = np.concatenate([g["c_metrics"], [g["c_vote_miou"], g["c_full_vote_miou"]]])
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(ev.full_confusion_matrix.get_confusion_matrix(), g["c_full_cm"])
    assert np.array_equal(np.array([m["test_iou_per_class"]["class%d" % i] for i in range(13)]), g["c_iou_per_class"])
    return got


def check_fixture_d(dev):
    g = golden()
    preds = []
    for name in ("d1", "d3"):
        voter = SM.SegmentationVoter(T(g[name + "_pos"], dev), T(g[name + "_y"], dev), 50,
                                     class_seg_map=[int(v) for v in g[name + "_map"]], k=int(g[name + "_k"]))
        for j in range(3):
            voter.add_vote(T(g["%s_ids_%d" % (name, j)], dev), T(g["%s_out_%d" % (name, j)], dev))
        assert voter.num_votes == int(g[name + "_num_votes"]) and voter.coverage == float(g[name + "_coverage"])
        assert np.array_equal(voter.vote_counts.cpu().numpy(), g[name + "_counts"].astype(np.int32))
        p = voter.full_res_preds.cpu().numpy()
        assert np.array_equal(p, g[name + "_preds"]), int((p != g[name + "_preds"]).sum())
        assert torch.equal(voter.full_res_labels.cpu(), torch.from_numpy(g[name + "_y"]))
        preds.append(p)
    return preds
