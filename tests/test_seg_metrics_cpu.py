"""Segmentation metrics without a GPU (torch_points3d_amd/seg_metrics.py): CPU tensors take the numpy restatement of the
counting kernels, which must reproduce tests/golden/seg_metrics.npz -- the reference's own ConfusionMatrix,
SegmentationTracker, ShapenetPartTracker, S3DISTracker and SegmentationVoter -- exactly: matrices and counts with
array_equal, metrics equal as float64, votes with torch.equal.  Shared checks: tests/seg_metrics_cases.py."""
import os
import re

import numpy as np
import pytest
import torch

import seg_metrics_cases as sc
from conftest import ROOT
from torch_points3d_amd import _lib
from torch_points3d_amd import seg_metrics as SM

CPU = "cpu"


def test_fixture_a_confusion_and_metrics_after_each_batch():
    sc.check_fixture_a(CPU)


def test_fixture_b_shapenet_part_ious_ragged_and_dense():
    sc.check_fixture_b(CPU)


def test_fixture_c_s3dis_votes_and_full_resolution():
    sc.check_fixture_c(CPU)


def test_fixture_d_voters_with_class_seg_map():
    sc.check_fixture_d(CPU)


def test_create_from_matrix_round_trip():
    g = sc.golden()
    c = SM.ConfusionMatrix.create_from_matrix(g["a_cm_2"])
    assert c.number_of_labels == 13 and np.array_equal(c.get_confusion_matrix(), g["a_cm_2"])
    assert 100 * c.get_overall_accuracy() == g["a_metrics_2"][0]
    assert 100 * c.get_mean_class_accuracy() == g["a_metrics_2"][1]
    assert 100 * c.get_average_intersection_union() == g["a_metrics_2"][2]
    again = SM.ConfusionMatrix.create_from_matrix(c.get_confusion_matrix())
    again.count_predicted_batch(np.array([0, 1, 1]), np.array([0, 1, 2]))
    want = g["a_cm_2"].copy()
    want[0, 0] += 1
    want[1, 1] += 1
    want[1, 2] += 1
    assert np.array_equal(again.get_confusion_matrix(), want)


def test_count_predicted_batch_is_the_reference_bincount():
    rng = np.random.RandomState(0)
    gt, pred = rng.randint(0, 7, 500), rng.randint(0, 7, 500)
    c = SM.ConfusionMatrix(7)
    c.count_predicted_batch(torch.from_numpy(gt), torch.from_numpy(pred))
    assert np.array_equal(c.get_confusion_matrix(), np.bincount(7 * gt + pred, minlength=49).reshape(7, 7))
    assert c.get_count(2, 3) == int(((gt == 2) & (pred == 3)).sum())


def test_non_contiguous_category_is_refused():
    with pytest.raises(ValueError, match="non-contiguous"):
        SM.ShapenetPartEvaluator({"A": [0, 1, 3], "B": [2]})
    with pytest.raises(ValueError, match="parts"):
        SM.ShapenetPartEvaluator({"A": list(range(SM.PART_IOU_MAX_PARTS + 1))})


def test_invalid_label_raises_at_read_and_counts_nothing():
    c = SM.ConfusionMatrix(4)
    scores = torch.zeros(3, 4)
    c.count_scores(torch.tensor([1, 4, -1]), scores, ignore_label=-1)  # 4 is out of range, -1 is ignored
    assert c._cm[:16].sum() == 1 and c._cm[16] == 1 and c._cm[1 * 4 + 0] == 1
    with pytest.raises(ValueError, match="outside"):
        c.get_confusion_matrix()


def test_row_index_and_columns_on_the_host():
    scores = torch.tensor([[0.0, 5.0, 9.0], [3.0, 1.0, 9.0], [1.0, 1.0, 9.0]])
    c = SM.ConfusionMatrix(3)
    c.count_scores(torch.tensor([0, 1, 2, 2]), scores, row_index=torch.tensor([2, -1, 0, 0]), columns=(0, 2))
    want = np.zeros((3, 3), dtype=np.int64)
    want[0, 0] += 1  # row 2: tie of columns 0 and 1 -> 0
    want[2, 1] += 2  # row 0 twice
    assert np.array_equal(c.get_confusion_matrix(), want)


def test_vote_duplicate_rule_and_bad_id_on_the_host():
    ev = SM.S3DISEvaluator(3, torch.rand(10, 3), torch.randint(0, 3, (10,)), stage="test")
    out = torch.tensor([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 4.0]])
    ev.track(out, torch.tensor([0, 1, 2]), torch.tensor([7, 3, 7]))
    assert ev.votes[7].tolist() == [0, 0, 4.0] and ev.prediction_count[7] == 1 and ev.votes[3].tolist() == [0, 2.0, 0]
    ev.track(out, torch.tensor([0, 1, 2]), torch.tensor([1, 10, 2]))
    with pytest.raises(ValueError, match="Origin ids"):
        ev.finalise()


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tp3d_hip.h")).read()
    for name in ("tp3d_confusion_count_f32", "tp3d_part_iou_counts_f32", "tp3d_vote_add_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    assert int(re.search(r"#define TP3D_PART_IOU_MAX_PARTS (\d+)", header).group(1)) == SM.PART_IOU_MAX_PARTS >= 8


def test_gpu_wrappers_refuse_cpu_tensors():
    from torch_points3d_amd import torchpoints as tp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.confusion_count(torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), scores=torch.zeros(3, 2))
