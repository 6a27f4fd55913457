"""The host side of the panoptic evaluation (torch_points3d_amd/panoptic_metrics.py): the numpy restatements of the
kernels' rules and the evaluator on CPU tensors.

References, none of them the code under test: the stored results of the reference's own PanopticTracker and
get_instances (tests/golden/panoptic_tracker.npz through tests/panoptic_cases.py), this repository's dense yardsticks
pointgroup.cross_iou / non_max_suppression / instance_iou_csr, and serial Python written here."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc
from torch_points3d_amd import panoptic_metrics as PM
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd.torchpoints import ClusterSet


@pytest.mark.parametrize("thr", [0.25, 0.5])
@pytest.mark.parametrize("as_set", [True, False])
def test_evaluator_against_the_reference_tracker(thr, as_set):
    ev = pc.run_evaluator(thr, "cpu", as_set=as_set)
    pc.check_final(ev, thr)


def test_best_instance_against_the_reference_matches_and_instance_iou():
    checked = 0
    for n in range(3):
        results, labels, batch = pc.batch_inputs(n, "cpu")
        clusters = results.clusters
        column, offsets, per_cloud = pc.columns(labels, batch)
        G = int(per_cloud.sum())
        gt_size = np.bincount(column[column >= 0], minlength=G)
        first = np.full(G, -1)
        for p in range(column.shape[0] - 1, -1, -1):
            if column[p] >= 0:
                first[column[p]] = p
        gt_class = labels.y.numpy()[first]
        head = clusters.members[clusters.starts[:-1]].numpy()
        cloud = batch.numpy()[head]
        cluster_class = results.semantic_logits.argmax(1).numpy()[head]
        best = PM.cluster_best_instance_numpy(clusters, column, gt_size, gt_class, cluster_class, offsets[cloud],
                                              offsets[cloud] + per_cloud[cloud])
        checked += pc.check_matches(n, best, labels, batch, clusters)
        dense = pg.instance_iou_csr(clusters, labels.instance_labels, batch)
        values, indices = dense.max(1)
        positive = values > 0
        assert torch.equal(best[1][positive], indices[positive]) and bool((best[1][~positive] == -1).all())
        fi, size = best[0].float(), clusters.sizes().float()
        iou = fi / ((size + torch.from_numpy(gt_size).float()[best[1].clamp(min=0)]) - fi).clamp(min=1.0)
        assert torch.equal(iou[positive], values[positive])
    assert checked > 20


def test_best_instance_first_maximum_and_no_candidate():
    column, gt_size, gt_class, sets, classes = pc.tie_case()
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    K = len(clusters)
    out = PM.cluster_best_instance_numpy(clusters, column, gt_size, gt_class, np.array(classes), np.zeros(K, dtype=np.int64),
                                         np.full(K, gt_size.shape[0]))
    assert [t.tolist() for t in out] == [list(v) for v in pc.TIE_CASE_ANSWER]


@pytest.mark.parametrize("seed,N,K,lo,hi,dup", [(0, 60, 12, 1, 12, False), (1, 200, 40, 1, 30, True), (2, 30, 1, 5, 5, False),
                                                 (3, 5000, 30, 1, 3, False)])
def test_overlaps_against_cross_iou(seed, N, K, lo, hi, dup):
    rng = np.random.default_rng(seed)
    clusters = pc.random_clusters(rng, N, K, lo, hi, dup)
    ov = PM.cluster_overlaps_numpy(clusters)
    if dup:  # cross_iou counts a repeated point twice; the reference's 0/1 mask, and the sparse form, once
        plain = ClusterSet.from_list([torch.unique(c) for c in clusters.to_list()])
        want = pc.cross_intersections(plain)
    else:
        want = pc.cross_intersections(clusters)
    assert np.array_equal(pc.dense_from_sparse(ov, K), want)
    assert int(ov[0][-1]) == ov[1].numel() == int((want > 0).sum())


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("threshold", [0.3, 0.1])
def test_nms_against_the_dense_suppression(seed, threshold):
    rng = np.random.default_rng(10 + seed)
    K = 50
    clusters = pc.random_clusters(rng, 120, K, 2, 25, windows=True)
    scores = torch.from_numpy(rng.permutation(K).astype(np.float32) / K)
    keep, order = PM.cluster_nms_numpy(clusters, scores, threshold)
    want = pg.non_max_suppression(pg.cross_iou(clusters).numpy(), scores.numpy(), threshold)
    assert order[keep[order]].tolist() == [int(i) for i in want]
    assert 0 < int(keep.sum()) < K


def test_nms_exact_three_tenths_and_chain():
    st = list(range(100))
    # 6 and 7 points with 3 shared: IoU 3 / 10, not above 0.3 in float32; 6 and 6 with 3 shared: 1 / 3
    # chain A-B-C: A kills B, so B cannot kill C
    sets = [st[0:6], st[3:10], st[20:26], st[23:29], st[40:50], st[44:54], st[48:58]]
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3])
    keep, order = PM.cluster_nms_numpy(clusters, scores, 0.3)
    assert keep.tolist() == [True, True, True, False, True, False, True]
    want = pg.non_max_suppression(pg.cross_iou(clusters).numpy(), scores.numpy(), 0.3)
    assert order[keep[order]].tolist() == [int(i) for i in want]


def test_nms_tie_rule_is_a_stable_sort_read_from_the_back():
    rng = np.random.default_rng(5)
    K = 40
    clusters = pc.random_clusters(rng, 80, K, 2, 20, windows=True)
    scores = torch.from_numpy(rng.integers(0, 4, K).astype(np.float32) / 4)  # four distinct values
    keep, order = PM.cluster_nms_numpy(clusters, scores, 0.2)
    visiting = sorted(range(K), key=lambda i: (-float(scores[i]), -i))
    assert order.tolist() == visiting
    iou = pg.cross_iou(clusters).numpy()
    alive, picked = np.ones(K, dtype=bool), []
    for i in visiting:
        if alive[i]:
            picked.append(i)
            alive &= ~(iou[i] > np.float32(0.2))
    assert order[keep[order]].tolist() == picked


def test_refusals():
    ev = PM.PanopticEvaluator(6)
    results, labels, batch = pc.batch_inputs(0, "cpu")
    with pytest.raises(ValueError, match="iou_threshold"):
        ev.track(results, labels, batch, iou_threshold=0.0)
    clusters = results.clusters
    with pytest.raises(ValueError, match="one score per cluster"):
        PM.cluster_nms_numpy(clusters, results.cluster_scores[:-1], 0.3)
    # no batch vector: only the semantic part is tracked; nothing at all: empty metrics
    ev.track(results, labels)
    ev.finalise()
    m = ev.get_metrics()
    assert m["train_pos"] == 0.0 and m["train_Iacc"] == 0.0 and "train_map" not in m and m["train_acc"] > 0


def test_instance_id_beyond_num_instances_is_reported_at_the_end():
    results, labels, batch = pc.batch_inputs(0, "cpu")
    fewer = labels.num_instances.clone()
    fewer[0] -= 1
    ev = PM.PanopticEvaluator(6, stage="val")
    ev.track(results, labels._replace(num_instances=fewer), batch)
    with pytest.raises(ValueError, match="num_instances"):
        ev.finalise()


def test_batch_without_instances_is_skipped():
    results, labels, batch = pc.batch_inputs(0, "cpu")
    empty = labels._replace(instance_labels=torch.zeros_like(labels.instance_labels),
                            num_instances=torch.zeros_like(labels.num_instances))
    ev = PM.PanopticEvaluator(6, stage="val")
    ev.track(results, empty, batch)  # the reference raises ZeroDivisionError here
    ev.finalise()
    m = ev.get_metrics()
    assert m["val_pos"] == 0.0 and m["val_neg"] == 0.0 and "val_map" not in m
