"""The stored results of the reference's panoptic tracker (tests/golden/panoptic_tracker.npz, written by
tests/golden/make_golden_panoptic_tracker.py) and the comparisons both the CPU and the GPU tests make against them.
Lists, flags and matched ids are compared exactly; metrics within 1e-12 absolute: they are ratios of small integers in
[0, 1], a handful of float64 roundings apart from the reference's running mean."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN
from torch_points3d_amd import panoptic_metrics as PM
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd.pointgroup import PanopticLabels, PanopticResults
from torch_points3d_amd.torchpoints import ClusterSet

BAR = 1e-12
_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(os.path.join(GOLDEN, "panoptic_tracker.npz"))
        _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def tag(thr):
    return "t%02d" % int(round(100 * thr))


def batch_inputs(n, device, as_set=True):
    """(PanopticResults, PanopticLabels, batch) of stored batch n on `device`"""
    z = fixture()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    sizes = z["b%d_sizes" % n]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    members = z["b%d_members" % n]
    y, inst, batch = T(z["b%d_y" % n]), T(z["b%d_inst" % n]), T(z["b%d_batch" % n])
    logits = T(z["b%d_logits" % n])
    if as_set:
        clusters = ClusterSet(T(members), T(starts), label=None, cloud=None)
    else:
        clusters = [T(members[starts[k]:starts[k + 1]]) for k in range(sizes.shape[0])]
    N = y.shape[0]
    zeros = torch.zeros(N, 3, device=device)
    results = PanopticResults(semantic_logits=logits, offset_logits=zeros, cluster_scores=T(z["b%d_scores" % n]), clusters=clusters,
                              cluster_type=torch.zeros(sizes.shape[0], dtype=torch.uint8, device=device))
    labels = PanopticLabels(center_label=zeros, y=y, num_instances=T(z["b%d_num_instances" % n]), instance_labels=inst,
                            instance_mask=inst > 0, vote_label=zeros)
    return results, labels, batch


def random_clusters(rng, N, K, lo, hi, dup=False, windows=False):
    """K clusters of lo..hi points out of N: scattered, or (windows) runs of neighbouring points, which overlap a lot"""
    sets = []
    for _ in range(K):
        n = int(rng.integers(lo, hi + 1))
        c = np.sort(rng.choice(N, n, replace=False)) if not windows else int(rng.integers(0, N - n + 1)) + np.arange(n)
        if dup and n > 1:
            c = np.concatenate([c, c[:1]])  # one point listed twice
        sets.append(torch.from_numpy(c))
    return ClusterSet.from_list(sets)


def dense_from_sparse(ov, K):
    ov_start, ov_other, ov_inter = (t.cpu().numpy() for t in ov[:3])
    m = np.zeros((K, K), dtype=np.int64)
    for k in range(K):
        assert (np.diff(ov_other[ov_start[k]:ov_start[k + 1]]) > 0).all()  # ascending, each once
        m[k, ov_other[ov_start[k]:ov_start[k + 1]]] = ov_inter[ov_start[k]:ov_start[k + 1]]
    return m


def cross_intersections(clusters):
    """the intersection counts behind cross_iou, recovered exactly: iou * (n_i + n_j) / (1 + iou), rounded"""
    iou = pg.cross_iou(clusters).double().cpu().numpy()
    n = clusters.sizes().double().cpu().numpy()
    inter = np.rint(iou * (n[:, None] + n[None, :]) / (1.0 + iou)).astype(np.int64)
    np.fill_diagonal(inter, 0)
    return inter


def tie_case():
    """(column, gt_size, gt_class, clusters, cluster classes) of one cloud with seven instances, worked by hand:
    columns 0..6 hold 2, 4, 2, 1, 5, 5, 1 points; points 8-11 belong to no instance.
      cluster 3  one point in column 0 and one in column 2, both of 2 points: 1 / 4 twice, the first column wins;
      cluster 4  1 / (3 + 1 - 1) with column 3 and 2 / (3 + 5 - 2) with column 4: equal values from different
                 integers, the first wins; cluster 5 meets them in the other order;
      cluster 2  predicts class 2 and touches only columns of class 3: no candidate;  cluster 6 touches no instance."""
    column = np.array([0, 0, 1, 1, 1, 1, 2, 2, -1, -1, -1, -1, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 6])
    gt_size = np.array([2, 4, 2, 1, 5, 5, 1])
    gt_class = np.array([3, 3, 2, 3, 3, 2, 2])
    sets = [[0, 8], [2, 3, 8, 9], [1, 4, 5, 8, 9, 10, 11], [0, 6, 9], [12, 13, 14], [18, 19, 23], [8, 9]]
    return column, gt_size, gt_class, sets, [3, 3, 2, 2, 3, 2, 3]


# inter_all, col_all, inter_cls, col_cls of tie_case()
TIE_CASE_ANSWER = ((1, 2, 2, 1, 1, 2, 0), (0, 1, 1, 0, 3, 5, -1), (1, 2, 0, 1, 1, 2, 0), (0, 1, -1, 2, 3, 5, -1))


def columns(labels, batch):
    """the column layout of torch_points_kernels.instance_iou, on the host: (column (N,), offsets (B,), per_cloud (B,))"""
    gt, b = labels.instance_labels.cpu().numpy(), batch.cpu().numpy()
    nb = labels.num_instances.shape[0]
    per_cloud = np.zeros(nb, dtype=np.int64)
    np.maximum.at(per_cloud, b, gt)
    offsets = np.cumsum(per_cloud) - per_cloud
    return np.where(gt > 0, offsets[b] + gt - 1, -1), offsets, per_cloud


def check_instances(n, valid, order):
    """instances_device against get_instances' stored list"""
    z = fixture()
    valid, order = valid.cpu().numpy(), order.cpu().numpy()
    assert order[valid[order]].tolist() == z["b%d_pick" % n].tolist()


def check_matches(n, best, labels, batch, clusters):
    """the class-restricted best instances (cluster_best_instance's inter_cls, col_cls) against the stored
    find_best_match of every record of batch n: instance id inside the cloud and float64 IoU, exactly"""
    z = fixture()
    rec = z["b%d_records" % n]
    column, offsets, _ = columns(labels, batch)
    inter_cls, col_cls = best[2].cpu().numpy(), best[3].cpu().numpy()
    size = clusters.sizes().cpu().numpy()
    head = clusters.members[clusters.starts[:-1]].cpu().numpy()
    cloud = batch.cpu().numpy()[head]
    gt_size = np.bincount(column[column >= 0])
    for row in rec:
        k = int(row[6])
        assert size[k] == row[3]
        if row[4] == 0:
            assert col_cls[k] == -1 and inter_cls[k] == 0
        else:
            assert col_cls[k] - offsets[cloud[k]] + 1 == row[4]
            assert float(inter_cls[k]) / float(size[k] + gt_size[col_cls[k]] - inter_cls[k]) == row[5]
    return len(rec)


def run_evaluator(thr, device, as_set=True, **kw):
    """tracks the stored batches; checks, batch by batch, the instance lists, the records and the running means"""
    z = fixture()
    ev = PM.PanopticEvaluator(int(z["num_classes"]), stage="val", ignore_label=-1, **kw)
    seen = []
    for n in range(int(z["num_batches"])):
        results, labels, batch = batch_inputs(n, device, as_set)
        ev.track(results, labels, batch, iou_threshold=thr)
        valid, order = PM.instances_device(results, min_cluster_points=10)
        check_instances(n, valid, order)
        acc = z["%s_b%d_acc" % (tag(thr), n)]
        if not np.isnan(acc).any():
            seen.append(acc)
        m = ev.get_metrics()
        want = np.mean(seen, axis=0) if seen else np.zeros(3)
        got = np.array([m["val_pos"], m["val_neg"], m["val_Iacc"]])
        assert np.abs(got - want).max() <= BAR, (n, got, want)
        # the records of the batch: classes and scores of the valid clusters, by descending score as stored
        cls, score, _ = ev.prediction_records()
        rec = z["b%d_records" % n]
        if rec.shape[0]:
            cls, score = cls[-rec.shape[0]:], score[-rec.shape[0]:]
            best_first = np.argsort(-score, kind="stable")
            assert cls[best_first].tolist() == rec[:, 0].astype(np.int64).tolist()
            assert score[best_first].tolist() == rec[:, 1].tolist()
    assert len(seen) == 2  # two batches had valid clusters
    return ev


def check_final(ev, thr):
    """flags per class, rec / ap per class and every metric after finalise"""
    z = fixture()
    t = tag(thr)
    ev.finalise()
    cls, score, flag = ev.prediction_records()
    classes = z[t + "_classes"].tolist()
    assert list(ev._ap.keys()) == classes and list(ev._rec.keys()) == classes
    for c in classes:
        mine = np.flatnonzero(cls == c)
        mine = mine[np.argsort(-score[mine], kind="stable")]
        assert score[mine].tolist() == z["%s_scores_c%d" % (t, c)].tolist()
        assert flag[mine].astype(np.int64).tolist() == z["%s_flags_c%d" % (t, c)].tolist()
    assert np.abs(np.array([ev._ap[c] for c in classes]) - z[t + "_ap"]).max() <= BAR
    assert np.abs(np.array([ev._rec[c] for c in classes]) - z[t + "_rec"]).max() <= BAR
    want = json.loads(str(z[t + "_metrics_json"]))
    got = ev.get_metrics(verbose=True)
    assert sorted(got.keys()) == sorted(want.keys())
    for k, v in want.items():
        if isinstance(v, dict):
            assert sorted(str(a) for a in got[k].keys()) == sorted(v.keys())
            assert max(abs(float(got[k][int(a)]) - b) for a, b in v.items()) <= BAR, k
        elif isinstance(v, str):
            assert got[k] == v, k
        else:
            assert abs(float(got[k]) - v) <= BAR, (k, got[k], v)
