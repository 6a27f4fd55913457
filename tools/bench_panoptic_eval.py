"""Panoptic evaluation of PointGroup: the device operators (torchpoints.cluster_overlaps / cluster_nms /
cluster_best_instance, csrc/panoptic_metrics.hip) and one PanopticEvaluator.track call, on the two scenes of
tools/bench_region_grow.py: the clusters of the lattice scene (81) and the same points with a random label per voxel
(61 768 clusters on 345 948 points).  Ground truth: the 81 boxes as instances, their labels as classes.

Against, on the 81-cluster scene only:
  (i)  the composition this repository had before, on device tensors: PanopticResults.get_instances (dense cross_iou,
       suppression in numpy) plus pointgroup.instance_iou_csr(...).max(1) -- wall clock + synchronise;
  (ii) the reference tracker's loops restated in numpy (_compute_acc's masks, _pred / _gt_instances_per_scan,
       np.intersect1d per pair in _eval_cls) -- wall clock.
Neither is run on the 61 768-cluster scene: (i) needs a (K, K) float matrix of 15 GB there, (ii) K x G set
intersections in Python.  A third operator timing takes two partitions of the many-cluster scene together (every point
in two clusters), so that the overlaps are not empty and the walk has work.
Device timings: HIP events, median of --runs (30).  Needs a GPU (no fallback).

    python tools/bench_panoptic_eval.py [--out profiles/panoptic_eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_region_grow import H, STUFF, scene  # noqa: E402
from bench_sparseconv import timed  # noqa: E402


def wall(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def reference_loops(clusters, scores, predicted, inst, y, batch, thr):
    """what PanopticTracker does per batch after get_instances, on host arrays (metrics/panoptic_tracker.py:191-269,
    49-79): masks over the batch per cluster, torch.where per instance, np.intersect1d per (prediction, instance) pair"""
    nb = int(batch.max()) + 1
    gts = {}
    for b in range(nb):
        mask = batch == b
        local, yl = inst[mask], y[mask]
        for i in range(int(local.max())):
            idx = np.where(local == i + 1)[0]
            gts.setdefault((int(yl[idx[0]]), b), []).append(idx)
    start = np.concatenate([[0], np.cumsum(np.bincount(batch))])
    tp = 0
    for k in np.argsort(-scores):
        cl = clusters[k]
        b = int(batch[cl[0]])
        mine = gts.get((int(predicted[cl[0]]), b), [])
        best, at = -np.inf, -1
        for j, g in enumerate(mine):
            inter = float(len(np.intersect1d(g, cl - start[b])))
            iou = inter / float(len(g) + len(cl) - inter)
            if iou > best:
                best, at = iou, j
        sample = batch == b
        classes, counts = np.unique(y[sample][inst[sample] == inst[cl[0]]], return_counts=True)
        tp += int(best >= thr and classes[counts.argmax()] == predicted[cl[0]])
    return tp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_panoptic_eval needs a GPU: nothing is measured without one")
    from torch_points3d_amd import panoptic_metrics as PM
    from torch_points3d_amd import pointgroup as pg
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    pos, labels, batch = [t.to(dev) for t in scene(args.clouds, args.points)]
    N = pos.shape[0]
    ignore = torch.tensor([-1, STUFF], device=dev)
    grow = dict(ignore_labels=ignore, radius=1.5 * H, nsample=300)
    boxes = tp.region_grow_csr(pos, labels, batch, min_cluster_size=10, **grow)
    kept = ~torch.isin(labels, ignore)
    g = torch.Generator().manual_seed(1)
    noisy = [torch.where(kept, torch.randint(1, 9, labels.shape, generator=g).to(dev), labels) for _ in range(2)]
    tiny = [tp.region_grow_csr(pos, lab, batch, min_cluster_size=1, **grow) for lab in noisy]

    # ground truth: the boxes, numbered per cloud
    cloud = boxes.cloud.cpu().numpy()
    ids = np.zeros(len(boxes), dtype=np.int64)
    for b in range(args.clouds):
        ids[cloud == b] = 1 + np.arange(int((cloud == b).sum()))
    inst = torch.zeros(N, dtype=torch.int64, device=dev)
    inst[boxes.members] = torch.from_numpy(ids).to(dev)[boxes.member_cluster]
    num_instances = torch.from_numpy(np.bincount(cloud, minlength=args.clouds)).to(dev)
    logits = torch.nn.functional.one_hot(labels, 9).float()
    zeros = torch.zeros(N, 3, device=dev)
    gt = pg.PanopticLabels(center_label=zeros, y=labels, num_instances=num_instances, instance_labels=inst,
                           instance_mask=inst > 0, vote_label=zeros)

    def results_for(cs):
        gen = torch.Generator().manual_seed(2)
        scores = (torch.randperm(len(cs), generator=gen).float() + 0.5) / len(cs)
        return pg.PanopticResults(semantic_logits=logits, offset_logits=zeros, cluster_scores=scores.to(dev), clusters=cs,
                                  cluster_type=torch.zeros(len(cs), dtype=torch.uint8, device=dev))

    def operators(cs, name):
        res = results_for(cs)
        M = cs.members.numel()
        ov = tp.cluster_overlaps(cs, capacity=M, num_points=N, return_stats=True)
        pairs, entries, overflow = ov[3].tolist()
        assert not overflow
        ev = PM.PanopticEvaluator(9, stage="val")
        offsets = torch.cumsum(num_instances, 0) - num_instances
        column = torch.where(inst > 0, offsets[batch] + inst - 1, torch.full_like(inst, -1))
        K, G = len(cs), len(boxes)
        gt_size = torch.zeros(G + 1, dtype=torch.int64, device=dev).scatter_add_(
            0, torch.where(column >= 0, column, torch.full_like(column, G)), torch.ones_like(column))[:G]
        args_best = (cs, column, gt_size, boxes.label, cs.label, offsets[cs.cloud], offsets[cs.cloud] + num_instances[cs.cloud])
        ms = {"cluster_overlaps": timed(lambda: tp.cluster_overlaps(cs, capacity=M, num_points=N), args.runs),
              "cluster_nms": timed(lambda: tp.cluster_nms(cs, res.cluster_scores, 0.3, overlaps=ov), args.runs),
              "cluster_best_instance": timed(lambda: tp.cluster_best_instance(*args_best), args.runs),
              "evaluator_track": timed(lambda: ev.track(res, gt, batch), args.runs)}
        ev.finalise()
        return {"scene": name, "clusters": K, "member_slots": M, "ordered_pairs": pairs, "overlap_entries": entries, "ms": ms}

    rows = [operators(boxes, "lattice boxes"), operators(tiny[0], "random label per voxel"),
            operators(tp.ClusterSet.cat(tiny), "two partitions of the random-label scene")]

    # (i) and (ii), 81-cluster scene only
    res = results_for(boxes)

    def composition():
        picked = res.get_instances(min_cluster_points=10)
        best = pg.instance_iou_csr(boxes, inst, batch).max(1)
        return picked, best

    composition_ms = wall(composition, args.host_runs)
    host = [c.cpu().numpy() for c in boxes.to_list()]
    host_args = (host, res.cluster_scores.cpu().numpy(), labels.cpu().numpy(), inst.cpu().numpy(), labels.cpu().numpy(),
                 batch.cpu().numpy(), 0.25)
    t0 = time.perf_counter()
    reference_loops(*host_args)
    loops_ms = round(1e3 * (time.perf_counter() - t0), 3)
    result = {"workload": "panoptic_eval", "points": int(N), "clouds": args.clouds, "instances": int(len(boxes)),
              "timer": {"device": "hip events, median of %d" % args.runs,
                        "composition": "wall clock + synchronise, median of %d" % args.host_runs,
                        "reference_loops": "wall clock, one run, host arrays already copied"},
              "scenes": rows,
              "lattice_boxes_baselines_ms": {"get_instances_plus_instance_iou_csr_max": composition_ms,
                                             "reference_tracker_loops_numpy": loops_ms},
              "not_run": {"composition on %d clusters" % len(tiny[0]):
                          "the (K, K) float32 matrix of cross_iou alone is %.1f GB" % (4e-9 * len(tiny[0]) ** 2),
                          "reference loops on %d clusters" % len(tiny[0]): "K x G np.intersect1d calls in Python"},
              "not_timed": ["finalise / get_metrics (host, three numbers per predicted instance)",
                            "cluster_overlaps with capacity=None (adds two device-to-host reads)"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
