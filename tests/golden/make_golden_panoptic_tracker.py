"""Generator of tests/golden/panoptic_tracker.npz: the REFERENCE's panoptic tracker on the CPU (data only).

Runs the reference's own classes, imported from the reference tree: `PanopticTracker.track / finalise / get_metrics`
with its `InstanceAPMeter` (metrics/panoptic_tracker.py) and `PanopticResults.get_instances`
(models/panoptic/structures.py), behind the stand-ins the other generators use:
  * make_golden.install_stubs, and the stand-ins of make_golden_votenet.py / make_golden_seg_metrics.py that let
    metrics/box_detection/ap.py (voc_ap) and metrics/segmentation_tracker.py import;
  * a small working `AverageValueMeter` for torchnet (`add`, `value()`, `n`; the mean is kept as a running mean);
  * `scatter_add` for torch_scatter (one scatter_add_ on zeros);
  * this project's `torch_points_kernels.instance_iou` (torch_points_kernels/metrics.py, loaded by file path).
The tracker is driven through its public `track(model, data=...)` with a minimal model object that only hands over
the tensors; no line of the tracker is restated.

The case (six classes, 0 and 1 stuff; about 3 000 points): four batches -- three ragged clouds (one of a single point),
two clouds, two clouds with only 9 clusters (no valid cluster: the early return) and one batch with an empty cluster
list.  Clusters are made from the instances by dropping and adding points.  Asserted on what the reference produced:
  * a best IoU of exactly 1/4 (|A| = 2, |B| = 3, one shared point);
  * best IoUs on both sides of 0.25 and 0.5;
  * two clusters of one class on one instance, both at IoU >= 0.25 (the later one a false positive by `visited`);
  * a cluster whose best instance overall has another class than the one it predicts;
  * a cluster without any instance point;
  * a class with ground truth and no prediction; a class predicted and absent from the ground truth;
  * overlapping cluster pairs with cross-IoU of exactly 3/10 (both picked at 0.3 in float32) and of 1/3 (one dropped);
  * all scores distinct.
Stored: the inputs, and per batch get_instances' list, the (tp, fp, acc) of _compute_acc and the meter's records
(class, score, scan id, size); after finalise rec and ap per class and the metrics, at iou_threshold 0.25 and 0.5.

    python tests/golden/make_golden_panoptic_tracker.py
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_seg_metrics as mgs  # noqa: E402
import make_golden_votenet as mgv  # noqa: E402

C = 6
STUFF = (0, 1)
THRESHOLDS = (0.25, 0.5)


class Meter(object):
    """what the tracker asks of torchnet's AverageValueMeter"""

    def __init__(self):
        self.n, self.mean = 0, 0.0

    def add(self, value, n=1):
        self.n += n
        self.mean += (value - self.mean) * n / float(self.n)

    def value(self):
        return self.mean, float("nan")


def scatter_add(src, index, dim=0):
    return torch.zeros(int(index.max()) + 1, dtype=src.dtype).scatter_add_(dim, index, src)


def load_reference():
    mgv.load_reference()
    mgs.load_reference()
    sys.modules["torchnet"].meter.AverageValueMeter = Meter
    sys.modules["torch_scatter"].scatter_add = scatter_add
    spec = importlib.util.spec_from_file_location("_tpk_metrics", os.path.join(mg.ROOT, "torch_points_kernels", "metrics.py"))
    metrics = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metrics)
    sys.modules["torch_points_kernels"].instance_iou = metrics.instance_iou
    from torch_points3d.metrics.panoptic_tracker import PanopticTracker
    from torch_points3d.models.panoptic.structures import PanopticLabels, PanopticResults
    return PanopticTracker, PanopticResults, PanopticLabels


class Model(mgs.Model):
    pass


class Cloud(object):
    """points of one cloud: y, instance ids 1..g (0: none), and the clusters (local indices, class, or None = y[first])"""

    def __init__(self, rng, n, sizes, classes):
        self.n = n
        self.y = rng.integers(0, 2, n)  # stuff
        self.inst = np.zeros(n, dtype=np.int64)
        self.ranges = []
        at = 0
        for g, (s, c) in enumerate(zip(sizes, classes)):
            at += int(rng.integers(3, 12))  # stuff points between the instances
            self.inst[at:at + s] = g + 1
            self.y[at:at + s] = c
            noisy = at + 1 + np.flatnonzero(rng.random(s - 1) < 0.1)  # the first point keeps the instance's class
            self.y[noisy] = rng.integers(0, C, noisy.shape[0])
            self.ranges.append((at, at + s))
            at += s
        assert at < n
        self.stuff = np.flatnonzero(self.inst == 0)
        self.clusters = []

    def add(self, idx, cls=None):
        self.clusters.append((np.asarray(idx, dtype=np.int64), cls))

    def random_cluster(self, rng, g, keep, extra, cls=None):
        a, b = self.ranges[g]
        pts = a + np.sort(rng.permutation(b - a)[:max(1, int(round(keep * (b - a))))])
        more = rng.permutation(self.stuff)[:int(round(extra * (b - a)))]
        self.add(np.concatenate([pts, more]), cls)


def build_batch(rng, clouds):
    """tensors of one batch; the predicted label of a point is its y, but the first member of a cluster predicts the
    class asked for it"""
    y = np.concatenate([c.y for c in clouds])
    inst = np.concatenate([c.inst for c in clouds])
    batch = np.concatenate([np.full(c.n, i, dtype=np.int64) for i, c in enumerate(clouds)])
    pred = y.copy()
    clusters, off, asked = [], 0, {}
    for c in clouds:
        for idx, cls in c.clusters:
            clusters.append(torch.from_numpy(idx + off))
            if cls is not None:
                assert asked.setdefault(int(idx[0] + off), cls) == cls  # no two clusters ask two classes of one point
                pred[idx[0] + off] = cls
        off += c.n
    logits = mgs.quantise(torch.from_numpy(rng.normal(0, 1, (y.shape[0], C)).astype(np.float32)))
    logits[torch.arange(y.shape[0]), torch.from_numpy(pred)] += 8.0
    assert torch.equal(logits.max(1)[1], torch.from_numpy(pred))
    K = len(clusters)
    scores = torch.from_numpy((0.03 + 0.94 * (rng.permutation(K) + rng.random(K) * 0.5) / max(K, 1)).astype(np.float32))
    assert len(set(scores.tolist())) == K
    num_instances = torch.tensor([int(c.inst.max()) for c in clouds])
    return dict(y=torch.from_numpy(y), inst=torch.from_numpy(inst), batch=torch.from_numpy(batch), logits=logits,
                clusters=clusters, scores=scores, num_instances=num_instances)


def make_batches():
    rng = np.random.default_rng(20240607)
    # batch 0: three ragged clouds, the second a single point
    a = Cloud(rng, 760, [3, 60, 40, 50, 30, 45, 38, 26, 64], [2, 2, 3, 2, 3, 5, 2, 3, 2])
    s3 = a.ranges[0]
    a.add([s3[1] - 1, int(a.stuff[-1])], 2)                                  # |A| = 2, |B| = 3, one shared: IoU 1/4
    i1 = a.ranges[1]
    a.add(np.arange(i1[0], i1[0] + 33), 2)                                   # two clusters on one instance ...
    a.add(np.arange(i1[0] + 33, i1[1]), 2)                                   # ... disjoint, so both pass the suppression
    j, k2 = a.ranges[2], a.ranges[3]
    a.add(np.concatenate([np.arange(k2[0], k2[0] + 10), np.arange(j[0], j[0] + 30)]), 2)  # best overall: class 3; asks 2
    a.add(a.stuff[5:25])                                                     # no instance point
    a.random_cluster(rng, 4, 0.9, 0.1, 4)                                    # predicts class 4: absent from the ground truth
    st = a.stuff[30:60]
    a.add(st[0:6]), a.add(st[3:10])                                          # 6 and 7 points, 3 shared: 3 / 10
    a.add(st[12:18]), a.add(st[15:21])                                       # 6 and 6 points, 3 shared: 1 / 3
    for g, keep, extra in ((3, 0.45, 0.3), (5, 0.8, 0.0), (6, 0.3, 0.1), (7, 1.0, 0.2), (8, 0.6, 0.6), (8, 0.2, 0.0)):
        a.random_cluster(rng, g, keep, extra, 2 if g == 5 else None)         # class 5 is never predicted
    one = Cloud(rng, 1, [], [])
    b = Cloud(rng, 520, [35, 48, 22, 57, 41], [3, 2, 2, 3, 5])
    for g, keep, extra in ((0, 0.7, 0.2), (1, 0.35, 0.0), (1, 0.5, 0.5), (2, 1.0, 0.0), (3, 0.15, 0.1), (3, 0.85, 0.15),
                           (4, 0.5, 0.0)):
        b.random_cluster(rng, g, keep, extra, 3 if g == 4 else None)
    batches = [build_batch(rng, [a, one, b])]
    # batch 1: two clouds
    c = Cloud(rng, 640, [44, 31, 52, 28, 36, 47], [2, 3, 3, 2, 5, 3])
    for g, keep, extra in ((0, 0.95, 0.05), (0, 0.3, 0.0), (1, 0.55, 0.4), (2, 0.25, 0.0), (2, 0.75, 0.1), (3, 0.5, 1.0),
                           (5, 0.65, 0.0)):
        c.random_cluster(rng, g, keep, extra)
    c.add(c.stuff[10:40], 3)
    d = Cloud(rng, 480, [39, 53, 25, 33], [3, 2, 3, 2])
    for g, keep, extra in ((0, 0.6, 0.1), (1, 0.9, 0.0), (1, 0.4, 0.3), (2, 0.2, 0.0), (3, 0.8, 0.5), (3, 0.5, 0.0)):
        d.random_cluster(rng, g, keep, extra, 4 if (g, keep) == (2, 0.2) else None)
    batches.append(build_batch(rng, [c, d]))
    # batch 2: 9 clusters -- get_instances' size test compares the number of clusters with min_cluster_points = 10
    e = Cloud(rng, 300, [40, 30, 35], [2, 3, 2])
    f = Cloud(rng, 260, [28, 45], [3, 5])
    for cl, g in ((e, 0), (e, 0), (e, 1), (e, 2), (e, 2), (f, 0), (f, 1), (f, 1), (f, 0)):
        cl.random_cluster(rng, g, float(rng.uniform(0.3, 1.0)), float(rng.uniform(0.0, 0.3)))
    batches.append(build_batch(rng, [e, f]))
    # batch 3: no cluster at all
    batches.append(build_batch(rng, [Cloud(rng, 120, [30, 20], [2, 3])]))
    return batches


def check_conditions(meter, batches, picks):
    preds = [p for v in meter._pred_clusters.values() for p in v]
    gts = {}
    for by_scan in meter._gt_clusters.values():
        for scan, lst in by_scan.items():
            gts.setdefault(scan, []).extend(lst)
    best_all, best_cls = [], []
    for p in preds:
        everything = gts.get(p.scan_id, [])
        mine = [g for g in everything if g.classname == p.classname]
        best_all.append(p.find_best_match(everything) + (everything,))
        best_cls.append(p.find_best_match(mine) + (mine,))
    ious = np.array([b[0] for b in best_cls if b[1] >= 0])
    assert (ious == 0.25).any()
    assert ((ious > 0) & (ious < 0.25)).any() and ((ious > 0.25) & (ious < 0.5)).any() and (ious >= 0.5).any()
    taken, twice = set(), False
    for p, b in zip(preds, best_cls):
        if b[1] >= 0 and b[0] >= 0.25:
            key = (p.scan_id, p.classname, b[1])
            twice |= key in taken
            taken.add(key)
    assert twice
    assert any(a[1] >= 0 and c[1] >= 0 and a[2][a[1]].classname != p.classname and a[2][a[1]] is not c[2][c[1]]
               for p, a, c in zip(preds, best_all, best_cls))
    assert any(a[0] == 0 for a in best_all)
    gt_classes, pred_classes = set(meter._gt_clusters.keys()), set(meter._pred_clusters.keys())
    assert gt_classes - pred_classes and pred_classes - gt_classes
    cl = batches[0]["clusters"]
    sets = [set(c.tolist()) for c in cl]
    exact, above = False, False
    for i in range(len(cl)):
        for j in range(i + 1, len(cl)):
            inter = np.float32(len(sets[i] & sets[j]))
            if inter == 0:
                continue
            iou = inter / (np.float32(len(sets[i])) + np.float32(len(sets[j])) - inter)
            if iou == np.float32(3) / np.float32(10) and len(sets[i] & sets[j]) == 3:
                exact |= i in picks[0] and j in picks[0]
            if iou == np.float32(3) / np.float32(9):
                above |= (i in picks[0]) != (j in picks[0])
    assert exact and above


def main():
    PanopticTracker, PanopticResults, PanopticLabels = load_reference()
    batches = make_batches()
    out = {"num_classes": np.int64(C), "num_batches": np.int64(len(batches)), "thresholds": np.array(THRESHOLDS)}
    for thr in THRESHOLDS:
        tag = "t%02d" % int(round(100 * thr))
        tracker = PanopticTracker(mgs.Dataset(C), stage="val", ignore_label=-1)
        picks = []
        for n, bt in enumerate(batches):
            N = bt["y"].shape[0]
            results = PanopticResults(semantic_logits=bt["logits"], offset_logits=torch.zeros(N, 3), cluster_scores=bt["scores"],
                                      clusters=bt["clusters"], cluster_type=torch.zeros(len(bt["clusters"]), dtype=torch.uint8))
            labels = PanopticLabels(center_label=torch.zeros(N, 3), y=bt["y"], num_instances=bt["num_instances"],
                                    instance_labels=bt["inst"], instance_mask=bt["inst"] > 0, vote_label=torch.zeros(N, 3))
            data = mgs.Area(pos=torch.zeros(N, 3), batch=bt["batch"])
            before = sum(len(v) for v in tracker._ap_meter._pred_clusters.values())
            order_before = {k: len(v) for k, v in tracker._ap_meter._pred_clusters.items()}
            scan_before = tracker._scan_id_offset
            tracker.track(Model(results, labels), data=data, iou_threshold=thr)
            pick = [int(i) for i in results.get_instances(min_cluster_points=10)]
            picks.append(pick)
            valid = [bt["clusters"][i] for i in pick]
            acc = (PanopticTracker._compute_acc(valid, bt["logits"].max(1)[1], labels, bt["batch"], bt["num_instances"], thr)
                   if valid else (np.nan, np.nan, np.nan))
            new = [p for k, v in tracker._ap_meter._pred_clusters.items() for p in v[order_before.get(k, 0):]]
            assert len(new) == len(valid) and sum(len(v) for v in tracker._ap_meter._pred_clusters.values()) == before + len(new)
            if thr == THRESHOLDS[0]:
                out["b%d_logits" % n], out["b%d_y" % n] = bt["logits"].numpy(), bt["y"].numpy()
                out["b%d_inst" % n], out["b%d_batch" % n] = bt["inst"].numpy(), bt["batch"].numpy()
                out["b%d_num_instances" % n], out["b%d_scores" % n] = bt["num_instances"].numpy(), bt["scores"].numpy()
                out["b%d_members" % n] = (torch.cat(bt["clusters"]).numpy() if bt["clusters"] else np.zeros(0, dtype=np.int64))
                out["b%d_sizes" % n] = np.array([c.numel() for c in bt["clusters"]], dtype=np.int64)
                out["b%d_pick" % n] = np.array(pick, dtype=np.int64)
                # the meter's records of this batch, sorted by descending score: (class, score, scan id, size, the instance
                # id inside its cloud of find_best_match over the ground truth of its class and scan, that IoU, the
                # cluster, found by its members); id 0 where there is no candidate or the best IoU is 0
                by_members = {tuple(bt["clusters"][i].tolist()): i for i in pick}
                assert len(by_members) == len(pick)
                new.sort(key=lambda p: -p.score)
                rows, cluster_of = [], {}
                for p in new:
                    first = int(torch.nonzero(bt["batch"] == p.scan_id - scan_before)[0])
                    cluster_of[id(p)] = by_members[tuple((p.indices + first).tolist())]
                    gts = tracker._ap_meter._gt_clusters.get(p.classname, {}).get(p.scan_id, [])
                    iou, best = p.find_best_match(gts) if gts else (0.0, -1)
                    start = int(torch.nonzero(bt["batch"] == p.scan_id - scan_before)[0])
                    match = int(bt["inst"][start + int(gts[best].indices[0])]) if best >= 0 and iou > 0 else 0
                    rows.append([p.classname, p.score, p.scan_id, len(p.indices), match, iou if match else 0.0, cluster_of[id(p)]])
                out["b%d_records" % n] = np.array(rows, dtype=np.float64).reshape(-1, 7)
            out["%s_b%d_acc" % (tag, n)] = np.array(acc, dtype=np.float64)
        if thr == THRESHOLDS[0]:
            check_conditions(tracker._ap_meter, batches, picks)
            assert picks[2] == [] and picks[3] == [] and len(batches[2]["clusters"]) == 9 and not batches[3]["clusters"]
        meter = tracker._ap_meter
        for c in sorted(meter._gt_clusters.keys()):  # the true-positive flags, read off the recall curve of _eval_cls
            rec, _, _ = meter._eval_cls(c, thr)
            ngt = sum(len(g) for g in meter._gt_clusters[c].values())
            hits = np.round(np.asarray(rec) * ngt)
            out["%s_flags_c%d" % (tag, c)] = np.diff(np.concatenate([[0.0], hits])).astype(np.int64)
            out["%s_scores_c%d" % (tag, c)] = np.array([p.score for p in meter._pred_clusters.get(c, [])], dtype=np.float64)
            out["%s_ngt_c%d" % (tag, c)] = np.int64(ngt)
        tracker.finalise()
        m = tracker.get_metrics(verbose=True)
        classes = sorted(tracker._ap.keys())
        out[tag + "_classes"] = np.array(classes, dtype=np.int64)
        out[tag + "_ap"] = np.array([tracker._ap[c] for c in classes], dtype=np.float64)
        out[tag + "_rec"] = np.array([tracker._rec[c] for c in classes], dtype=np.float64)
        plain = {k: ({str(a): float(b) for a, b in v.items()} if isinstance(v, dict) else (v if isinstance(v, str) else float(v)))
                 for k, v in m.items()}
        out[tag + "_metrics_json"] = np.array(json.dumps(plain, sort_keys=True))
        print(tag, {k: v for k, v in plain.items() if not isinstance(v, dict)})
    path = os.path.join(HERE, "panoptic_tracker.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
