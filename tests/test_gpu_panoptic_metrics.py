"""The panoptic-evaluation kernels of csrc/panoptic_metrics.hip on the device (torchpoints.cluster_best_instance /
cluster_overlaps / cluster_nms / instance_ap_match) and the PanopticEvaluator built on them.

References, none of them the code under test: this repository's dense yardsticks pointgroup.instance_iou_csr, cross_iou
and non_max_suppression, the numpy restatements of torch_points3d_amd/panoptic_metrics.py (pinned on the CPU by
tests/test_panoptic_metrics_cpu.py), and the stored results of the reference's own tracker
(tests/golden/panoptic_tracker.npz through tests/panoptic_cases.py).  Every operator comparison is integer or bit
equality.  Shapes: around the wave and the one-wave / workgroup seam of the histogram kernel (63, 64, 65, 256, 257,
1025 members), both sides of its column window, slot runs across the 256-slot workgroups of the pair kernels, and
neighbour lists around the wave and the workgroup of the walk."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc
from torch_points3d_amd import _lib
from torch_points3d_amd import panoptic_metrics as PM
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd import torchpoints as tp
from torch_points3d_amd.torchpoints import ClusterSet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = tp.CLUSTER_BEST_WINDOW


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_dev(clusters):
    return ClusterSet(clusters.members.to(DEV), clusters.starts.to(DEV), clusters.member_cluster.to(DEV))


def same(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def test_window_is_the_documented_one():
    assert _lib.load().tp3d_cluster_best_window() == W == PM.CLUSTER_BEST_WINDOW


# ---------------------------------------------------------------------------------------------------- (a) best instance
def best_both(clusters, column, gt_size, gt_class, cluster_class, lo, hi):
    got = tp.cluster_best_instance(to_dev(clusters), T(column), T(gt_size), T(gt_class), T(cluster_class), T(lo), T(hi))
    again = tp.cluster_best_instance(to_dev(clusters), T(column), T(gt_size), T(gt_class), T(cluster_class), T(lo), T(hi))
    assert same(got, again)  # bit-equal repeats
    want = PM.cluster_best_instance_numpy(clusters, column, gt_size, gt_class, cluster_class, lo, hi)
    assert same(got, want)
    return got


def against_dense(clusters, got, inst, batch):
    dense = pg.instance_iou_csr(to_dev(clusters), T(inst), T(batch))
    values, indices = dense.max(1)
    positive = values > 0
    assert torch.equal(got[1][positive], indices[positive]) and bool((got[1][~positive] == -1).all())
    column, _, _ = pc.columns(type("L", (), {"instance_labels": torch.from_numpy(inst), "num_instances": torch.zeros(int(batch.max()) + 1)}),
                              torch.from_numpy(batch))
    gt_size = T(np.bincount(column[column >= 0], minlength=dense.shape[1])).float()
    fi, size = got[0].float(), to_dev(clusters).sizes().float()
    iou = fi / ((size + gt_size[got[1].clamp(min=0)]) - fi).clamp(min=1.0)
    assert torch.equal(iou[positive], values[positive])
    return int(positive.sum())


def scene(rng, clouds, n, g):
    """`clouds` clouds of n points with g instances each (ids 1..g, about a third of the points in none)"""
    inst = np.concatenate([np.where(rng.random(n) < 0.35, 0, rng.integers(1, g + 1, n)) for _ in range(clouds)])
    for c in range(clouds):
        inst[c * n:c * n + g] = np.arange(1, g + 1)  # every id is present
    batch = np.repeat(np.arange(clouds), n)
    y = rng.integers(0, 5, clouds * n)
    return inst, batch, y


def tables(inst, batch, y):
    labels = type("L", (), {"instance_labels": torch.from_numpy(inst), "num_instances": torch.zeros(int(batch.max()) + 1)})
    column, offsets, per_cloud = pc.columns(labels, torch.from_numpy(batch))
    G = int(per_cloud.sum())
    gt_size = np.bincount(column[column >= 0], minlength=G)
    first = np.full(G, 0)
    first[column[column >= 0][::-1]] = np.flatnonzero(column >= 0)[::-1]  # the lowest point of every column
    return column, offsets, per_cloud, gt_size, y[first]


def test_best_instance_cluster_sizes_around_the_wave_and_the_workgroup():
    rng = np.random.default_rng(0)
    n = 3000
    inst, batch, y = scene(rng, 2, n, 23)
    column, offsets, per_cloud, gt_size, gt_class = tables(inst, batch, y)
    sets, cloud = [], []
    for c in range(2):
        for size in (1, 63, 64, 65, 256, 257, 1025):
            sets.append(torch.from_numpy(c * n + np.sort(rng.choice(n, size, replace=False))))
            start = int(rng.integers(0, n - size))
            sets.append(torch.from_numpy(c * n + start + np.arange(size)))
            cloud += [c, c]
    clusters = ClusterSet.from_list(sets)
    cloud = np.array(cloud)
    cluster_class = rng.integers(0, 5, len(sets))
    got = best_both(clusters, column, gt_size, gt_class, cluster_class, offsets[cloud], offsets[cloud] + per_cloud[cloud])
    assert against_dense(clusters, got, inst, batch) >= len(sets) - 4
    assert int((got[3] >= 0).sum()) > 4 and int((got[3] != got[1]).sum()) > 0


@pytest.mark.parametrize("G", [1, W, W + 1])
def test_best_instance_on_both_sides_of_the_column_window(G):
    extra = 40
    inst = np.concatenate([np.arange(1, G + 1), np.zeros(extra, dtype=np.int64)])  # instance g + 1 is point g alone
    batch = np.zeros(G + extra, dtype=np.int64)
    y = np.arange(G + extra) % 3
    column, offsets, per_cloud, gt_size, gt_class = tables(inst, batch, y)
    stuff = list(range(G, G + 5))
    last, nxt = min(W, G) - 1, min(W, G - 1)  # the last column of the first window, the first of the second
    sets = [[last] + stuff, [nxt] + stuff, sorted({last, nxt}) + stuff, stuff, sorted({0, last, nxt}) + stuff[:2]]
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    K = len(sets)
    cluster_class = np.array([y[last], y[nxt], y[nxt], 0, y[nxt]])
    got = best_both(clusters, column, gt_size, gt_class, cluster_class, np.zeros(K, dtype=np.int64), np.full(K, G))
    assert got[1].tolist() == [last, nxt, last, -1, 0]
    assert against_dense(clusters, got, inst, batch) == 4


def test_best_instance_first_maximum_and_no_candidate():
    column, gt_size, gt_class, sets, classes = pc.tie_case()
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    K = len(sets)
    got = best_both(clusters, column, gt_size, gt_class, np.array(classes), np.zeros(K, dtype=np.int64), np.full(K, 7))
    assert [t.tolist() for t in got] == [list(v) for v in pc.TIE_CASE_ANSWER]


# ---------------------------------------------------------------------------------------------------- (b) overlaps
@pytest.mark.parametrize("seed,N,K,lo,hi,dup,windows", [
    (0, 60, 12, 1, 12, False, False),     # points in 1, 2 and 3 clusters
    (1, 200, 40, 1, 30, True, False),     # a point listed twice by a cluster counts once
    (2, 30, 1, 5, 5, False, False),       # K = 1
    (3, 5000, 30, 1, 3, False, False),    # no overlap at all: P = 0
    (4, 400, 90, 5, 40, False, True),     # ~2000 slots: point runs across the 256-slot workgroups of the pair kernels
])
def test_overlaps_against_cross_iou(seed, N, K, lo, hi, dup, windows):
    rng = np.random.default_rng(seed)
    clusters = pc.random_clusters(rng, N, K, lo, hi, dup, windows)
    dev = to_dev(clusters)
    ov = tp.cluster_overlaps(dev)
    assert same(ov, tp.cluster_overlaps(dev)) and same(ov, PM.cluster_overlaps_numpy(clusters))
    plain = ClusterSet.from_list([torch.unique(c) for c in clusters.to_list()]) if dup else clusters
    want = pc.cross_intersections(to_dev(plain))
    assert np.array_equal(pc.dense_from_sparse(ov, K), want)
    P = int((want > 0).sum())
    assert int(ov[0][-1]) == ov[1].numel() == P
    if seed == 3:
        assert P == 0
    if seed == 4:
        per_point = np.bincount(clusters.members.numpy(), minlength=N)
        assert clusters.members.numel() > 1024 and per_point.max() >= 3
        by_point = np.sort(clusters.members.numpy())  # the slots as the pair kernels see them: 256 per workgroup
        assert any(by_point[s - 1] == by_point[s] for s in range(256, by_point.shape[0], 256))
    # with a capacity nothing is read back: the same entries in front, statistics on the device
    Q = int(want.sum())  # ordered pairs over all points
    start, other, inter, stats = tp.cluster_overlaps(dev, capacity=Q + 7, num_points=N, return_stats=True)
    assert torch.equal(start, ov[0]) and torch.equal(other[:P], ov[1]) and torch.equal(inter[:P], ov[2])
    assert stats.tolist() == [Q, P, 0] and other.numel() == Q + 7
    start, other, inter, stats = tp.cluster_overlaps(dev, capacity=Q, return_stats=True)  # exactly enough
    assert torch.equal(start, ov[0]) and torch.equal(other[:P], ov[1]) and stats.tolist() == [Q, P, 0]
    if Q:  # too small: flagged, no entry listed
        start, other, inter, stats = tp.cluster_overlaps(dev, capacity=Q - 1, return_stats=True)
        assert stats.tolist()[0] == Q and stats.tolist()[2] == 1 and int(start.abs().sum()) == 0


def test_overlaps_refuse_more_pairs_than_they_index():
    clusters = to_dev(ClusterSet.from_list([torch.tensor([0, 1]), torch.tensor([1, 2])]))
    with pytest.raises(ValueError, match="2\\^31"):
        tp.cluster_overlaps(clusters, capacity=1 << 31)


# ---------------------------------------------------------------------------------------------------- (c) suppression
def nms_against_dense(clusters, scores, threshold):
    dev = to_dev(clusters)
    keep, order = tp.cluster_nms(dev, T(scores), threshold)
    pairs = int(pc.cross_intersections(dev).sum())
    keep2, order2 = tp.cluster_nms(dev, T(scores), threshold, capacity=pairs + 3)
    assert same((keep, order), (keep2, order2))  # bit-equal repeats, with and without the reads
    assert same((keep, order), PM.cluster_nms_numpy(clusters, torch.from_numpy(scores), threshold))
    want = pg.non_max_suppression(pg.cross_iou(dev).cpu().numpy(), scores, threshold)
    keep, order = keep.cpu(), order.cpu()
    assert order[keep[order]].tolist() == [int(i) for i in want]
    return keep


@pytest.mark.parametrize("seed,K,threshold", [(0, 50, 0.3), (1, 50, 0.1), (2, 700, 0.3), (3, 700, 0.05)])
def test_nms_against_the_dense_suppression(seed, K, threshold):
    rng = np.random.default_rng(20 + seed)
    clusters = pc.random_clusters(rng, 3 * K, K, 2, 25, windows=True)
    scores = (rng.permutation(K).astype(np.float32) + 0.5) / K
    keep = nms_against_dense(clusters, scores, threshold)
    assert 0 < int(keep.sum()) < K


def test_nms_exact_three_tenths_and_chain():
    st = list(range(100))
    sets = [st[0:6], st[3:10], st[20:26], st[23:29], st[40:50], st[44:54], st[48:58]]
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    keep = nms_against_dense(clusters, np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float32), 0.3)
    assert keep.tolist() == [True, True, True, False, True, False, True]


@pytest.mark.parametrize("L", [63, 64, 65, 300])
def test_nms_neighbour_lists_around_the_wave_and_the_workgroup(L):
    # a hub of L points, every point shared with one small cluster; the hub has the best score and clears the small
    # clusters whose IoU 1 / (L + n - 1) exceeds the threshold: those of 1 and 2 points, not those of 3
    rng = np.random.default_rng(L)
    sets = [list(range(L))] + [[i] + list(range(1000 + 3 * i, 1000 + 3 * i + i % 3)) for i in range(L)]
    clusters = ClusterSet.from_list([torch.tensor(s) for s in sets])
    scores = np.concatenate([[2.0], rng.permutation(L) / L]).astype(np.float32)
    threshold = float(np.float32(1.0) / np.float32(L + 1.5))
    keep = nms_against_dense(clusters, scores, threshold)
    assert keep.tolist() == [True] + [i % 3 == 2 for i in range(L)]


def test_nms_equal_scores_follow_the_defined_rule():
    rng = np.random.default_rng(5)
    K = 300
    clusters = pc.random_clusters(rng, 600, K, 2, 20, windows=True)
    scores = rng.integers(0, 4, K).astype(np.float32) / 4
    dev = to_dev(clusters)
    keep, order = tp.cluster_nms(dev, T(scores), 0.2)
    visiting = sorted(range(K), key=lambda i: (-float(scores[i]), -i))
    assert order.tolist() == visiting
    iou = pg.cross_iou(dev).cpu().numpy()
    alive, picked = np.ones(K, dtype=bool), []
    for i in visiting:
        if alive[i]:
            picked.append(i)
            alive &= ~(iou[i] > np.float32(0.2))
    assert order[keep[order]].tolist() == picked and 0 < len(picked) < K


# ---------------------------------------------------------------------------------------------------- the evaluator
@pytest.mark.parametrize("thr", [0.25, 0.5])
def test_evaluator_against_the_reference_tracker(thr):
    ev = pc.run_evaluator(thr, DEV)
    pc.check_final(ev, thr)
    again = pc.run_evaluator(thr, DEV, pair_capacity=4096)
    assert all(np.array_equal(a, b) for a, b in zip(ev.prediction_records(), again.prediction_records()))
    assert torch.equal(ev._sums, again._sums) and torch.equal(ev._ngt, again._ngt)


def test_best_instance_against_the_reference_matches():
    checked = 0
    for n in range(3):
        results, labels, batch = pc.batch_inputs(n, DEV)
        clusters = results.clusters
        column, offsets, per_cloud = pc.columns(labels, batch)
        G = int(per_cloud.sum())
        gt_size = np.bincount(column[column >= 0], minlength=G)
        first = np.full(G, 0)
        first[column[column >= 0][::-1]] = np.flatnonzero(column >= 0)[::-1]
        head = clusters.members[clusters.starts[:-1]].cpu().numpy()
        cloud = batch.cpu().numpy()[head]
        cluster_class = results.semantic_logits.argmax(1).cpu().numpy()[head]
        best = tp.cluster_best_instance(clusters, T(column), T(gt_size), T(labels.y.cpu().numpy()[first]), T(cluster_class),
                                        T(offsets[cloud]), T(offsets[cloud] + per_cloud[cloud]))
        checked += pc.check_matches(n, best, labels, batch, clusters)
    assert checked > 20


def test_small_pair_capacity_is_reported_at_the_end():
    ev = PM.PanopticEvaluator(6, stage="val", pair_capacity=2)
    ev.track(*pc.batch_inputs(0, DEV))
    with pytest.raises(ValueError, match="pair_capacity"):
        ev.finalise()


def test_track_reads_nothing_back():
    ev = PM.PanopticEvaluator(6, stage="val")
    inputs = [pc.batch_inputs(n, DEV) for n in range(4)]
    ev.track(*inputs[0])  # warm-up: library load, workspaces
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enforced = False
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            enforced = True
        if enforced:
            for args in inputs:
                ev.track(*args)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not enforced:
        pytest.skip("this ROCm build of torch does not enforce set_sync_debug_mode('error'): a deliberate .item() did not raise")
    ev.finalise()
    assert ev.get_metrics()["val_pos"] > 0


def test_forty_thousand_clusters_need_no_dense_matrix():
    # K = 40 000 clusters of 1 to 3 neighbouring points: the (K, K) float matrix would take 6.4 GB
    rng = np.random.default_rng(7)
    K, N = 40000, 60000
    size = rng.integers(1, 4, K)
    starts = np.concatenate([[0], np.cumsum(size)])
    members = np.repeat(rng.integers(0, N - 3, K), size) + (np.arange(starts[-1]) - np.repeat(starts[:-1], size))
    clusters = ClusterSet(T(members), T(starts))
    scores = T(rng.permutation(K).astype(np.float32))
    inst = np.arange(N) // 4 + 1  # 15 000 instances of four points in one cloud
    column, gt_size = T(inst - 1), T(np.full(N // 4, 4))
    gt_class, cluster_class = T(np.arange(N // 4) % 3), T(rng.integers(0, 3, K))
    lo, hi = T(np.zeros(K, dtype=np.int64)), T(np.full(K, N // 4))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ov = tp.cluster_overlaps(clusters, num_points=N)
    keep, order = tp.cluster_nms(clusters, scores, 0.3, overlaps=ov)
    best = tp.cluster_best_instance(clusters, column, gt_size, gt_class, cluster_class, lo, hi)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 64 << 20, peak
    assert 0 < int(keep.sum()) < K and ov[1].numel() > K // 4 and int((best[1] >= 0).sum()) == K
    cpu = ClusterSet(clusters.members.cpu(), clusters.starts.cpu(), clusters.member_cluster.cpu())
    assert same(ov, PM.cluster_overlaps_numpy(cpu))
    assert same((keep, order), PM.cluster_nms_numpy(cpu, scores.cpu(), 0.3, overlaps=[t.cpu() for t in ov]))
