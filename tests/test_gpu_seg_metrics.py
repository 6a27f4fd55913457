"""The segmentation-metric kernels of csrc/seg_metrics.hip on the device (torchpoints.confusion_count / part_iou_counts /
vote_add) and the evaluators of torch_points3d_amd/seg_metrics.py built on them.

References, none of them the code under test: numpy's argmax and bincount, serial Python loops written here, and the
stored results of the reference's own trackers (tests/golden/seg_metrics.npz, through tests/seg_metrics_cases.py).
Every comparison is integer or bit equality: the kernels count, and the one float operation (the vote add) is a single
IEEE addition per element.  Shapes: around the wave (63, 64, 65), around the row tile (tile - 1, tile, tile + 1,
4 tile + 3), more tiles than workgroups, and the class counts on both sides of the LDS route limit."""
import numpy as np
import pytest
import torch

import seg_metrics_cases as sc
from torch_points3d_amd import _lib
from torch_points3d_amd import seg_metrics as SM
from torch_points3d_amd import torchpoints as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256      # tp3d_confusion_tile_rows(), asserted below
LDS_MAX_C = 80  # TP3D_CONFUSION_LDS_MAX_CLASSES, asserted below


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def new_cm(C):
    return torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)


def ref_cm(C, labels, pred, ignore=None):
    """serial statement of the counting rule: (matrix, invalid)"""
    cm, invalid = np.zeros((C, C), dtype=np.int64), 0
    for l, p in zip(labels.tolist(), pred.tolist()):
        if ignore is not None and l == ignore:
            continue
        if p is None:
            continue
        if not (0 <= l < C) or not (0 <= p < C):
            invalid += 1
        else:
            cm[l, p] += 1
    return cm, invalid


def split(cm, C):
    flat = cm.cpu().numpy()
    return flat[:C * C].reshape(C, C), int(flat[C * C])


def random_scores(rng, N, C):
    """few distinct values, all negative: many tied maxima, and a running maximum started at 0 would never move"""
    return -1.0 - rng.randint(0, 6, (N, C)).astype(np.float32) * 0.25


def test_limits_are_the_documented_ones():
    h = _lib.load()
    assert h.tp3d_confusion_tile_rows() == TILE and h.tp3d_confusion_lds_max_classes() == LDS_MAX_C
    assert h.tp3d_part_iou_max_parts() == tp.PART_IOU_MAX_PARTS == SM.PART_IOU_MAX_PARTS >= 8


@pytest.mark.parametrize("C", [1, 2, 13, 20, 50, 64, 65, LDS_MAX_C, LDS_MAX_C + 1])
def test_confusion_sizes_and_widths(C):
    rng = np.random.RandomState(C)
    for N in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE + 3):
        scores = random_scores(rng, N, C)
        labels = rng.randint(-1, C, N).astype(np.int64)
        cm = tp.confusion_count(new_cm(C), T(labels), scores=T(scores), ignore_label=-1)
        got, invalid = split(cm, C)
        pred = scores.argmax(1) if N else np.zeros(0, dtype=np.int64)
        want, _ = ref_cm(C, labels, pred, ignore=-1)
        assert invalid == 0 and np.array_equal(got, want), (C, N)


@pytest.mark.parametrize("C", [13, LDS_MAX_C + 1])
def test_confusion_more_tiles_than_workgroups(C):
    N = 1030 * TILE + 5
    rng = np.random.RandomState(1)
    scores = random_scores(rng, N, C)
    labels = rng.randint(0, C, N).astype(np.int64)
    got, invalid = split(tp.confusion_count(new_cm(C), T(labels), scores=T(scores)), C)
    want = np.bincount(C * labels + scores.argmax(1), minlength=C * C).reshape(C, C)
    assert invalid == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("C", [13, LDS_MAX_C + 1])
def test_confusion_column_slice_of_a_wider_tensor(C):
    rng = np.random.RandomState(2)
    N = 2 * TILE + 9
    wide = T(random_scores(rng, N, C + 7))
    labels = rng.randint(0, C, N).astype(np.int64)
    view = wide[:, 3:3 + C]
    assert not view.is_contiguous()
    got, _ = split(tp.confusion_count(new_cm(C), T(labels), scores=view), C)
    want, _ = ref_cm(C, labels, view.cpu().numpy().argmax(1))
    assert np.array_equal(got, want)


def test_confusion_ties_all_equal_rows_and_negative_scores():
    C = 13
    scores = np.full((6, C), -7.5, dtype=np.float32)
    scores[1, 4] = scores[1, 9] = -2.0            # tie: the lower column
    scores[2, 12] = -0.5                           # the last column
    scores[3, 0] = -1e30                           # all equal but the first: column 1
    scores[4] = -np.arange(C, 0, -1)               # ascending: the last column
    scores[5] = -3.0e38                            # all equal, hugely negative: column 0
    labels = np.arange(6, dtype=np.int64)
    got, _ = split(tp.confusion_count(new_cm(C), T(labels), scores=T(scores)), C)
    want = np.zeros((C, C), dtype=np.int64)
    for l, p in enumerate([0, 4, 12, 1, 12, 0]):
        want[l, p] += 1
    assert np.array_equal(got, want) and np.array_equal(scores.argmax(1), [0, 4, 12, 1, 12, 0])


@pytest.mark.parametrize("C", [13, LDS_MAX_C + 1])
def test_confusion_every_label_ignored_and_out_of_range_labels(C):
    rng = np.random.RandomState(3)
    N = TILE + 40
    scores = T(random_scores(rng, N, C))
    cm = tp.confusion_count(new_cm(C), torch.full((N,), -1, dtype=torch.int64, device=DEV), scores=scores, ignore_label=-1)
    assert int(cm.abs().sum()) == 0
    labels = rng.randint(0, C, N).astype(np.int64)
    labels[[0, 70, N - 1]] = [C, -5, 1 << 40]
    got, invalid = split(tp.confusion_count(cm, T(labels), scores=scores, ignore_label=-1), C)
    want, bad = ref_cm(C, labels, scores.cpu().numpy().argmax(1), ignore=-1)
    assert invalid == bad == 3 and np.array_equal(got, want) and got.sum() == N - 3
    m = SM.ConfusionMatrix(C, DEV)
    m.count_scores(T(labels), scores, ignore_label=-1)
    with pytest.raises(ValueError, match="outside"):
        m.get_confusion_matrix()


@pytest.mark.parametrize("C", [13, LDS_MAX_C + 1])
def test_confusion_three_calls_equal_one_and_a_cell_past_int32(C):
    rng = np.random.RandomState(4)
    parts = [(random_scores(rng, n, C), rng.randint(0, C, n).astype(np.int64)) for n in (300, 1, TILE)]
    cm = new_cm(C)
    for s, l in parts:
        tp.confusion_count(cm, T(l), scores=T(s))
    s_all, l_all = np.concatenate([s for s, _ in parts]), np.concatenate([l for _, l in parts])
    one = tp.confusion_count(new_cm(C), T(l_all), scores=T(s_all))
    assert torch.equal(cm, one)
    want = np.bincount(C * l_all + s_all.argmax(1), minlength=C * C)
    cell = int(want.argmax())
    seeded = new_cm(C)
    seeded[cell] = 2 ** 31 - 1
    tp.confusion_count(seeded, T(l_all), scores=T(s_all))
    assert int(seeded[cell]) == 2 ** 31 - 1 + int(want[cell]) > 2 ** 31
    seeded[cell] -= 2 ** 31 - 1
    assert torch.equal(seeded, one)


@pytest.mark.parametrize("C", [13, LDS_MAX_C + 1])
def test_confusion_row_index_column_range_and_pred_vector(C):
    rng = np.random.RandomState(5)
    n, N = 100, 3 * TILE + 1
    scores = random_scores(rng, n, C)
    rows = rng.randint(-1, n, N).astype(np.int64)  # repeats and -1
    labels = rng.randint(0, C, N).astype(np.int64)
    assert (rows == -1).any()
    got, invalid = split(tp.confusion_count(new_cm(C), T(labels), scores=T(scores), row_index=T(rows)), C)
    pred = [None if r < 0 else int(scores[r].argmax()) for r in rows]
    want, _ = ref_cm(C, labels, np.array(pred, dtype=object))
    assert invalid == 0 and np.array_equal(got, want)
    rows[5] = n  # past the scores: invalid, not read
    got2, invalid = split(tp.confusion_count(new_cm(C), T(labels), scores=T(scores), row_index=T(rows)), C)
    assert invalid == 1 and got2.sum() == got.sum() - (pred[5] is not None)
    lo, hi = 2, C - 3
    labels_n = rng.randint(0, C, n).astype(np.int64)
    got, _ = split(tp.confusion_count(new_cm(C), T(labels_n), scores=T(scores), columns=(lo, hi)), C)
    want, _ = ref_cm(C, labels_n, lo + scores[:, lo:hi].argmax(1))
    assert np.array_equal(got, want) and got[:, :lo].sum() == 0 and got[:, hi:].sum() == 0
    p = rng.randint(0, C, N).astype(np.int64)
    p[7] = C
    got, invalid = split(tp.confusion_count(new_cm(C), T(labels), pred=T(p)), C)
    want, bad = ref_cm(C, labels, p)
    assert invalid == bad == 1 and np.array_equal(got, want)


def test_confusion_bad_shapes():
    cm, labels = new_cm(4), torch.zeros(5, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        tp.confusion_count(cm, labels, scores=torch.zeros(4, 4, device=DEV))
    with pytest.raises(ValueError):
        tp.confusion_count(cm, labels, scores=torch.zeros(5, 4, device=DEV), columns=(2, 5))
    with pytest.raises(ValueError):
        tp.confusion_count(cm, labels)
    with pytest.raises(ValueError):
        tp.confusion_count(torch.zeros(16, dtype=torch.int64, device=DEV), labels, pred=labels)


# ------------------------------------------------------------------------------------------------------ part counts
def ref_part_counts(scores, labels, seg, classes):
    """serial statement of shapenet_part_tracker.py:63-70, 117-127 as counts"""
    seg_to = {l: segs for segs in classes.values() for l in segs}
    B = len(seg) - 1
    counts, cat_lo = np.zeros((B, SM.PART_IOU_MAX_PARTS, 2), dtype=np.int32), np.full(B, -1, dtype=np.int32)
    for b in range(B):
        segl, logits = labels[seg[b]:seg[b + 1]], scores[seg[b]:seg[b + 1]]
        if len(segl) == 0:
            continue
        segs = seg_to[int(segl[0])]
        segp = logits[:, segs].argmax(1) + segs[0]
        cat_lo[b] = segs[0]
        for l in segs:
            counts[b, l - segs[0]] = [np.sum((segl == l) & (segp == l)), np.sum((segl == l) | (segp == l))]
    return counts, cat_lo


def test_part_counts_of_the_fixture_and_edge_clouds():
    g, classes = sc.golden(), sc.seg_classes()
    scores, labels, batch = g["b_scores"], g["b_labels"], g["b_batch"]
    seg = np.concatenate([[0], np.cumsum(np.bincount(batch))])
    _, _, counts = sc.check_fixture_b(DEV)
    want, _ = ref_part_counts(scores, labels, seg, classes)
    assert np.array_equal(counts, want)
    # an empty cloud in the middle, a cloud of four row tiles and three rows, labels outside the category
    rng = np.random.RandomState(6)
    n_long = 4 * TILE + 3
    s2 = random_scores(rng, n_long, 50)
    l2 = rng.randint(30, 36, n_long).astype(np.int64)  # Motorbike
    l2[3::5] = rng.randint(0, 50, len(l2[3::5]))        # any label; the first row keeps the category
    scores2, labels2 = np.concatenate([scores[:64], s2]), np.concatenate([labels[:64], l2])
    seg2 = np.array([0, 1, 1, 64, 64 + n_long], dtype=np.int64)
    ev = SM.ShapenetPartEvaluator(classes)
    ev.track(T(scores2), T(labels2), seg=T(seg2))
    counts2, cat_lo2 = ev.cloud_counts()
    want2, want_lo2 = ref_part_counts(scores2, labels2, seg2, classes)
    assert np.array_equal(counts2, want2) and np.array_equal(cat_lo2, want_lo2) and cat_lo2[1] == -1
    free = s2.argmax(1)
    assert ((free < 30) | (free >= 36)).any()  # the prediction is restricted to the category all the same
    assert counts2[3, :6, 1].sum() >= n_long and counts2[3, 6:].sum() == 0
    ev.get_metrics()


def test_part_counts_refuse_wide_categories_and_flag_unknown_first_labels():
    C = 20
    lo = torch.zeros(C, dtype=torch.int32, device=DEV)
    hi = torch.full((C,), C, dtype=torch.int32, device=DEV)
    scores, labels = torch.zeros(4, C, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    seg = torch.tensor([0, 4], device=DEV)
    with pytest.raises(RuntimeError, match="exceeds"):
        tp.part_iou_counts(scores, labels, seg, lo, hi, C)
    counts, cat_lo = tp.part_iou_counts(scores, labels, seg, lo, hi, 8)  # the tables are wider than claimed: flagged
    assert int(cat_lo[0]) == -2 and int(counts.abs().sum()) == 0
    ev = SM.ShapenetPartEvaluator({"A": [0, 1], "B": [3, 4]})  # label 2 belongs to no category
    ev.track(torch.zeros(3, 5, device=DEV), torch.tensor([2, 0, 0], device=DEV), seg=torch.tensor([0, 3], device=DEV))
    with pytest.raises(ValueError, match="no category"):
        ev.get_metrics()


# ------------------------------------------------------------------------------------------------------ vote_add
def fresh_votes(Tn, C):
    return SM._Votes(Tn, C, torch.device(DEV))


def test_vote_add_unique_ids_is_the_torch_statement():
    rng = np.random.RandomState(7)
    Tn, C = 5000, 13
    votes_cpu, counts_cpu = torch.zeros(Tn, C), torch.zeros(Tn, dtype=torch.int32)
    st = fresh_votes(Tn, C)
    for n in (1, 63, 2 * TILE + 1, 3000):
        ids = torch.from_numpy(rng.permutation(Tn)[:n])
        wide = torch.from_numpy(rng.randn(n, C + 3).astype(np.float32))
        out = wide[:, 1:1 + C]  # rows of a wider tensor
        votes_cpu[ids] += out
        counts_cpu[ids] += 1
        st.add(ids.to(DEV), wide.to(DEV)[:, 1:1 + C])
    assert torch.equal(st.votes.cpu(), votes_cpu) and torch.equal(st.counts.cpu(), counts_cpu)
    st.check()


def test_vote_add_duplicate_rule_against_a_serial_loop():
    rng = np.random.RandomState(8)
    Tn, C, n = 300, 5, 4 * TILE + 7  # every target named several times
    st = fresh_votes(Tn, C)
    votes, counts = np.zeros((Tn, C), dtype=np.float32), np.zeros(Tn, dtype=np.int32)
    for _ in range(3):
        ids, out = rng.randint(0, Tn, n), rng.randn(n, C).astype(np.float32)
        last = {}
        for i, t in enumerate(ids.tolist()):
            last[t] = i  # the highest row index
        for t, i in last.items():
            votes[t] += out[i]
            counts[t] += 1
        st.add(T(ids), T(out))
    assert np.array_equal(st.votes.cpu().numpy(), votes) and np.array_equal(st.counts.cpu().numpy(), counts)


def test_vote_add_stale_workspace_two_dimensional_ids_and_bad_ids():
    C = 3
    pos, y = torch.rand(1000, 3, device=DEV), torch.randint(0, C, (1000,), device=DEV)
    ev = SM.S3DISEvaluator(C, pos, y, stage="test")
    ids1 = torch.arange(1000, 2000, device=DEV) % 1000
    ids1[500] = 7  # id 7 at row 500 of call 1 (and at row 7: a duplicate, row 500 wins)
    out1 = torch.randn(1000, C, device=DEV)
    ev.track(out1, y[ids1], ids1.reshape(4, 250))
    ids2 = torch.tensor([20, 21, 22, 7, 24], device=DEV)  # id 7 at row 3 of call 2: must land although 3 < 500
    out2 = torch.randn(5, C, device=DEV)
    ev.track(out2, y[ids2], ids2)
    assert torch.equal(ev.votes[7], out1[500] + out2[3]) and int(ev.prediction_count[7]) == 2
    assert int(ev.prediction_count[500]) == 0 and int(ev.prediction_count[20]) == 2
    ev.finalise(full_res=True)
    ev.track(out2, y[ids2], torch.tensor([0, 1000, -1, 3, 4], device=DEV))
    assert int(ev.prediction_count[3]) == 2 and int(ev.prediction_count[0]) == 2  # track does not raise
    with pytest.raises(ValueError, match="Origin ids"):
        ev.finalise()


def test_two_voters_share_nothing():
    pos = torch.rand(50, 3, device=DEV)
    y = torch.zeros(50, dtype=torch.int64, device=DEV)
    a, b = SM.SegmentationVoter(pos, y, 4), SM.SegmentationVoter(pos, y, 4)
    ids, out = torch.arange(10, device=DEV), torch.randn(10, 4, device=DEV)
    a.add_vote(ids, out)
    a.add_vote(ids, out)
    b.add_vote(ids + 5, out)
    assert torch.equal(a.votes[:10], out + out) and int(a.votes[10:].abs().sum()) == 0
    assert torch.equal(b.votes[5:15], out) and int(b.vote_counts.sum()) == 10 and a.num_votes == 2 and b.num_votes == 1
    assert a.coverage == 0.2 and b.coverage == 0.2


# ------------------------------------------------------------------------------------------------------ end to end
def test_fixture_a_on_the_device_equals_the_host_path():
    dev, cpu = sc.check_fixture_a(DEV), sc.check_fixture_a("cpu")
    assert all(np.array_equal(d, c) for d, c in zip(dev, cpu))


def test_fixture_b_on_the_device_equals_the_host_path():
    dev, cpu = sc.check_fixture_b(DEV), sc.check_fixture_b("cpu")
    assert all(np.array_equal(d, c) for d, c in zip(dev, cpu))


def test_fixture_c_on_the_device_equals_the_host_path():
    assert np.array_equal(sc.check_fixture_c(DEV), sc.check_fixture_c("cpu"))


def test_fixture_d_on_the_device_equals_the_host_path():
    dev, cpu = sc.check_fixture_d(DEV), sc.check_fixture_d("cpu")
    assert all(np.array_equal(d, c) for d, c in zip(dev, cpu))
