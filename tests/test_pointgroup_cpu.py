"""PointGroup's CSR side on CPU tensors (torch_points3d_amd/pointgroup.py, torchpoints.ClusterSet): everything around the
HIP region growing is index arithmetic that runs anywhere; the region growing itself has no CPU form and must say so."""
import numpy as np
import pytest
import torch

import pointgroup_util as pgu
import torch_points_kernels as tpk
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd import torchpoints as tp


def random_clusters(seed, n_points=300, k=25):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(k):
        size = int(torch.randint(1, 40, (1,), generator=g))
        out.append(torch.sort(torch.randperm(n_points, generator=g)[:size])[0])
    return out


def test_cluster_set_round_trip():
    clusters = random_clusters(0)
    cs = tp.ClusterSet.from_list(clusters)
    assert len(cs) == len(clusters)
    back = cs.to_list()
    assert all(torch.equal(a, b) for a, b in zip(back, clusters))
    assert all(b.data_ptr() == cs.members.data_ptr() + 8 * int(cs.starts[i]) for i, b in enumerate(back))  # views
    assert torch.equal(cs.member_cluster, torch.repeat_interleave(torch.arange(len(clusters)), cs.sizes()))
    assert int(cs.starts[0]) == 0 and int(cs.starts[-1]) == cs.members.numel()
    empty = tp.ClusterSet.from_list([])
    assert len(empty) == 0 and empty.to_list() == [] and empty.members.numel() == 0
    both = tp.ClusterSet.cat([cs, cs])
    assert all(torch.equal(a, b) for a, b in zip(both.to_list(), clusters + clusters))
    assert torch.equal(both.member_cluster[cs.members.numel():], cs.member_cluster + len(cs))


def test_cluster_set_labels_from_first_member():
    labels = torch.tensor([5, 5, 7, 7, 7])
    batch = torch.tensor([0, 0, 0, 1, 1])
    cs = tp.ClusterSet.from_list([torch.tensor([0, 1]), torch.tensor([3, 4])], labels=labels, batch=batch)
    assert cs.label.tolist() == [5, 7] and cs.cloud.tolist() == [0, 1]


def test_offset_loss_known_answers():  # test/test_pointgroup.py:13-25
    pred = torch.tensor([[2, 0, 0], [0, 1, 0]]).float()
    losses = pg.offset_loss(pred, torch.tensor([[2, 0, 0], [0, 1, 0]]).float(), 2)
    assert losses["offset_norm_loss"].item() == 0
    assert losses["offset_dir_loss"].item() == pytest.approx(-1, abs=1e-5)
    losses = pg.offset_loss(pred, torch.tensor([[2, 0, 0], [0, -1, 0]]).float(), 2)
    assert losses["offset_norm_loss"].item() == pytest.approx(1.0, abs=1e-5)
    assert losses["offset_dir_loss"].item() == pytest.approx(0.0, abs=1e-5)


@pytest.mark.parametrize("as_set", [False, True])
def test_score_loss_known_answers(as_set):  # test/test_pointgroup.py:27-39
    clusters = [torch.tensor([0, 1, 2]), torch.tensor([3, 4])]
    if as_set:
        clusters = tp.ClusterSet.from_list(clusters)
    scores = torch.tensor([1, 0]).float()
    batch = torch.tensor([0, 0, 0, 0, 0])
    assert pg.instance_iou_loss(clusters, scores, torch.tensor([1, 1, 1, 0, 0]), batch).item() == 0
    assert pg.instance_iou_loss(clusters, scores, torch.tensor([1, 1, 1, 2, 2]), batch).item() == pytest.approx(50)


def test_instance_iou_csr_equals_list_form():
    clusters = random_clusters(1)
    g = torch.Generator().manual_seed(2)
    batch = torch.sort(torch.randint(0, 3, (300,), generator=g))[0]
    inst = torch.randint(0, 6, (300,), generator=g)
    cs = tp.ClusterSet.from_list(clusters)
    want = tpk.instance_iou(cs.to_list(), inst, batch)
    got = pg.instance_iou_csr(cs, inst, batch)
    assert got.shape == want.shape and torch.equal(got, want)
    assert pg.instance_iou_csr(tp.ClusterSet.from_list([]), inst, batch).shape == (0, want.shape[1])


def test_cross_iou_equals_dense_masks():
    clusters = random_clusters(3)
    cs = tp.ClusterSet.from_list(clusters)
    want = pgu.reference_cross_ious(clusters, 300)
    torch.testing.assert_close(pg.cross_iou(cs), want, rtol=0, atol=0)  # counts below 2^24 and one division each: exact


@pytest.mark.parametrize("k,min_cluster_points", [(25, 100), (25, 10), (120, 100)])
def test_get_instances_equals_reference(k, min_cluster_points):
    # structures.py:46-47 compares the number of clusters with min_cluster_points: 25 > 100 picks nothing, 120 > 100 does
    clusters = random_clusters(4, k=k)
    scores = torch.rand(k, generator=torch.Generator().manual_seed(5))
    want = pgu.reference_get_instances(clusters, scores, 300, min_cluster_points=min_cluster_points)
    for form in (clusters, tp.ClusterSet.from_list(clusters)):
        res = pg.PanopticResults(semantic_logits=torch.zeros(300, 4), offset_logits=torch.zeros(300, 3), cluster_scores=scores,
                                 clusters=form, cluster_type=torch.zeros(k, dtype=torch.uint8))
        got = res.get_instances(min_cluster_points=min_cluster_points)
        assert [int(i) for i in got] == [int(i) for i in want]
    assert (len(want) > 0) == (k > min_cluster_points)
    none = pg.PanopticResults(torch.zeros(3, 4), torch.zeros(3, 3), None, None, None)
    assert none.get_instances() == []


def test_region_grow_csr_refuses_cpu_tensors():
    s = pgu.scene()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.region_grow_csr(s["pos"], s["labels"], s["batch"], ignore_labels=pgu.IGNORE, radius=pgu.RADIUS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pg.region_grow(s["pos"], s["labels"], s["batch"])


def test_unserved_scorers_say_why():
    for scorer in ("encoder", "unet"):
        with pytest.raises(NotImplementedError, match="2\\^9 clouds"):
            pg.PointGroup(3, 5, scorer_type=scorer, backbone=torch.nn.Identity())


def test_scene_generator_keeps_its_promises():
    s = pgu.scene()  # asserts the 2 % margin and the neighbour count itself
    pos, labels, batch = s["pos"], s["labels"], s["batch"]
    assert pos.dtype == torch.float32 and bool((batch[1:] >= batch[:-1]).all()) and batch.unique().tolist() == [0, 1]
    assert sorted(labels.unique().tolist()) == [0, 1, 2, 3]
    ref = pgu.scene_reference()
    sizes = sorted(len(c) for c in ref)
    assert sizes[0] == pgu.MIN_CLUSTER_SIZE and sizes[-1] == pgu.SNAKE_ROW * pgu.SNAKE_ROWS + pgu.SNAKE_ROWS
    assert sizes.count(2910) == 2                      # the snake of either cloud: equal coordinates, never merged
    assert sizes.count(16) >= 2 and sizes.count(12) >= 4 and sizes.count(27) >= 4  # edge, corner and face contacts
    assert all(labels[c[0]] != 0 for c in ref)
    assert all(len(set(batch[c].tolist())) == 1 and len(set(labels[c].tolist())) == 1 for c in ref)
    # the host walk and the float64 connected components agree on this scene, order included
    assert ref == pgu.components_reference(pos, labels, batch, pgu.IGNORE, pgu.RADIUS, pgu.MIN_CLUSTER_SIZE)
    # (label ascending, lowest member ascending) is the list order
    keys = [(int(labels[c[0]]), c[0]) for c in ref]
    assert keys == sorted(keys)


# ---- the edge generators of test_gpu_region_grow_edges.py, held to their own guarantees without a GPU -----------------
# Every generator asserts its margins (and, where it has them, its intended cells) when called; here the host walk, the
# float64 components and the literal expectation are shown to agree, so that a failure on the GPU points at the kernel.
def _host(s, **kw):
    from test_gpu_region_grow import host
    return host(s, **kw)


def _components(s, ignore=pgu.IGNORE, radius=pgu.RADIUS, min_cluster_size=pgu.MIN_CLUSTER_SIZE):
    return pgu.components_reference(s["pos"], s["labels"], s["batch"], list(ignore), radius, min_cluster_size)


@pytest.mark.parametrize("which", sorted(pgu.SHIFTS))
def test_edges_shifted_scenes_keep_the_clusters(which):
    s, base = pgu.scene_shifted(which), pgu.scene()
    assert torch.equal(s["labels"], base["labels"]) and torch.equal(s["batch"], base["batch"])
    shift = torch.tensor(pgu.SHIFTS[which], dtype=torch.float64) * pgu.H
    assert float((s["pos"].double() - base["pos"].double() - shift).abs().max()) <= pgu.H / 64 + 1e-12  # at most the jitter
    assert _host(s) == pgu.scene_reference() == _components(s)


def test_edges_far_point_is_beyond_the_coordinate_limit():
    s = pgu.scene_with_far_point(1e6)
    assert int(pgu.cells_fp32(s["pos"][-1:].numpy(), pgu.RADIUS)[0, 0]) > 1 << 24
    assert _host(s) == pgu.scene_reference() == _components(s)  # the far single is dropped


@pytest.mark.parametrize("swap", [False, True])
def test_edges_twenty_six_pairs(swap):
    s = pgu.pairs26(swap)  # asserts the cells of every pair
    want = [[2 * i, 2 * i + 1] for i in range(26)]
    assert s["want"] == want == _host(s, min_cluster_size=2) == _components(s, min_cluster_size=2)
    low_end_first = s["pos"][0::2, 0] < s["pos"][1::2, 0]  # pairs across +x: which end is the lower index
    dx = torch.tensor([d[0] for d in pgu.DIRS26 + pgu.DIRS26])
    assert bool((low_end_first[dx == 1] != swap).all()) and bool((low_end_first[dx == -1] == swap).all())


@pytest.mark.parametrize("extra", [None, "label4095", "label-1", "cloud1024", "ignored"])
def test_edges_key_field_pairs(extra):
    s = pgu.pairs26_fields(extra)
    assert bool((s["batch"][1:] >= s["batch"][:-1]).all())
    assert sorted(s["batch"].unique().tolist())[:3] == list(pgu.FIELD_CLOUDS)
    kw = dict(ignore_labels=s["ignore"], min_cluster_size=2)
    assert s["want"] == _host(s, **kw) == _components(s, s["ignore"], min_cluster_size=2)
    if extra is not None:  # the extra points are there, and are singles: min_cluster_size 1 shows them
        assert len(_host(s, ignore_labels=(), min_cluster_size=1)) == 26 + 52 + (2 if extra == "ignored" else 1)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("k", [pgu.CELL_MAX, pgu.CELL_MAX + 1])
def test_edges_span_limit(axis, k):
    s = pgu.span_limit(axis, k)  # asserts the intended cells
    assert pgu.CELL_MAX == (1 << 14) - 3 and int(s["cells"][:, axis].max() - s["cells"][:, axis].min()) == k
    assert s["want"] == _host(s, min_cluster_size=3) == _components(s, min_cluster_size=3)


@pytest.mark.parametrize("count", [63, 64, 65, 128, 129])
def test_edges_piles(count):
    from test_gpu_region_grow import pile
    s = pile(count)
    pgu.check_margins(s["pos"], s["batch"], pgu.RADIUS, 300)
    want = [list(range(1, count + 1))]
    assert want == _host(s, nsample=300) == _components(s)
    s = pgu.pile3(count)
    assert s["want"] == [list(range(1, 3 * count + 1))] == _components(s)
    if 3 * count <= 300:
        pgu.check_margins(s["pos"], s["batch"], pgu.RADIUS, 300)
        assert s["want"] == _host(s, nsample=300)


def test_edges_strict_pairs():
    s = pgu.strict_pairs()  # asserts d2 == r2 and d2 < r2 in fp32
    assert s["want"] == [[0], [1], [2, 3]] == _host(s, radius=pgu.STRICT_RADIUS, min_cluster_size=1)
    # (no float64 components here: cKDTree's ball is closed and joins the pair on the radius)


@pytest.mark.parametrize("runs", [1, 1023, 1024, 1025, 2049])
def test_edges_line_of_singles(runs):
    s = pgu.line_of_singles(runs)
    assert s["want"] == [[i] for i in range(runs)] == _host(s, min_cluster_size=1) == _components(s, min_cluster_size=1)
    assert int(pgu.cells_fp32(s["pos"].numpy(), pgu.RADIUS)[:, 0].max()) == 3 * (runs - 1) <= pgu.CELL_MAX


@pytest.mark.parametrize("ignored", [0, 100])
def test_edges_alternating_runs(ignored):
    s = pgu.alternating_runs(2049, ignored)
    assert int((s["labels"] == 0).sum()) == ignored and s["pos"].shape[0] == 1025 * 2 + 1024 + ignored
    assert len(s["want"]) == 1025 and s["want"] == _host(s, min_cluster_size=2) == _components(s, min_cluster_size=2)
    # at min_cluster_size 1 the runs alternate pair, single, pair, ... in list order
    sizes = [len(c) for c in _components(s, min_cluster_size=1)]
    assert sizes == [2, 1] * 1024 + [2]


@pytest.mark.parametrize("order", ["ascending", "descending", "bitrev"])
def test_edges_snake_chain(order):
    s = pgu.snake_chain(order)
    n = pgu.SNAKE_ROW * pgu.SNAKE_ROWS + pgu.SNAKE_ROWS
    assert s["want"] == [list(range(n))] == _host(s) == _components(s)
    idx = s["index"]
    step = np.abs(np.diff(idx))
    if order == "bitrev":  # neighbours on the path are far apart in index, every second step by about half the range
        assert sorted(idx.tolist()) == list(range(n)) and np.median(step) > n // 4
    else:
        assert np.all(step == 1) and idx[0] == (0 if order == "ascending" else n - 1)
    d = np.linalg.norm(np.diff(s["pos"].numpy()[idx].astype(np.float64), axis=0), axis=1)
    assert d.max() < pgu.RADIUS  # consecutive positions on the path are linked: a chain


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_edges_scene_permutations(seed):
    s, base = pgu.scene_permuted(seed), pgu.scene()
    assert not np.array_equal(s["perm"], np.arange(len(s["perm"]))) and torch.equal(s["pos"], base["pos"][s["perm"]])
    assert pgu.map_back(_host(s), s) == pgu.scene_reference()
