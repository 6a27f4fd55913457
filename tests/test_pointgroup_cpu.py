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
