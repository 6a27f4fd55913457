"""Region growing on the device (csrc/region_grow.hip, torchpoints.region_grow_csr) and PointGroup on top of it
(torch_points3d_amd/pointgroup.py).

Clusters are index sets, so every comparison is exact.  The references: torch_points_kernels.region_grow on CPU copies
(the host ball query and the host walk) wherever the reference's cap decides the result, float64 connected components
(scipy) for the uncapped form, and the reference's formulas restated in pointgroup_util.py for what follows the
clustering.  The scene (pointgroup_util.scene) keeps every pair 2 % away from the radius."""
import types

import numpy as np
import pytest
import torch

import pointgroup_util as pgu
import torch_points_kernels as tpk
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd import sparseconv as sc
from torch_points3d_amd import torchpoints as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def grow(s, **kw):
    args = dict(ignore_labels=pgu.IGNORE, radius=pgu.RADIUS, nsample=pgu.NSAMPLE, min_cluster_size=pgu.MIN_CLUSTER_SIZE)
    args.update(kw)
    return tp.region_grow_csr(s["pos"].to(DEV), s["labels"].to(DEV), s["batch"].to(DEV), **args)


def host(s, **kw):
    args = dict(ignore_labels=pgu.IGNORE, radius=pgu.RADIUS, nsample=pgu.NSAMPLE, min_cluster_size=pgu.MIN_CLUSTER_SIZE)
    args.update(kw)
    return pgu.as_sorted_lists(tpk.region_grow(s["pos"], s["labels"], s["batch"], **args))


def check_csr(cs, s, want):
    """to_list() equals `want` as lists (order included, members ascending) and the CSR is consistent with it"""
    got = [c.tolist() for c in cs.to_list()]
    assert got == want
    sizes = torch.tensor([len(c) for c in want], dtype=torch.int64)
    starts = torch.zeros(len(want) + 1, dtype=torch.int64)
    starts[1:] = torch.cumsum(sizes, 0)
    assert cs.starts.dtype == torch.int64 and torch.equal(cs.starts.cpu(), starts)
    assert torch.equal(cs.member_cluster.cpu(), torch.repeat_interleave(torch.arange(len(want)), sizes))
    first = torch.tensor([c[0] for c in want], dtype=torch.int64)
    assert torch.equal(cs.label.cpu(), s["labels"][first]) and torch.equal(cs.cloud.cpu(), s["batch"][first])
    assert len(cs) == len(want)


def test_scene_equals_host_path_and_is_deterministic():
    s = pgu.scene()
    a = grow(s)
    assert a.route == "device"
    check_csr(a, s, pgu.scene_reference())
    b = grow(s)
    for name in ("members", "starts", "member_cluster", "label", "cloud"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # the reference's list form through the same call
    lists = pg.region_grow(s["pos"].to(DEV), s["labels"].to(DEV), s["batch"].to(DEV), ignore_labels=pgu.IGNORE,
                           radius=pgu.RADIUS, nsample=pgu.NSAMPLE, min_cluster_size=pgu.MIN_CLUSTER_SIZE)
    assert [c.tolist() for c in lists] == pgu.scene_reference()
    assert all(c.data_ptr() == lists[0].data_ptr() + 8 * int(a.starts[i]) for i, c in enumerate(lists))  # views


def pile(count):
    """`count` identical points between two far-away singles"""
    pos = torch.tensor([[0.5, 0.5, 0.5]]).repeat(count + 2, 1)
    pos[0] = torch.tensor([0.0, 0.0, 0.0])
    pos[-1] = torch.tensor([1.0, 1.0, 1.0])
    n = count + 2
    return dict(pos=pos, labels=torch.ones(n, dtype=torch.int64), batch=torch.zeros(n, dtype=torch.int64))


def test_cap_edge():
    full = pile(pgu.NSAMPLE)  # exactly nsample neighbours, the point itself included: the table holds them all
    a = grow(full)
    assert a.route == "device"
    want = host(full)
    assert want == [list(range(1, pgu.NSAMPLE + 1))]
    check_csr(a, full, want)
    over = pile(pgu.NSAMPLE + 1)  # one more: the reference's table is truncated and its walk decides
    b = grow(over)
    assert b.route == "host"
    check_csr(b, over, host(over))
    c = grow(over, cap=None)  # uncapped components: all nsample + 1
    assert c.route == "device"
    check_csr(c, over, [list(range(1, pgu.NSAMPLE + 2))])


def dense_blobs():
    """blobs with up to 40 points per voxel on the jittered lattice: neighbour counts far above nsample"""
    rng = np.random.RandomState(7)
    pos, labels, batch = [], [], []
    for cloud in range(2):
        for blob in range(6):
            lo = rng.randint(0, 40, size=3) + np.asarray([0, 0, 50 * blob])  # blobs apart along z
            vox = pgu._box(lo, rng.randint(1, 5, size=3))
            vox = np.repeat(vox, rng.randint(1, 41, size=len(vox)), axis=0)
            pos.append(vox * pgu.H + rng.uniform(-pgu.H / 64, pgu.H / 64, size=vox.shape))
            labels.append(np.full(len(vox), 1 + blob % 3))
            batch.append(np.full(len(vox), cloud))
    pos = np.concatenate(pos).astype(np.float32)
    labels, batch = np.concatenate(labels), np.concatenate(batch)
    order = np.lexsort((rng.permutation(len(pos)), batch))  # shuffled inside each cloud
    return dict(pos=torch.from_numpy(pos[order]), labels=torch.from_numpy(labels[order]).long(),
                batch=torch.from_numpy(batch[order]).long())


def test_uncapped_components_on_dense_blobs():
    s = dense_blobs()
    a = grow(s, cap=None)
    assert a.route == "device"
    want = pgu.components_reference(s["pos"], s["labels"], s["batch"], pgu.IGNORE, pgu.RADIUS, pgu.MIN_CLUSTER_SIZE)
    assert len(want) >= 6 and max(len(c) for c in want) > 10 * pgu.NSAMPLE
    check_csr(a, s, want)
    assert grow(s).route == "host"  # the same input under the reference's cap: a neighbourhood overflows


def test_degenerate_inputs():
    s = pgu.scene()
    empty = dict(pos=torch.zeros(0, 3), labels=torch.zeros(0, dtype=torch.int64), batch=torch.zeros(0, dtype=torch.int64))
    a = grow(empty)
    assert len(a) == 0 and a.to_list() == [] and a.starts.tolist() == [0] and a.members.numel() == 0
    ignored = dict(s, labels=torch.zeros_like(s["labels"]))
    a = grow(ignored)
    assert len(a) == 0 and a.route == "device" and a.starts.tolist() == [0] and a.members.numel() == 0
    one = dict(pos=torch.rand(1, 3), labels=torch.ones(1, dtype=torch.int64), batch=torch.zeros(1, dtype=torch.int64))
    assert len(grow(one)) == 0
    a = grow(one, min_cluster_size=1)
    assert a.route == "device" and [c.tolist() for c in a.to_list()] == [[0]]
    keep = s["batch"] == 1  # one cloud, and its id is not 0
    single = dict(pos=s["pos"][keep], labels=s["labels"][keep], batch=s["batch"][keep])
    a = grow(single)
    assert a.route == "device"
    check_csr(a, single, host(single))
    with pytest.raises(ValueError):  # a label the key does not hold is refused under cap=None, never wrapped
        grow(dict(one, labels=torch.full((1,), 5000, dtype=torch.int64)), cap=None)
    wide = dict(s, labels=torch.where(s["labels"] == 3, torch.full_like(s["labels"], 5000), s["labels"]))
    a = grow(wide)  # ... and served by the host path under the reference's cap
    assert a.route == "host"
    check_csr(a, wide, host(wide))


def test_cluster_iou_and_instances_against_the_reference_formulas():
    s = pgu.scene()
    pos, labels, batch = s["pos"], s["labels"], s["batch"]
    shift = torch.tensor([0.25, -0.125, 0.5])  # a translation: the votes keep the scene's margins
    votes = (pos.to(DEV) + shift.to(DEV)).cpu()
    stuff = torch.tensor([pg.IGNORE_LABEL, 0])
    cs, cluster_type = pg.cluster(pos.to(DEV), votes.to(DEV), labels.to(DEV), batch.to(DEV), stuff.to(DEV), pgu.RADIUS)
    on_pos = tpk.region_grow(pos, labels, batch, ignore_labels=stuff, radius=pgu.RADIUS)
    on_votes = tpk.region_grow(votes, labels, batch, ignore_labels=stuff, radius=pgu.RADIUS, nsample=200)
    want = pgu.as_sorted_lists(on_pos + on_votes)
    assert cs.route == "device" and len(on_pos) > 50
    check_csr(cs, s, want)
    assert cluster_type.dtype == torch.uint8 and cluster_type.tolist() == [0] * len(on_pos) + [1] * len(on_votes)

    # instance labels 1..g per cloud: every second reference cluster is an instance, with a few members taken away
    inst = torch.zeros_like(labels)
    count = [0, 0]
    for k, c in enumerate(on_pos[::2]):
        b = int(batch[c[0]])
        count[b] += 1
        inst[torch.sort(c)[0][: max(1, (3 * len(c)) // 4)]] = count[b]
    want_iou = tpk.instance_iou([torch.tensor(c) for c in want], inst, batch)
    got_iou = pg.instance_iou_csr(cs, inst.to(DEV), batch.to(DEV))
    assert got_iou.shape == want_iou.shape and torch.equal(got_iou.cpu(), want_iou)
    assert float(want_iou.max()) > 0.7

    scores = torch.rand(len(cs), generator=torch.Generator().manual_seed(3))
    res = pg.PanopticResults(semantic_logits=torch.zeros(pos.shape[0], 4, device=DEV), offset_logits=None,
                             cluster_scores=scores.to(DEV), clusters=cs, cluster_type=cluster_type)
    torch.testing.assert_close(pg.cross_iou(cs).cpu(), pgu.reference_cross_ious([torch.tensor(c) for c in want], pos.shape[0]),
                               rtol=0, atol=0)
    want_pick = pgu.reference_get_instances([torch.tensor(c) for c in want], scores, pos.shape[0])
    assert len(want) > 100 and 0 < len(want_pick) < len(want)
    assert [int(i) for i in res.get_instances()] == [int(i) for i in want_pick]


def two_level_unet(input_nc, f=16):
    down = dict(N=[0, 1, 1], down_conv_nn=[[input_nc, f], [f, f], [f, 2 * f]], kernel_size=[3, 3, 3], stride=[1, 2, 2],
                block="ResBlock")
    up = dict(N=[1, 1, 0], block="ResBlock", kernel_size=[3, 3, 3], stride=[2, 2, 1],
              up_conv_nn=[[2 * f, f], [f + f, f], [f + f, f]])
    return sc.SparseConv3dUnet(dict(down_conv=down, up_conv=up), input_nc)


@pytest.mark.parametrize("scorer_type", ["MLP", None])
def test_pointgroup_forward_loss_backward(scorer_type):
    rng = np.random.RandomState(11)
    coords, batch = [], []
    for cloud in range(2):  # two blocks of 13 x 13 x 12 voxels, 2 028 points each
        coords.append(pgu._box((0, 0, 0), (13, 13, 12)))
        batch.append(np.full(len(coords[-1]), cloud))
    coords, batch = np.concatenate(coords), np.concatenate(batch)
    pos = (coords * pgu.H + rng.uniform(-pgu.H / 64, pgu.H / 64, size=coords.shape)).astype(np.float32)
    n = len(pos)
    data = types.SimpleNamespace(x=torch.from_numpy(rng.randn(n, 4).astype(np.float32)).to(DEV),
                                 coords=torch.from_numpy(coords).int().to(DEV), batch=torch.from_numpy(batch).long().to(DEV),
                                 pos=torch.from_numpy(pos).to(DEV))
    inst = torch.from_numpy((coords[:, 0] // 5 + 3 * (coords[:, 1] // 5)).astype(np.int64))  # 8 instances per cloud, 0 = none
    labels = pg.PanopticLabels(center_label=None, y=torch.from_numpy(rng.randint(-1, 5, size=n)).long().to(DEV),
                               num_instances=None, instance_labels=inst.to(DEV), instance_mask=(inst > 0).to(DEV),
                               vote_label=torch.from_numpy(rng.randn(n, 3).astype(np.float32)).to(DEV))
    torch.manual_seed(0)
    net = pg.PointGroup(4, 5, stuff_classes=[0], backbone=two_level_unet(4), scorer_type=scorer_type,
                        cluster_radius_search=pgu.RADIUS).to(DEV).train()
    assert net(data, epoch=5).clusters is None  # prepare_epoch: no clustering before epoch 120
    out = net(data)
    assert isinstance(out, pg.PanopticResults) and len(out.clusters) > 0
    assert out.cluster_scores.shape == (len(out.clusters),) and out.cluster_type.shape == (len(out.clusters),)

    # the clusters are torch_points_kernels.region_grow of the predicted labels, on the positions and on the votes
    pred = torch.max(out.semantic_logits, 1)[1].cpu()
    votes = (data.pos + out.offset_logits.detach()).cpu()
    stuff = torch.tensor([pg.IGNORE_LABEL, 0])
    bat = torch.from_numpy(batch).long()
    on_pos = tpk.region_grow(torch.from_numpy(pos), pred, bat, ignore_labels=stuff, radius=pgu.RADIUS)
    on_votes = tpk.region_grow(votes, pred, bat, ignore_labels=stuff, radius=pgu.RADIUS, nsample=200)
    assert [c.tolist() for c in out.clusters.to_list()] == pgu.as_sorted_lists(on_pos + on_votes)
    assert out.cluster_type.tolist() == [0] * len(on_pos) + [1] * len(on_votes)

    if scorer_type is None:  # the mean semantic row per cluster, then its maximum
        logits = out.semantic_logits.detach().cpu().double()
        want = torch.stack([logits[c.cpu()].mean(0).max() for c in out.clusters.to_list()])
        torch.testing.assert_close(out.cluster_scores.cpu().double(), want, rtol=1e-5, atol=1e-6)
        assert not out.cluster_scores.requires_grad

    losses = net.compute_loss(labels)
    assert set(losses) == set(pg.PointGroup.loss_names)
    for name, value in losses.items():
        if name == "score_loss" and scorer_type is None:
            assert value is None
            continue
        assert torch.isfinite(value).all(), name
    losses["loss"].backward()
    off_path = ("ScorerMLP", "ScorerHead") if scorer_type is None else ()
    for name, p in net.named_parameters():
        if name.startswith(off_path) and off_path:
            assert p.grad is None, name
        else:  # the reference's criterion (test/utils.py:4-31): no parameter with an all-zero gradient
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) > 0, name
