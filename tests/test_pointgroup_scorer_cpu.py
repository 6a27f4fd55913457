"""PointGroup's sparse scorers without a GPU: the safety conditions of the reference-generated fixtures
(tests/golden/pointgroup_scorer_*.npz, README_pointgroup.md) on the committed data, the restatement of
tests/pointgroup_scorer_ref.py against them, pointgroup_config against the resolved YAML, state_dict names and shapes
against the reference's classes, and the host-side validation of SparseTensor(clouds=K)."""
import pytest
import torch

import pointgroup_scorer_ref as psr
import sparseconv_ref as sr
from torch_points3d_amd import pointgroup as pg
from torch_points3d_amd import sparseconv as sc

NON_BACKBONE_KEYS = (
    ["ScorerMLP.%d.%s" % (i, k) for i in (0, 1) for k in ("0.weight", "0.bias", "1.batch_norm.weight", "1.batch_norm.bias",
                                                            "1.batch_norm.running_mean", "1.batch_norm.running_var",
                                                            "1.batch_norm.num_batches_tracked")]
    + ["ScorerHead.0.weight", "ScorerHead.0.bias"]
    + [h + k for h in ("Offset.", "Semantic.")
       for k in ("0.0.0.weight", "0.0.1.batch_norm.weight", "0.0.1.batch_norm.bias", "0.0.1.batch_norm.running_mean",
                 "0.0.1.batch_norm.running_var", "0.0.1.batch_norm.num_batches_tracked", "1.weight", "1.bias")])


class _Backbone(torch.nn.Module):
    output_nc = 8


def _run_restatement(kind, g, dtype):
    numbers = psr.fixture_numbers()["fixture"]
    net = psr.FixtureScorer(kind, numbers[kind]).to(dtype).train()
    net.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in psr.fixture_state(g).items()}, strict=True)
    x = g["x"].to(dtype).clone().requires_grad_(True)
    rows, kinks = {}, []
    scores = net(psr.fixture_clusters(g), x, g["pos"], numbers["size"], rows, kinks)
    (scores * g["cot"].to(dtype)).sum().backward()
    return scores.detach(), x.grad, rows, kinks, net


@pytest.mark.parametrize("kind", psr.KINDS)
def test_fixture_safety_conditions_and_restatement(kind):
    g = psr.load_fixture(kind)
    numbers = psr.fixture_numbers()["fixture"]
    sizes = (g["starts"][1:] - g["starts"][:-1]).tolist()
    assert sizes == numbers["sizes"] and len(sizes) == 12 and min(sizes) >= 20 and max(sizes) <= 60
    assert g["x"].shape[1] == numbers["in_feat"] == 8
    counts = torch.bincount(g["members"])
    assert int((counts == 2).sum()) > 0  # points in two clusters
    # every pos / size stays away from a half-integer: fp32 and float64 agree on every voxel
    q = g["pos"].double() / numbers["size"]
    assert float((q - torch.floor(q) - 0.5).abs().min()) >= psr.HALF_MARGIN
    for dtype in (torch.float32, torch.float64):
        scores, grad_x, rows, kinks, net = _run_restatement(kind, g, dtype)
        assert min(kinks) >= psr.KINK_MARGIN, "an activation input lies %.3g from 0" % min(kinks)
        r, owner = rows["rows"].detach(), rows["rows_batch"]
        for c in range(len(sizes)):
            mine = r[owner == c]
            assert len(mine) >= 1
            if len(mine) > 1:
                top = torch.topk(mine, 2, dim=0).values
                assert float((top[0] - top[1]).min()) >= psr.MAX_MARGIN, "a maximum of cluster %d wins by less" % c
        C = rows["voxel_coords"]
        assert torch.equal(C[:, :3], g["voxel_coords"].long()) and torch.equal(C[:, 3], g["voxel_batch"].long())
        assert len(C) < len(g["members"])  # some voxel holds several points
        assert len(sr.down_coords(C.int(), 4)) >= psr.COARSE_ROWS
        # the restatement is the reference: its float64 pass against the fixture's
        if dtype == torch.float64:
            torch.testing.assert_close(scores, torch.from_numpy(g["f64/scores"]), rtol=1e-9, atol=1e-11)
            torch.testing.assert_close(grad_x, torch.from_numpy(g["f64/grad_x"]), rtol=1e-7, atol=1e-11)
            torch.testing.assert_close(rows["voxel_x"].detach(), torch.from_numpy(g["f64/voxel_x"]), rtol=1e-12, atol=1e-14)
            for k, v in net.state_dict().items():
                if "running_" in k:
                    torch.testing.assert_close(v, torch.from_numpy(g["f64/after/" + k]), rtol=1e-9, atol=1e-12)
        else:
            torch.testing.assert_close(scores, g["scores"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["PointGroup", "PointGroup-PAPER"])
def test_config_equals_the_resolved_yaml(name):
    recorded = psr.fixture_numbers()
    entry, feat = recorded["entries"][name], recorded["feat"]
    cfg = pg.pointgroup_config(name, feat)

    def numbers(d):
        return {k: v for k, v in d.items() if k not in ("class", "conv_type")}

    assert cfg["scorer_unet"] == numbers(entry["scorer_unet"]) and cfg["scorer_encoder"] == numbers(entry["scorer_encoder"])
    for k in ("scorer_type", "prepare_epoch", "min_iou_threshold", "max_iou_threshold", "loss_weights"):
        assert cfg[k] == entry[k], k
    if name == "PointGroup":
        assert cfg["backbone"] is None and entry["backbone"] == {"architecture": "unet"}
        assert cfg["scorer_unet"]["down_conv"]["down_conv_nn"] == [[96, 192], [192, 384]] and cfg["scorer_unet"]["down_conv"]["N"] == 1
        assert cfg["scorer_encoder"]["innermost"]["nn"] == [384, 96] and cfg["scorer_encoder"]["innermost"]["aggr"] == "max"
    else:
        assert cfg["feat_size"] == entry["feat_size"] == 16
        assert cfg["backbone"] == numbers(entry["backbone"]["config"])
        assert cfg["backbone"]["down_conv"]["stride"] == [1, 2, 2, 2, 2, 2, 2] and cfg["scorer_unet"]["up_conv"]["N"] == 2
        # the configs build: the 7-level backbone gives feat_size channels, the scorers take them
        backbone = sc.SparseConv3dUnet(cfg["backbone"], feat)
        assert backbone.output_nc == 16 and len(backbone.down_modules) == 7 and len(backbone.up_modules) == 7
        net = pg.PointGroup(feat, 5, backbone=backbone, scorer_type="unet", scorer_unet=cfg["scorer_unet"])
        assert net.ScorerUnet.output_nc == 16 and net.ScorerHead[0].in_features == 16
    with pytest.raises(ValueError, match="unknown PointGroup configuration"):
        pg.pointgroup_config("PointGroup-LARGE", feat)


@pytest.mark.parametrize("kind", psr.KINDS)
def test_scorer_state_dict_is_the_references(kind):
    recorded = psr.fixture_numbers()
    net = pg.PointGroup(3, 5, backbone=_Backbone(), scorer_type=kind, **{"scorer_" + kind: recorded["fixture"][kind]})
    prefix = ("ScorerUnet." if kind == "unet" else "ScorerEncoder.", "ScorerHead.")
    got = [[k, list(v.shape)] for k, v in net.state_dict().items() if k.startswith(prefix)]
    assert sorted(got) == sorted(recorded["state_dicts"][kind])
    other = "ScorerEncoder" if kind == "unet" else "ScorerUnet"
    assert not hasattr(net, other) and not any(k.startswith(other) for k in net.state_dict())
    net.load_state_dict(psr.fixture_state(psr.load_fixture(kind)), strict=False)
    # the scorer takes the backbone's width or says so
    with pytest.raises(ValueError, match="the backbone gives 8"):
        pg.PointGroup(3, 5, backbone=_Backbone(), scorer_type=kind, **{"scorer_" + kind: pg._scorer_config(kind, 16, 1)})


def test_sparse_scorers_are_opt_in():
    """scorer_type "unet" / "encoder" without the scorer's config is refused as before (tests/test_pointgroup_cpu.py pins the
    error); with it the scorer is built, and the other scorer's config is not a substitute"""
    backbone = sc.SparseConv3dUnet("unet_4", 3, in_feat=4)
    cfg = {k: pg._scorer_config(k, backbone.output_nc, 1) for k in psr.KINDS}
    for kind in psr.KINDS:
        other = "encoder" if kind == "unet" else "unet"
        with pytest.raises(NotImplementedError, match="scorer_%s=<config>" % kind):
            pg.PointGroup(3, 5, scorer_type=kind, backbone=backbone)
        with pytest.raises(NotImplementedError, match="2\\^9 clouds"):
            pg.PointGroup(3, 5, scorer_type=kind, backbone=backbone, **{"scorer_" + other: cfg[other]})
        net = pg.PointGroup(3, 5, scorer_type=kind, backbone=backbone, **{"scorer_" + kind: cfg[kind]})
        assert hasattr(net, "ScorerUnet" if kind == "unet" else "ScorerEncoder") and net._scorer_cfg is cfg[kind]
    # a config handed to a model that does not use it builds nothing
    assert not hasattr(pg.PointGroup(3, 5, backbone=backbone, scorer_unet=cfg["unet"]), "ScorerUnet")


def test_default_model_keeps_its_keys():
    backbone = sc.SparseConv3dUnet("unet_4", 3, in_feat=4)
    net = pg.PointGroup(3, 5, backbone=backbone)
    keys = list(net.state_dict())
    assert [k for k in keys if not k.startswith("Backbone.")] == NON_BACKBONE_KEYS
    assert [k[len("Backbone."):] for k in keys if k.startswith("Backbone.")] == list(backbone.state_dict())
    assert net._scorer_type == "MLP" and net.cluster_voxel_size == 0.05
    assert list(pg.PointGroup(3, 5, backbone=backbone, scorer_type=None).state_dict()) == keys
    with pytest.raises(ValueError, match="unknown scorer_type"):
        pg.PointGroup(3, 5, backbone=backbone, scorer_type="Unet")


def test_clouds_are_validated_on_the_host():
    C = torch.tensor([[0, 0, 0, 0], [1, 2, 3, 512], [1, 2, 3, 511]], dtype=torch.int32)
    x = torch.zeros(3, 2)
    with pytest.raises(ValueError, match="batch < 2\\^9"):
        sc.SparseTensor(x, C)
    with pytest.raises(ValueError, match="batch < clouds = 512"):
        sc.SparseTensor(x, C, clouds=512)
    st = sc.SparseTensor(x, C, clouds=513)
    assert st.clouds == 513 and st._like(x + 1).clouds == 513 and sc.cat(st, st).clouds == 513 and (st + st).clouds == 513
    assert st.to("cpu") is st and sc.SparseTensor(x[:2], C[[0, 2]]).clouds is None
    sc.check_coords_host(C, clouds=513)
    sc.check_coords_host(torch.tensor([[0, 0, 0, (1 << 24) - 1]]), clouds=1 << 24)
    with pytest.raises(ValueError, match="out of range"):
        sc.check_coords_host(torch.tensor([[0, 0, 0, 1 << 24]]), clouds=1 << 24)
    with pytest.raises(ValueError, match="duplicate"):
        sc.SparseTensor(x, C[[0, 1, 1]], clouds=600)
    for bad in (0, -1, (1 << 24) + 1, 1.5, True):
        with pytest.raises(ValueError, match="clouds must be"):
            sc.SparseTensor(x, C, clouds=bad)
    assert sc.CLOUD_LIMIT_MAX == 1 << 24 and sc.BATCH_LIMIT == 1 << 9  # the default bound is unchanged


def test_innermost_aggregations():
    cfg = pg._scorer_config("encoder", 8, 1)
    enc = sc.SparseConv3dEncoder(cfg, 8)
    assert isinstance(enc.inner_modules[0], sc._GlobalMax) and enc.output_nc == 8
    assert type(sc.SparseConv3dEncoder("encoder_2", 3).inner_modules[0]) is sc._GlobalMean
    cfg["innermost"] = dict(cfg["innermost"], aggr="add")
    with pytest.raises(NotImplementedError, match="aggr 'add'"):
        sc.SparseConv3dEncoder(cfg, 8)
