"""MS-SVConv without a GPU: argument rules of WideConv3d and the routing switch, the stage-list handling of the U-Net, the
resolved configurations against the recorded YAML entries, state_dict names against the lists recorded from the reference's
classes, the fixture's safety conditions, the plain-torch restatement (tests/ms_svconv_ref.py) against the fixture in fp32 and
float64, the new symbols in the header and the binding, and the rounding rule as data."""
import os
import re

import pytest
import torch

import ms_svconv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BACKBONE = dict(down_conv=dict(module_name="ResNetDown", dimension=3, down_conv_nn=[[1, 8], [8, 16]], kernel_size=[5, 3],
                               stride=[1, 2], dilation=[1, 1]),
                up_conv=dict(module_name="ResNetUp", dimension=3, bn_momentum=0.05, up_conv_nn=[[16, 8], [16, 8]],
                             kernel_size=[3, 3], stride=[2, 1], dilation=[1, 1]))
OPTION_UNET = dict(input_nc=1, grid_size=[0.05, 0.1], post_mlp_nn=[8, 8], backbone=BACKBONE)
MLP_CLS = dict(nn=[16, 8, 8], bn_momentum=0.05)


def test_wide_conv3d_argument_rules():
    from torch_points3d_amd import sparseconv as sc
    for k in (3, 5):
        m = sc.WideConv3d(2, 6, kernel_size=k)
        assert isinstance(m, sc.Conv3d) and m.kernel.shape == (k ** 3, 2, 6) and m.bias is None
        bound = 1.0 / (2 * k ** 3) ** 0.5  # the initialisation rule of Conv3d
        assert float(m.kernel.abs().max()) <= bound and float(m.kernel.abs().max()) > 0.5 * bound
    with pytest.raises(NotImplementedError, match="stride"):
        sc.WideConv3d(2, 6, kernel_size=5, stride=2)
    with pytest.raises(NotImplementedError, match="transposed"):
        sc.WideConv3d(2, 6, kernel_size=5, transposed=True)
    with pytest.raises(NotImplementedError, match="dilation"):
        sc.WideConv3d(2, 6, kernel_size=5, dilation=2)
    for k in (1, 2, 4, 7):
        with pytest.raises(NotImplementedError, match="kernel_size"):
            sc.WideConv3d(2, 6, kernel_size=k)


def test_conv3d_still_rejects_kernel_size_5():
    from torch_points3d_amd import sparseconv as sc
    with pytest.raises(NotImplementedError, match="kernel_size"):
        sc.Conv3d(4, 4, kernel_size=5)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        sc.Conv3dTranspose(4, 4, kernel_size=5)


def test_wide_route_values(monkeypatch):
    from torch_points3d_amd import sparseconv as sc
    assert sc.WIDE_ROUTE == "auto"
    for route, one, four in (("auto", True, False), ("wide", True, True), ("generic", False, False)):
        monkeypatch.setattr(sc, "WIDE_ROUTE", route)  # "auto": the measured winner only (profiles/ms_svconv_bench.json)
        assert sc._wide_route(125, 1) is one and sc._wide_route(125, 4) is four
        assert sc._wide_route(125, 5) is False and sc._wide_route(27, 1) is False
    monkeypatch.setattr(sc, "WIDE_ROUTE", "fast")
    with pytest.raises(ValueError, match="WIDE_ROUTE"):
        sc._wide_route(125, 1)


def test_stage_lists_without_N_and_with_extra_keys():
    from torch_points3d_amd import sparseconv as sc
    net = sc.SparseConv3dUnet(BACKBONE, input_nc=1)
    first = net.down_modules[0]
    assert type(first.conv_in[0]) is sc.WideConv3d and first.conv_in[0].kernel.shape == (125, 1, 8)
    assert len(first.blocks) == 1 and len(net.down_modules[1].blocks) == 1 and len(net.up_modules[0].blocks) == 1
    assert all(type(m) is not sc.WideConv3d for m in first.blocks.modules())  # the blocks are kernel_size 3
    assert type(net.down_modules[1].conv_in[0]) is sc.Conv3d
    assert "down_modules.0.conv_in.0.kernel" in net.state_dict()
    assert net.output_nc == 8
    with pytest.raises(NotImplementedError, match="kernel_size"):
        sc.ResNetUp(up_conv_nn=[16, 8], kernel_size=5, stride=1)
    # the configurations of applications/conf/sparseconv3d keep their explicit N
    assert [len(m.blocks) if m.blocks else 0 for m in sc.SparseConv3dUnet("unet_4", input_nc=3).down_modules] == [0, 1, 2, 2, 3]


def test_configurations():
    from torch_points3d_amd import ms_svconv as ms
    assert len(ms.REGISTRATION_ENTRIES) == 15 and len(set(ms.REGISTRATION_ENTRIES)) == 15
    down = [[1, 32], [32, 64], [64, 128], [128, 256]]
    up = [[256, 64], [192, 64], [128, 64], [96, 64]]
    for base, size in (("B2cm", 0.02), ("B4cm", 0.04), ("B6cm", 0.06)):
        for heads, scales in (("1head", 1), ("2head", 2), ("3head", 3), ("3head_unshared", 3), ("4head", 4)):
            c = ms.ms_svconv_config("MS_SVCONV_%s_X2_%s" % (base, heads))
            o = c["option_unet"]
            assert c["cls"] == ("MS_SparseConv3d" if "unshared" in heads else "MS_SparseConv3d_Shared")
            assert o["grid_size"] == pytest.approx([size * 2 ** i for i in range(scales)], rel=1e-12) and o["input_nc"] == 1
            assert o["post_mlp_nn"] == [64, 32] and c["mlp_cls"] == dict(nn=[32 * scales, 32, 32], bn_momentum=0.05)
            assert c["normalize_feature"] is True and c["loss_mode"] == "match" and c["backend"] == "torchsparse"
            assert c["metric_loss"]["params"] == dict(num_pos=1024, num_hn_samples=256, pos_thresh=0.1, neg_thresh=1.4)
            d, u = o["backbone"]["down_conv"], o["backbone"]["up_conv"]
            assert d["down_conv_nn"] == down and d["kernel_size"] == [5, 3, 3, 3] and d["stride"] == [1, 2, 2, 2] and "N" not in d
            assert u["up_conv_nn"] == up and u["kernel_size"] == [3, 3, 3, 3] and u["stride"] == [2, 2, 2, 1] and "N" not in u
    seg = ms.ms_svconv_config(ms.SEGMENTATION_ENTRY)
    assert seg["cls"] == "MS_SparseConvModel" and seg["output_nc"] == 32 and seg["option_unet"]["grid_size"] == [0.04, 0.08, 0.16]
    assert ms.ms_svconv_config("MS_SVCONV_B2cm_X2_1head", input_nc=4)["option_unet"]["backbone"]["down_conv"]["down_conv_nn"][0] == [4, 32]
    with pytest.raises(ValueError):
        ms.ms_svconv_config("MS_SVCONV_B8cm_X2_1head")


def _names(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_names_equal_the_restatement():
    from torch_points3d_amd import ms_svconv as ms
    pairs = [
        (ms.UnetMSparseConv3d(BACKBONE, post_mlp_nn=[8, 8], pre_mlp_nn=[1, 4, 1], pointnet_nn=[1, 4, 1]),
         ref.Unet(BACKBONE, post_mlp_nn=[8, 8], pre_mlp_nn=[1, 4, 1], pointnet_nn=[1, 4, 1])),
        (ms.MS_SparseConv3d(OPTION_UNET, MLP_CLS), ref.MSNet(BACKBONE, [0.05, 0.1], [16, 8, 8], shared=False, post_mlp_nn=[8, 8])),
        (ms.MS_SparseConv3d_Shared(OPTION_UNET, MLP_CLS), ref.MSNet(BACKBONE, [0.05, 0.1], [16, 8, 8], post_mlp_nn=[8, 8])),
        (ms.MS_SparseConvModel(OPTION_UNET, MLP_CLS, 8, 4), ref.MSNet(BACKBONE, [0.05, 0.1], [16, 8, 8], post_mlp_nn=[8, 8],
                                                                      num_classes=4)),
    ]
    for hip, r in pairs:
        assert _names(hip) == _names(r), type(hip).__name__
    shared = _names(pairs[2][0])
    for key in ("unet.unet.down_modules.0.conv_in.0.kernel", "unet.post_mlp.0.0.bias", "unet.post_mlp.0.1.batch_norm.running_mean",
                "FC_layer.0.0.weight", "FC_layer.1.1.batch_norm.weight"):
        assert key in shared, key
    assert shared["unet.unet.down_modules.0.conv_in.0.kernel"] == (125, 1, 8) and "FC_layer.0.0.bias" not in shared
    assert "unet.1.unet.down_modules.0.conv_in.0.kernel" in _names(pairs[1][0]) and "head.0.bias" in _names(pairs[3][0])


def test_not_served_options_raise():
    from torch_points3d_amd import ms_svconv as ms
    with pytest.raises(NotImplementedError, match="minkowski"):
        ms.UnetMSparseConv3d(BACKBONE, backend="minkowski")
    with pytest.raises(NotImplementedError, match="loss_mode"):
        ms.MS_SparseConv3d_Shared(OPTION_UNET, MLP_CLS, loss_mode="label")
    with pytest.raises(NotImplementedError, match="pool_mode"):
        ms.MS_SparseConv3d_Shared_Pool(OPTION_UNET, MLP_CLS, pool_mode="sum")


def test_scale_fuse_argument_rules():
    from torch_points3d_amd import torchpoints as tp
    with pytest.raises(ValueError, match="mode"):
        tp.scale_fuse([torch.zeros(2, 3)], "sum")
    with pytest.raises(ValueError, match="1 to 8"):
        tp.scale_fuse([torch.zeros(2, 3)] * 9)


def test_restatement_k5_equals_the_table_sum():
    """the dense k = 5 definition (F.conv3d, padding 2, grid indexed [x, y, z]) and the sum over the brute-force table are
    one function, in float64, at tensor strides 1 and 2"""
    g = torch.Generator().manual_seed(0)
    for ts in (1, 2):
        C = torch.unique(torch.cat([torch.randint(-4, 5, (110, 3), generator=g) * ts, torch.randint(0, 2, (110, 1), generator=g)], 1),
                         dim=0).int()
        x = torch.randn(len(C), 3, generator=g, dtype=torch.float64)
        W = torch.randn(125, 3, 4, generator=g, dtype=torch.float64)
        fwd, inv = ref.kernel_map(C, C, 5, ts)
        assert torch.equal(inv, fwd.flip(1)) and torch.equal(fwd[:, 62], torch.arange(len(C), dtype=torch.int32))
        dense = ref.conv(x, C, C, W, 5, 1, ts)
        assert float((dense - ref.conv_by_table(x, fwd, W)).abs().max()) < 1e-12
        # the input gradient is the mirrored table with W transposed
        xr = x.clone().requires_grad_(True)
        cot = torch.randn(len(C), 4, generator=g, dtype=torch.float64)
        (ref.conv(xr, C, C, W, 5, 1, ts) * cot).sum().backward()
        assert float((xr.grad - ref.conv_by_table(cot, inv, W.transpose(1, 2))).abs().max()) < 1e-12


def test_new_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "tp3d_hip.h")).read()
    from torch_points3d_amd import _lib
    assert _lib.ABI_VERSION == 39 and re.search(r"#define TP3D_ABI_VERSION 39\b", header)
    for name in ("tp3d_sparse_conv_wide_f32", "tp3d_sparse_wgrad_wide_f32", "tp3d_scale_fuse_fwd_f32", "tp3d_scale_fuse_bwd_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header), name
        args = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]), name
    for name in ("tp3d_sparse_conv_wide_serves", "tp3d_sparse_wgrad_wide_chunks", "tp3d_sparse_wgrad_wide_workspace_floats"):
        assert name in _lib.MISC and re.search(r"\b%s\(" % name, header), name


def test_round_half_to_even_known_answers():
    got = torch.round(torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5]))
    assert got.tolist() == [0.0, 2.0, 2.0, -0.0, -2.0] and bool(torch.signbit(got[3]))


# ------------------------------------------------------------------------- the reference-generated fixture (README_ms_svconv.md)
import ms_svconv_golden_util as gu  # noqa: E402

KINK_MARGIN, HALF_MARGIN, MAX_MARGIN, GAP_MARGIN, COARSE_ROWS = 5e-5, 1e-3, 1e-6, 1e-4, 8


def test_config_equals_the_recorded_yaml_entries():
    from torch_points3d_amd import ms_svconv as ms
    entries = gu.config()["entries"]
    assert sorted(entries) == sorted(ms.REGISTRATION_ENTRIES + [ms.SEGMENTATION_ENTRY]) and len(entries) == 16
    for name, want in entries.items():
        got = ms.ms_svconv_config(name)
        assert want["class"] == "ms_svconv3d." + got["cls"], name
        for key in ("option_unet", "mlp_cls", "normalize_feature", "backend"):
            assert got[key] == want[key], (name, key)
        for key in ("loss_mode", "metric_loss", "output_nc"):
            assert (key in got) == (key in want) and got.get(key) == want.get(key), (name, key)
        assert set(want) - set(got) <= {"class", "conv_type"}, name


def test_state_dict_names_equal_the_recorded_reference_lists():
    from torch_points3d_amd import ms_svconv as ms
    rec = gu.config()["state_dicts"]
    seg = ms.ms_svconv_config(ms.SEGMENTATION_ENTRY)
    models = {
        "MS_SVCONV_B2cm_X2_3head": ms.build("MS_SVCONV_B2cm_X2_3head"),
        "MS_SVCONV_B2cm_X2_3head_unshared": ms.build("MS_SVCONV_B2cm_X2_3head_unshared"),
        ms.SEGMENTATION_ENTRY: ms.MS_SparseConvModel(seg["option_unet"], seg["mlp_cls"], seg["output_nc"],
                                                     gu.config()["segmentation_num_classes"]),
    }
    assert sorted(rec) == sorted(models)
    for name, m in models.items():
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert sorted(got) == sorted(rec[name]), name
        assert len(got) > 100


def test_fixture_voxel_tables_and_input_margins():
    g = gu.load()
    grids = gu.fixture_numbers()[0]
    for c in (0, 1):
        pos, batch = g["pos%d" % c], g["batch%d" % c]
        for i, gs in enumerate(grids):
            q = pos.double() / gs
            assert float((q - torch.floor(q) - 0.5).abs().min()) >= HALF_MARGIN
            t = "tables/cloud%d/scale%d/" % (c, i)
            coords, vb, vpos, _, cluster, upi = ref.voxelize(pos, batch, gs, pos)
            assert torch.equal(cluster, g[t + "cluster"]) and torch.equal(upi, g[t + "unique_pos_indices"])
            assert torch.equal(coords, g[t + "coords"]) and torch.equal(vb, g[t + "batch"])
            assert len(coords) < len(pos)  # a voxel with several points
            C = torch.cat([coords, vb.unsqueeze(1)], 1)
            assert len(ref.sr.down_coords(C, 2)) >= COARSE_ROWS
    # the drawn candidate rows lie in distinct voxels at every scale (rows of one voxel carry equal descriptors)
    for sel in gu.selections(g):
        for c, key in ((0, "sel0"), (1, "sel1")):
            for i in range(2):
                cl = g["tables/cloud%d/scale%d/cluster" % (c, i)][sel[key]]
                assert len(torch.unique(cl)) == len(cl)


@pytest.mark.parametrize("tag", gu.CASES)
def test_restatement_reproduces_the_fixture_and_its_safety_conditions(tag):
    """float64: the restatement equals the reference's pass to rounding; fp32: two fp32 evaluations of one formula lie within
    their distances to the float64 one (bar: 1e-5 of the scale plus four times the recorded distance)"""
    g = gu.load()
    parts = []
    r64, m64, kink = gu.run_ref(tag, g, torch.float64, parts=parts)
    assert kink >= KINK_MARGIN, kink
    if parts:
        assert min(float(p["gap"].min()) for p in parts) >= GAP_MARGIN
        assert min(float(p["relu_args"].abs().min()) for p in parts) >= KINK_MARGIN
        assert len(parts) == (3 if tag == "shared" else 1)
    if tag == "pool_max":
        for side in ("", "_target"):
            assert float((g["pool_max/f64/scale0" + side] - g["pool_max/f64/scale1" + side]).abs().min()) >= MAX_MARGIN
    r32, m32, _ = gu.run_ref(tag, g, torch.float32)
    t = tag + "/"
    seen = 0
    for k in r64:
        want64, want32 = g[t + "f64/" + k], g[t + k]
        scale = max(1.0, float(want64.abs().max()))
        assert float((r64[k] - want64).abs().max()) <= 1e-10 * scale, (tag, k)
        own = float((want32.double() - want64).abs().max())
        assert float((r32[k].double() - want32.double()).abs().max()) <= 1e-5 * scale + 4 * own, (tag, k)
        seen += 1
    assert seen >= (1 if tag == "unet" else 3) and all(k[len(t):] in r64 for k in g if k.startswith(t) and k.count("/") == 1 and k != t + "seed")
    p32 = dict(m32.named_parameters())
    for name, p in m64.named_parameters():
        want64 = g[t + "f64/pgrad/" + name]
        scale = max(1.0, float(want64.abs().max()))
        assert float((p.grad - want64).abs().max()) <= 1e-9 * scale, (tag, name)
        own = float(g[t + "pgrad_own/" + name])
        assert float((p32[name].grad.double() - want64).abs().max()) <= 1e-5 * scale + 4 * own, (tag, name)
    s32, s64 = m32.state_dict(), m64.state_dict()
    for k in s64:
        if "running_" in k:
            assert float((s64[k] - g[t + "f64/after/" + k]).abs().max()) <= 1e-10 * max(1.0, float(s64[k].abs().max())), (tag, k)
            torch.testing.assert_close(s32[k], g[t + "after/" + k], rtol=1e-5, atol=1e-6)
