"""PosPool / PPNet, host side (no GPU): the plain-torch restatement tests/ppnet_ref.py against the reference's own tensors
(tests/golden/ppnet.npz, written by tests/golden/make_golden_ppnet.py), strict loading of the reference's state_dicts,
the argument errors, the network table against the reference's resolved YAML and the C-ABI table."""
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from ppnet_ref import pospool_ref

OP_CASES = [("xyz", 12), ("sin_cos", 12), ("sin_cos", 9)]


def _sub(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def build_stage(g, fused=True):
    from torch_points3d_amd.ppnet import PPStageBlock
    grid, f = float(g["stage/grid"][0]), int(g["stage/width"][0])
    stage = PPStageBlock(block_names=["SimpleInputBlock", "ResnetBBlock"], down_conv_nn=[[4, f, f], [f, 2 * f]],
                         grid_size=[grid, grid], prev_grid_size=[grid, grid], has_bottleneck=[False, True],
                         bottleneck_ratio=2, max_num_neighbors=[20, 26], position_embedding="sin_cos", reduction="avg",
                         output_conv=False, bn_momentum=0.01, fused=fused)
    stage.load_state_dict(_sub(g, "stage/sd."), strict=True)
    return stage


def build_strided(g, fused=True):
    from torch_points3d_amd.ppnet import ResnetBBlock
    prev_grid, grid = (float(v) for v in g["strided/grids"])
    f = int(g["strided/width"][0])
    block = ResnetBBlock(down_conv_nn=[f, 2 * f], grid_size=grid, prev_grid_size=prev_grid, max_num_neighbors=22,
                         position_embedding="sin_cos", reduction="avg", has_bottleneck=True, bottleneck_ratio=2,
                         bn_momentum=0.01, fused=fused)
    block.load_state_dict(_sub(g, "strided/sd."), strict=True)
    return block


def op_inputs(g, table, embedding, C):
    """(b) runs both embeddings on the sin_cos C=12 features"""
    key = "_%s%d" % (embedding, C)
    return g["op/query"], g["op/support"], g[table], g["op/features" + key], g["op/cot" + key], float(g["op/radius"][0])


@pytest.mark.parametrize("reduction", ["sum", "avg"])
@pytest.mark.parametrize("embedding,C", OP_CASES)
def test_restatement_matches_reference_fixture(embedding, C, reduction):
    """fp32: the same torch operations in the same order up to the order of the sum over the slots; float64: equal"""
    g = load_golden("ppnet")
    q, s, nbr, x, cot, radius = op_inputs(g, "op/neighbors", embedding, C)
    tag = "op/%s%d_%s/" % (embedding, C, reduction)
    before = nbr.clone()
    f = x.clone().requires_grad_(True)
    out = pospool_ref(q, s, nbr, f, radius, embedding, reduction)
    assert torch.equal(nbr, before)
    (out * cot).sum().backward()
    torch.testing.assert_close(out.detach(), g[tag + "out"], rtol=1e-5, atol=1e-5 * max(1.0, float(g[tag + "out"].abs().max())))
    torch.testing.assert_close(f.grad, g[tag + "grad_features"], rtol=1e-4,
                               atol=1e-5 * float(g[tag + "grad_features"].abs().max()))
    out64 = pospool_ref(q.double(), s.double(), nbr, x.double(), radius, embedding, reduction)
    torch.testing.assert_close(out64, torch.from_numpy(g[tag + "out64"]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("embedding", ["xyz", "sin_cos"])
def test_count_rule_on_a_table_without_shadows(embedding):
    """no shadow: the rows that hold the largest index count one slot fewer per such slot (ops.py:107-108)"""
    g = load_golden("ppnet")
    q, s, nbr, x, cot, radius = op_inputs(g, "full/neighbors", "sin_cos", 12)
    assert int(nbr.min()) >= 0 and int(nbr.max()) == s.shape[0] - 1
    tag = "full/%s12_avg/" % embedding
    out = pospool_ref(q, s, nbr, x, radius, embedding, "avg")
    torch.testing.assert_close(out, g[tag + "out"], rtol=1e-5, atol=1e-5 * max(1.0, float(g[tag + "out"].abs().max())))
    total = pospool_ref(q, s, nbr, x, radius, embedding, "sum")
    count = (nbr < nbr.max()).sum(-1).float()
    assert int(count[3]) == nbr.shape[1] - 2 and int(count[40]) == nbr.shape[1] - 1 and int(count[0]) == nbr.shape[1]
    torch.testing.assert_close(out, total / (count + 1e-5)[:, None], rtol=1e-6, atol=1e-7)


def test_reference_state_dicts_load_strictly():
    g = load_golden("ppnet")
    stage = build_stage(g)
    keys = set(stage.state_dict())
    assert "blocks.1.aggregation.pospool.bn.batch_norm.weight" in keys and "blocks.0.unary_1.0.weight" in keys
    assert "blocks.0.pospool.bn.batch_norm.running_mean" in keys and "blocks.1.shortcut_op.0.weight" in keys
    assert keys == set(_sub(g, "stage/sd."))
    block = build_strided(g)
    assert set(block.state_dict()) == set(_sub(g, "strided/sd.")) and block.is_strided and block.sampler is not None
    assert stage.blocks[0].neighbour_finder._radius == pytest.approx(2.5 * float(g["stage/grid"][0]))
    assert len(stage.sampler) == 2 and stage.sampler[0] is None and len(stage.neighbour_finder) == 2


def test_layer_defaults_are_the_reference_ones():
    from torch_points3d_amd.ppnet import PosPoolLayer, ResnetBBlock, SimpleBlock
    layer = PosPoolLayer(12, 12, 0.1)
    assert layer.position_embedding == "xyz" and layer.reduction == "avg" and not layer.output_conv
    assert layer.activation.negative_slope == 0.2 and layer.bn.batch_norm.momentum == 0.02
    assert PosPoolLayer(12, 24, 0.1).output_conv and "oconv.1.batch_norm.weight" in PosPoolLayer(12, 24, 0.1).state_dict()
    blk = SimpleBlock(down_conv_nn=[12, 12], grid_size=0.1, prev_grid_size=0.1)
    assert blk.pospool.bn.batch_norm.momentum == 0.01 and blk.pospool.radius == pytest.approx(0.25) and blk.sampler is None
    res = ResnetBBlock(down_conv_nn=[12, 24], grid_size=0.1, prev_grid_size=0.1)
    assert res.aggregation.pospool.num_inputs == 12 and len(res.unary_2) == 2 and len(res.shortcut_op) == 2
    assert len(res.unary_1) == 3 and isinstance(ResnetBBlock(down_conv_nn=[12, 12], grid_size=0.1,
                                                             prev_grid_size=0.1).shortcut_op, torch.nn.Identity)


def test_argument_errors():
    from torch_points3d_amd.ppnet import PosPoolLayer, pospool
    q, s = torch.rand(5, 3), torch.rand(7, 3)
    nbr = torch.zeros(5, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="reference cannot run it either"):
        pospool(q, s, nbr, torch.rand(7, 12), 0.3, "xyz", "max")
    with pytest.raises(NotImplementedError, match="reference cannot run it either"):
        PosPoolLayer(12, 12, 0.3, reduction="max")
    with pytest.raises(ValueError):
        pospool(q, s, nbr, torch.rand(7, 10), 0.3, "xyz", "avg")
    with pytest.raises(ValueError):
        pospool(q, s, nbr, torch.rand(7, 15), 0.3, "sin_cos", "avg")
    with pytest.raises(ValueError):
        PosPoolLayer(8, 8, 0.3, position_embedding="sin_cos")
    with pytest.raises(NotImplementedError):
        pospool(q, s, nbr, torch.rand(7, 12), 0.3, "fourier", "avg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pospool(q, s, nbr, torch.rand(7, 12), 0.3, "sin_cos", "avg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pospool(q, s, nbr, torch.rand(7, 9), 0.3, "sin_cos", "sum")


@pytest.mark.parametrize("key,name,feat,grid", [("PPNet_feat4_grid0.04", "sin_cos", 4, 0.04),
                                                ("PPNetxyz_feat1_grid0.05", "xyz", 1, 0.05)])
def test_config_reproduces_reference_yaml(key, name, feat, grid):
    import inspect
    from torch_points3d_amd.ppnet import PPNet, ppnet_config
    ref = json.load(open(os.path.join(GOLDEN, "ppnet_config.json")))[key]
    const = ref["constants"]
    defaults = {k: v.default for k, v in inspect.signature(PPNet.__init__).parameters.items()}
    for k in ("in_feat", "bn_momentum", "reduction", "output_conv", "bottleneck_ratio"):
        assert defaults[k] == const[k], k  # the builder's defaults are the YAML's constants
    assert defaults["position_embedding"] == "sin_cos" and const["position_embedding"] == name
    cfg = ppnet_config(feat, in_grid_size=grid, position_embedding=name)
    down, up = ref["down_conv"], ref["up_conv"]
    assert len(cfg["down_conv"]) == len(down["down_conv_nn"]) == 5 and len(cfg["up_conv"]) == len(up["up_conv_nn"]) == 4
    for i, level in enumerate(cfg["down_conv"]):
        for k in ("down_conv_nn", "block_names", "has_bottleneck", "max_num_neighbors", "position_embedding", "reduction",
                  "output_conv", "bottleneck_ratio", "bn_momentum"):
            assert level[k] == down[k][i], (i, k)
        for k in ("grid_size", "prev_grid_size"):
            assert level[k] == pytest.approx(down[k][i], rel=1e-12), (i, k)
        # the strided flag is an exact float comparison in the reference: keep it exact here too
        assert [a != b for a, b in zip(level["prev_grid_size"], level["grid_size"])] == \
               [a != b for a, b in zip(down["prev_grid_size"][i], down["grid_size"][i])]
    assert down["module_name"] == "PPStageBlock" and up["module_name"] == "FPModule_PD" and up["skip"] is True
    for i, stage in enumerate(cfg["up_conv"]):
        assert stage["up_conv_nn"] == up["up_conv_nn"][i] and stage["up_k"] == up["up_k"][i] == 1
        assert stage["bn_momentum"] == up["bn_momentum"][i]
    assert cfg["mlp_cls"] == ref["mlp_cls"]


def test_net_builds_with_reference_names_on_cpu():
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.ppnet import PPNet
    torch.manual_seed(0)
    net = PPNet(4, 7, 0.04, in_feat=12)
    assert len(net.down_modules) == 5 and len(net.up_modules) == 4 and len(net.inner_modules) == 1
    keys = set(net.state_dict())
    for k in ("down_modules.0.blocks.0.unary_1.0.weight", "down_modules.1.blocks.0.aggregation.pospool.bn.batch_norm.bias",
              "down_modules.4.blocks.1.unary_2.1.batch_norm.running_var", "up_modules.0.nn.0.0.weight",
              "FC_layer.1.0.weight", "FC_layer.1.1.batch_norm.weight", "FC_layer.Class.weight"):
        assert k in keys, k
    assert net.FC_layer.Class.weight.shape == (7, 12) and net.up_modules[0].nn[0][0].weight.shape == (96, 576)
    assert [n for n, _ in net.FC_layer.named_children()] == ["1", "Class", "Softmax"]
    w = net.down_modules[2].blocks[1].unary_1[0].weight  # xavier-normal: std = sqrt(2 / (fan_in + fan_out))
    assert float(w.detach().std()) == pytest.approx((2.0 / sum(w.shape)) ** 0.5, rel=0.15)
    strided = [[b.sampler is not None for b in stage.blocks] for stage in net.down_modules]
    assert strided == [[False, False]] + [[True, False]] * 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(PDData(pos=torch.rand(50, 3), x=torch.rand(50, 4), batch=torch.zeros(50, dtype=torch.long)))


def test_abi_table_has_the_pospool_entry_points():
    from torch_points3d_amd import _lib
    text = open(os.path.join(ROOT, "include", "tp3d_hip.h")).read()
    assert _lib.ABI_VERSION == 39 and re.search(r"#define TP3D_ABI_VERSION 39\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tp3d_pospool_padding_i64", "tp3d_pospool_fwd_f32", "tp3d_pospool_bwd_f32"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, name
        assert len(_lib.SIGNATURES[name]) == decl.group(1).count(",") + 1, name
        assert hasattr(_lib.load(), name)
