"""Host side of the message-passing RSConv (torch_points3d_amd/rsconv_mp.py) and the consistency of its fixture
tests/golden/rsconv_mp.npz (tests/golden/make_golden_rsconv_mp.py): the plain-torch restatement tests/rsconv_mp_ref.py
has to reproduce what the REFERENCE's own classes computed before the GPU tests trust it.  No GPU.

Bars, as tests/test_pointnet2_mp_cpu.py: indices torch.equal; floats 1e-5 * max(1, scale) (the float64 arrays are met to
rounding, the stored gradients are float32 ones)."""
import pytest
import torch

from conftest import load_golden
import pointnet2_mp_ref as mp
import rsconv_mp_ref as ref

STAGES = ("rs1", "rs2", "glob", "fp0", "fp1", "fp2", "out")


@pytest.fixture(scope="module")
def gold():
    return load_golden("rsconv_mp")


def _sub(gold, prefix):
    return {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}


def _within(got, want, what):
    want = torch.as_tensor(want).double()
    scale = max(1.0, float(want.abs().max()))
    d = float((got.detach().double() - want).abs().max())
    print("restatement vs fixture, %s: max distance %.3e (bar %.1e)" % (what, d, 1e-5 * scale))
    assert got.shape == want.shape and d <= 1e-5 * scale, (what, d, scale)


def _grad_within(p, gold, prefix, name, what):
    """a Linear bias under train-mode BatchNorm has an analytically zero gradient: the stored float32 one is rounding
    noise of the weight gradient's size, and is held to tests/test_gpu_pointnet2_mp.py's rule for it"""
    want = gold[prefix + name]
    if name.endswith(".0.bias"):
        wn = float(gold[prefix + name[:-4] + "weight"].norm())
        assert float(p.grad.norm()) < 1e-4 * wn + 1e-6 and float(want.norm()) < 1e-4 * wn + 1e-6, name
    else:
        _within(p.grad, want, what + name)


def _gold_plan(oracle, gold):
    down, up = ref.GOLD_CFG["down_conv"], ref.GOLD_CFG["up_conv"]
    plan = mp.search_plan(oracle, gold["pos"], gold["batch"], down["ratios"], down["radius"], [ref.GOLD_CAP] * 2, up["up_k"])
    for i in range(2):  # the oracle's searches ARE the fixture's
        assert torch.equal(plan["idx"][i], gold["rs%d/idx" % (i + 1)])
        assert torch.equal(plan["edges"][i][0][0], gold["edges/rs%d/edge_start" % (i + 1)])
        assert torch.equal(plan["edges"][i][0][1], gold["edges/rs%d/col" % (i + 1)])
    return plan


def test_cpu_tensors_are_refused():
    from torch_points3d_amd.torchpoints import rsconv_msgmax, rsconv_relation_rows
    es, col = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rsconv_relation_rows(torch.rand(4, 3), torch.rand(2, 3), es, col)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rsconv_msgmax(torch.rand(3, 4), torch.rand(4, 4), es, col)


def test_restatement_of_the_kernels_by_hand():
    pos_s = torch.tensor([[0.0, 0, 0], [3.0, 4, 0], [1.0, 1, 1]])
    pos_q = torch.tensor([[0.0, 0, 0], [1.0, 1, 1]])
    es, col = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 2])
    rows = ref.relation_rows(pos_s, pos_q, es, col, ld=12)
    assert rows.shape == (3, 12)
    assert rows[0].tolist() == [0.0] * 12  # a query that is a support point at the origin
    assert rows[1].tolist() == [5.0, -3.0, -4.0, 0.0, 0.0, 0.0, 0.0, 3.0, 4.0, 0.0, 0.0, 0.0]  # query minus support
    assert rows[2].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    w = torch.tensor([[1.0, -1.0], [2.0, -2.0], [0.5, 0.5], [9.0, 9.0]])
    x = torch.tensor([[1.0, 1.0], [1.0, 2.0], [-4.0, -4.0]])
    out, arg = ref.msgmax(w, x, torch.tensor([0, 2, 2, 4]), torch.tensor([0, 1, 2, 2]))
    # query 0: products (1, -1), (2, -4); query 1: no edge; query 2: all negative -> the negative maximum, not 0
    assert out.tolist() == [[2.0, -1.0], [0.0, 0.0], [-2.0, -2.0]] and arg.tolist() == [[1, 0], [-1, -1], [2, 2]]


def test_fixture_is_self_consistent(gold):
    for k in STAGES:
        a, b = gold[k + "/x"], torch.as_tensor(gold["f64/" + k + "/x"])
        assert float((a.double() - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), k
        assert gold["eval/" + k + "/x"].shape == a.shape
    assert "x" not in gold  # no input features: x_j = pos_j at the first level
    sizes = torch.bincount(gold["batch"]).tolist()
    assert tuple(sizes) == ref.GOLD_SIZES
    l1 = mp.fps_quota(sizes, 0.25)
    assert torch.bincount(gold["rs1/batch"]).tolist() == l1 == [38, 25, 16]
    assert torch.bincount(gold["rs2/batch"]).tolist() == mp.fps_quota(l1, 0.25) == [10, 7, 4]
    cap = int(gold["cap"])
    assert cap == 64
    for tag, nq in (("edges/rs1", 79), ("edges/rs2", 21), ("conv", 79)):
        es, col = gold[tag + "/edge_start"], gold[tag + "/col"]
        deg = es[1:] - es[:-1]
        assert es.numel() == nq + 1 and int(es[0]) == 0 and int(es[-1]) == col.numel()
        assert int(deg.min()) >= 1 and int(deg.max()) <= cap, "a query without an edge, or past the cap"
    deg = gold["edges/rs1/edge_start"][1:] - gold["edges/rs1/edge_start"][:-1]
    assert int(deg.max()) == cap and int((deg == cap).sum()) >= 5 and int((deg < cap).sum()) >= 5
    # the stand-alone Convolution: a support row wins for two different queries in one channel
    winners = gold["conv/col"][gold["conv/arg"]]
    assert max(int(torch.bincount(winners[:, c]).max()) for c in range(winners.shape[1])) >= 2
    for lvl in (1, 2):  # argmax is an absolute edge index inside the query's run
        es, arg = gold["edges/rs%d/edge_start" % lvl], gold["rs%d/arg" % lvl]
        assert bool((arg >= es[:-1, None]).all()) and bool((arg < es[1:, None]).all())


def test_float64_restatement_reproduces_the_fixture(oracle, gold):
    sd = _sub(gold, "sd/")
    net = ref.RSConvMP.from_state_dict(sd, torch.float64)
    assert net.levels == 2 and list(net.state_dict().keys()) == list(sd.keys())
    plan = _gold_plan(oracle, gold)
    rec = net(None, gold["pos"].double(), gold["batch"], plan)
    for k in STAGES:
        _within(rec[k], gold["f64/" + k + "/x"], k)
    blocks = net.blocks()
    for lvl in (1, 2):
        assert torch.equal(blocks[lvl - 1].down._conv.arg, gold["rs%d/arg" % lvl])
    (rec["out"] * gold["cot"].double()).sum().backward()
    checked = 0
    for name, p in net.named_parameters():
        assert ("pgrad/" + name) in gold and p.grad is not None, name
        _grad_within(p, gold, "pgrad/", name, "grad ")
        checked += 1
    assert checked > 40
    net32 = ref.RSConvMP.from_state_dict(sd, torch.float32)
    rec32 = net32(None, gold["pos"], gold["batch"], plan)
    for k in STAGES:
        _within(rec32[k], gold["f64/" + k + "/x"], k + " (float32 restatement)")


def test_float64_restatement_reproduces_the_stand_alone_convolution(gold):
    sd = _sub(gold, "conv/sd/")
    conv = ref.Convolution.from_state_dict(sd, torch.float64)
    x = gold["conv/x_in"].double().requires_grad_(True)
    pos = gold["pos"].double()
    out = conv(x, (pos, pos[gold["conv/idx"]]), (gold["conv/edge_start"], gold["conv/col"]))
    _within(out, gold["conv/f64/x"], "Convolution")
    assert torch.equal(conv.arg, gold["conv/arg"])
    (out * gold["conv/cot"].double()).sum().backward()
    _within(x.grad, gold["conv/grad_x"], "Convolution grad x")
    for name, p in conv.named_parameters():
        _grad_within(p, gold, "conv/pgrad/", name, "Convolution grad ")


def test_state_dict_keys_match_the_reference(gold):
    from torch_points3d_amd.rsconv_mp import Convolution, RSConvDown, RSConvMP
    net_sd = _sub(gold, "sd/")
    assert len(net_sd) > 80
    net = RSConvMP(ref.GOLD_CFG, ref.GOLD_CLASSES)
    assert list(net.state_dict().keys()) == list(net_sd.keys())
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(net_sd[k].shape), k
    down = ref.GOLD_CFG["down_conv"]
    rs = RSConvDown(ratio=down["ratios"][0], radius=down["radius"][0], local_nn=down["local_nn"][0],
                    down_conv_nn=down["down_conv_nn"][0])
    assert list(rs.state_dict().keys()) == list(_sub(gold, "sd/model.down."))
    assert rs.neighbour_finder._max_num_neighbors == 64
    conv = Convolution(local_nn=ref.GOLD_CONV["local_nn"], global_nn=ref.GOLD_CONV["global_nn"])
    conv_sd = _sub(gold, "conv/sd/")
    assert list(conv.state_dict().keys()) == list(conv_sd.keys())
    for k, v in conv.state_dict().items():
        assert tuple(v.shape) == tuple(conv_sd[k].shape), k
    with pytest.raises(NotImplementedError):
        Convolution(local_nn=[10, 8, 3], aggr="add")


def _widths(mlp):
    return [mlp[0][0].in_features] + [blk[0].out_features for blk in mlp]


def _levels(net):
    out, b = [], net.model
    while not b.innermost:
        out.append(b)
        b = b.submodule
    return out, b


@pytest.mark.parametrize("name,classes", [("RSConv_2LD", 13), ("RSConv_4LD", 13)])
def test_published_configurations_build_with_the_yaml_widths(name, classes):
    """conf/models/segmentation/rsconv.yaml:3-55 with FEAT = 3 (x = None)"""
    from torch_points3d_amd.rsconv_mp import RSConvMP, rsconv_mp_config
    want = {
        "RSConv_2LD": dict(local=[[10, 8, 3], [10, 32, 64, 64]], down=[[3, 16, 32, 64], [64, 64, 128]], inner=[131, 128],
                           up=[[256, 64], [128, 64], [64, 64]], ratios=[0.2, 0.25], radius=[0.1, 0.2], dropout=0.5),
        "RSConv_4LD": dict(local=[[10, 8, 3], [10, 16, 16], [10, 32, 32], [10, 64, 64]],
                           down=[[3, 16, 16], [16, 32, 32], [32, 64, 64], [64, 128, 128]], inner=[131, 128],
                           up=[[256, 128], [192, 64], [96, 32], [48, 32], [32, 64]], ratios=[0.5] * 4,
                           radius=[0.1, 0.2, 0.3, 0.4], dropout=0.1),
    }[name]
    cfg = rsconv_mp_config(name)
    net = RSConvMP(name, classes)
    levels, inner = _levels(net)
    assert len(levels) == len(want["local"])
    for i, b in enumerate(levels):
        assert _widths(b.down._conv.local_nn) == want["local"][i] and _widths(b.down._conv.global_nn) == want["down"][i]
        assert b.down.sampler._ratio == want["ratios"][i] and b.down.neighbour_finder._radius == want["radius"][i]
        assert b.down.neighbour_finder._max_num_neighbors == 64
    assert _widths(inner.inner.nn) == want["inner"]
    ups = [inner.up] + [b.up for b in reversed(levels)]
    assert [_widths(u.nn) for u in ups] == want["up"] and [u.k for u in ups] == cfg["up_conv"]["up_k"]
    assert all(u.nn[0][0].bias is None for u in ups)
    assert net.dropout == want["dropout"]
    assert (net.lin1.in_features, net.lin2.in_features, net.lin3.in_features, net.lin3.out_features) == (64, 64, 64, classes)
    with pytest.raises(ValueError):
        rsconv_mp_config("RSConv_MSN")
