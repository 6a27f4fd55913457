"""RandLA-Net networks without a GPU: the resolved configs, the route function's truth table, the sorted sampler, and
RandLANetSeg on CPU tensors (rows arithmetic) against the fixtures the REFERENCE's own classes produced
(tests/golden/make_golden_randlanet.py).  The searches here are the oracle's."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
import randlanet_util as ru


@pytest.fixture(scope="module", params=ru.CONFIGS)
def case(request):
    return request.param, ru.load_fixture(request.param)


# ---------------------------------------------------------------- configs

def test_randla_config_matches_the_yaml_numbers():
    """randlanet_config.json: the reference's YAML with FEAT resolved by the generator; a few widths spelled out here"""
    from torch_points3d_amd.randla import randla_config
    with open(os.path.join(GOLDEN, "randlanet_config.json")) as f:
        want = json.load(f)
    for feat in (3, 6):
        for name in ru.CONFIGS:
            got, ref = randla_config(name, feat), want["FEAT=%d" % feat][name]
            for part in ("down_conv", "up_conv", "innermost", "mlp_cls"):
                for field, v in ref[part].items():
                    if field == "module_name" and part != "down_conv":
                        continue
                    assert got[part][field] == v, (feat, name, part, field, got[part].get(field), v)
    conv = randla_config("Randlanet_Conv", 6)
    assert conv["down_conv"]["point_pos_nn"] == [[10, 8, 6], [10, 8, 16], [10, 16, 32]]
    assert conv["down_conv"]["attention_nn"] == [[12, 8, 12], [32, 64, 32], [64, 128, 64]]
    assert conv["down_conv"]["down_conv_nn"] == [[12, 8, 16], [32, 64, 32], [64, 128, 128]]
    assert conv["up_conv"]["up_conv_nn"] == [[256, 128], [160, 64], [80, 64], [70, 64]]
    assert conv["innermost"]["nn"] == [131, 128] and conv["up_conv"]["up_k"] == [1, 1, 1, 1]
    res = randla_config("Randlanet_Res", 3)
    assert res["down_conv"]["ratio"] == [[1, 1], [0.5, 0.5]] and res["down_conv"]["outdim"] == [32, 128]
    assert res["down_conv"]["attention_nn"] == [[[6, 8, 6], [32, 64, 32]], [[64, 128, 64], [128, 256, 128]]]
    assert res["up_conv"]["up_conv_nn"] == [[256, 128], [160, 64], [67, 64]]
    with pytest.raises(ValueError):
        randla_config("Randlanet", 3)


def test_state_dict_keys_are_the_references(case):
    from torch_points3d_amd.randla import RandLANetSeg
    name, gold = case
    net = RandLANetSeg(name, ru.FEAT, ru.CLASSES)
    sd = ru.state_of(gold)
    assert set(net.state_dict()) == set(sd)
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    assert "model.down._conv." + ("point_pos_nn" if name == "Randlanet_Conv" else "conv1._conv.point_pos_nn") + \
        ".0.0.weight" in sd
    assert all(conv._conv.lfa == "auto" and conv.sampler._sort for conv in ru.samplers(net))


# ---------------------------------------------------------------- the route function

def test_lfa_route_truth_table():
    from torch_points3d_amd import randla
    from torch_points3d_amd.partial_dense import MLP
    route = randla.lfa_route
    ok = dict(holes=False, training=False, device="cuda")
    served = [(3, [10, 8, 3], [6, 8, 6]), (6, [10, 8, 6], [12, 8, 12]), (16, [10, 8, 16], [32, 64, 32]),
              (32, [10, 16, 32], [64, 128, 64]), (5, [10, 7, 6], [11, 7, 11]), (16, [10, 16, 16], [32, 64, 32])]
    for Cx, pp, at in served:
        want = "fused" if randla.LFA_MEASURED_WIN[randla.lfa_width_class(Cx + pp[2])] else "rows"
        assert route(16, Cx, pp, at, **ok) == want, (Cx, pp, at)
        assert route(16, Cx, MLP(pp), MLP(at), **ok) == want  # modules are read for their widths
        assert route(16, Cx, pp, at, holes=True, training=False, device="cuda") == "rows"
        assert route(16, Cx, pp, at, holes=False, training=True, device="cuda") == "rows"
        assert route(16, Cx, pp, at, holes=False, training=False, device="cpu") == "rows"
        assert route(16, Cx, pp, at, holes=False, training=False, device=torch.device("cuda", 0)) == want
        assert route(8, Cx, pp, at, **ok) == "rows" and route(32, Cx, pp, at, **ok) == "rows"
    # the last convolution of Randlanet_Res: C = 128, A1 = 256
    assert route(16, 64, [10, 32, 64], [128, 256, 128], **ok) == "rows"
    assert route(16, 32, [10, 16, 32], [64, 129, 64], **ok) == "rows"  # A1 > 128
    assert route(16, 33, [10, 16, 32], [65, 64, 65], **ok) == "rows"  # C > 64
    assert route(16, 3, [10, 65, 3], [6, 8, 6], **ok) == "rows"  # P1 > 64
    assert route(16, 3, [10, 8, 8, 3], [6, 8, 6], **ok) == "rows"  # three-layer MLP
    assert route(16, 3, [10, 8, 3], [6, 8, 8, 6], **ok) == "rows"
    assert route(16, 3, [10, 8, 3], [7, 8, 7], **ok) == "rows"  # attention width is not Cx + P2
    assert route(16, 3, [9, 8, 3], [6, 8, 6], **ok) == "rows"
    # a class that is not recorded as a win goes to rows
    saved = dict(randla.LFA_MEASURED_WIN)
    try:
        randla.LFA_MEASURED_WIN[32] = False
        assert route(16, 16, [10, 8, 16], [32, 64, 32], **ok) == "rows"
    finally:
        randla.LFA_MEASURED_WIN.update(saved)
    assert [randla.lfa_width_class(c) for c in (1, 6, 16, 17, 32, 33, 64, 65)] == [16, 16, 16, 32, 32, 64, 64, None]


def test_kernel_keyword_on_cpu_tensors():
    """CPU tensors always take the existing path: "auto" equals "rows" bit for bit, "fused" refuses, a bad word raises"""
    from torch_points3d_amd.randla import RandlaKernel
    g = torch.Generator().manual_seed(5)
    pos = torch.rand(40, 3, generator=g)
    nbr = torch.randint(0, 40, (9, 16), generator=g)
    x = torch.randn(40, 6, generator=g)
    kw = dict(point_pos_nn=[10, 8, 6], attention_nn=[12, 8, 12], global_nn=[12, 8, 16])
    torch.manual_seed(1)
    rows = RandlaKernel(**kw).eval()
    assert rows.lfa == "rows"
    auto = RandlaKernel(lfa="auto", **kw).eval()
    auto.load_state_dict(rows.state_dict())
    with torch.no_grad():
        assert torch.equal(auto(x, (pos[:9], pos), nbr), rows(x, (pos[:9], pos), nbr))
        fused = RandlaKernel(lfa="fused", **kw).eval()
        with pytest.raises(ValueError, match="lfa='fused'"):
            fused(x, (pos[:9], pos), nbr)
    with pytest.raises(ValueError):
        RandlaKernel(lfa="always", **kw)


# ---------------------------------------------------------------- the sampler

def test_sorted_sampler_is_the_sorted_multiset_of_the_same_draw():
    from torch_points3d_amd.randla import RandlaConv, RandomSampler
    pos = torch.zeros(1000, 3)
    for ratio in (0.25, 1, 0.5):
        torch.manual_seed(77)
        plain = RandomSampler(ratio)(pos)
        torch.manual_seed(77)
        ordered = RandomSampler(ratio, sort=True)(pos)
        assert plain.numel() == int(1000 * ratio) and len(set(plain.tolist())) < plain.numel()  # with replacement
        assert torch.equal(ordered, torch.sort(plain)[0]) and not torch.equal(ordered, plain)
        torch.manual_seed(77)
        assert torch.equal(RandomSampler(ratio)(pos), plain)  # the default draw is what it was
    kw = dict(point_pos_nn=[10, 8, 3], attention_nn=[6, 8, 6], down_conv_nn=[6, 8, 16])
    assert not RandlaConv(0.25, 16, **kw).sampler._sort and RandlaConv(0.25, 16, sort=True, **kw).sampler._sort


# ---------------------------------------------------------------- the fixture on CPU tensors

def _host_searches(monkeypatch, oracle, net):
    """the three device searches of the network, on the oracle: kNN, nearest-row interpolation, per-cloud max"""
    from torch_points3d_amd import pointnet2_mp, randla

    def knn(k, x, y, bx=None, by=None, **kw):
        return oracle.knn(k, x.float(), y.float(), bx, by)

    def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, skip=None):
        assert k == 1
        idx, _ = oracle.knn(1, pos_x.float(), pos_y.float(), batch_x, batch_y)
        out = x[idx.reshape(-1)]
        return out if skip is None else torch.cat([out, skip], 1)

    def max_pool(x, batch):
        return torch.stack([x[batch == b].max(0)[0] for b in range(int(batch.max()) + 1)])

    monkeypatch.setattr(randla._tp, "knn", knn)
    monkeypatch.setattr(pointnet2_mp, "knn_interpolate", knn_interpolate)
    for m in net.modules():
        if isinstance(m, pointnet2_mp.GlobalBaseModule):
            m.pool = max_pool


def test_fixture_replayed_on_cpu_tensors(case, oracle, monkeypatch):
    """The module logic is pinned in float64: RandLANetSeg in double on the reference's weights and draws reproduces
    the reference's float64 train-mode pass to 1e-9, and its gradients to 1e-6 relative L2 (they are stored rounded to
    float32).  The float32 eval-mode pass (no batch statistics) meets the fixture's at 1e-5 * scale.  A float32
    train-mode pass on the CPU is not compared: PyTorch's CPU BatchNorm reduces in per-thread chunks and the reference
    itself moves with the thread count (tests/test_randla_golden_cpu.py); that bar is the GPU test's."""
    name, gold = case
    draws = ru.draws_of(gold)
    net64 = ru.build_net(name, gold, "cpu", "auto", torch.float64).train()
    _host_searches(monkeypatch, oracle, net64)
    ru.replay(net64, draws, "cpu")
    data = ru.bag(gold, "cpu", torch.float64)
    x = data.x.clone().requires_grad_(True)
    data.x = x
    out = net64(data)
    want = torch.as_tensor(gold["f64/out"])
    assert float((out.detach() - want).abs().max()) < 1e-9
    (out * gold["cot"].double()).sum().backward()
    rel = float((x.grad - gold["grad64/x"].double()).norm() / gold["grad64/x"].double().norm())
    assert rel < 1e-6, rel
    checked = 0
    for pname, p in net64.named_parameters():
        if p.grad is None:  # features_downsample_nn of a residual block: evaluated, not consumed
            assert "pgrad64/" + pname not in gold, pname
            continue
        g = gold["pgrad64/" + pname].double()
        if pname.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
            continue
        if ".inner.nn." in pname:
            # one cloud: the pooled row is the same for all 16 rows it is copied to, so the train-mode BatchNorm of
            # the first FPModule removes it -- analytically zero gradient, round-off on both sides
            assert float(p.grad.norm()) < 1e-9 and float(g.norm()) < 1e-9, pname
            continue
        rel = float((p.grad - g).norm() / (g.norm() + 1e-300))
        assert rel < 1e-6, (pname, rel)
        checked += 1
    assert checked > 60
    sd = net64.state_dict()
    after = {k[len("after/"):]: v for k, v in gold.items() if k.startswith("after/")}
    assert len(after) > 60
    for k, v in after.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 1, k
        else:
            torch.testing.assert_close(sd[k].float(), v, rtol=1e-5, atol=1e-6, msg=k)
    # eval mode on the statistics the reference's step left (its float32 buffers)
    net = ru.build_net(name, gold, "cpu", "auto")
    net.load_state_dict(dict(ru.state_of(gold), **after), strict=True)
    net.eval()
    _host_searches(monkeypatch, oracle, net)
    ru.replay(net, draws, "cpu")
    with torch.no_grad():
        ev = net(ru.bag(gold, "cpu"))
    scale = float(gold["eval/out"].abs().max())
    assert float((ev - gold["eval/out"]).abs().max()) <= 1e-5 * scale


# ---------------------------------------------------------------- the folded constants of the one-kernel pass

def _edge_mlps(seed=3):
    """a RandlaKernel in eval mode with the BatchNorm buffers and affine parameters of its edge MLPs off their defaults"""
    from torch_points3d_amd.randla import RandlaKernel
    torch.manual_seed(seed)
    ker = RandlaKernel(point_pos_nn=[10, 8, 6], attention_nn=[12, 8, 12], global_nn=[12, 16]).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in _edge_bns(ker):
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
            bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.2)
    return ker


def _edge_bns(ker):
    return [layer[1].batch_norm for mlp in (ker.point_pos_nn, ker.attention_nn) for layer in mlp]


def _fresh_fold(ker):
    from torch_points3d_amd import randla
    with torch.no_grad():
        return torch.cat([t.detach().float() for mlp in (ker.point_pos_nn, ker.attention_nn) for layer in mlp
                          for t in randla._fold_layer(layer)])


def _refolded(ker, old, values_moved=True):
    """_lfa_consts hands out a new buffer that is the fold of the module's current tensors, and keeps that one"""
    from torch_points3d_amd import randla
    new = randla._lfa_consts(ker.point_pos_nn, ker.attention_nn)
    assert new is not old
    assert torch.equal(new, _fresh_fold(ker))
    assert torch.equal(new, old) != values_moved
    assert randla._lfa_consts(ker.point_pos_nn, ker.attention_nn) is new
    return new


def test_lfa_consts_follow_parameter_writes_loads_and_moves():
    from torch_points3d_amd import randla
    ker = _edge_mlps()
    old = randla._lfa_consts(ker.point_pos_nn, ker.attention_nn)
    assert torch.equal(old, _fresh_fold(ker))
    assert randla._lfa_consts(ker.point_pos_nn, ker.attention_nn) is old
    # an in-place write under no_grad, to a parameter of each kind
    for pick in (lambda k: k.point_pos_nn[0][0].weight, lambda k: k.point_pos_nn[1][0].bias,
                 lambda k: k.attention_nn[0][1].batch_norm.weight, lambda k: k.attention_nn[1][1].batch_norm.bias):
        with torch.no_grad():
            pick(ker).mul_(1.25).add_(0.125)
        old = _refolded(ker, old)
    # load_state_dict of another module's state
    ker.load_state_dict(_edge_mlps(seed=9).state_dict())
    old = _refolded(ker, old)
    # .double().float(): the values round-trip exactly, the storages are new ones (the old ones are held here, so that
    # no new storage can land on an old address)
    held = [t.data for t in list(ker.parameters()) + list(ker.buffers())]
    ker.double().float()
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(held, list(ker.parameters()) + list(ker.buffers()))
               if a.is_floating_point())
    _refolded(ker, old, values_moved=False)


@pytest.mark.parametrize("trigger", ["replay", "train_pass"])
@pytest.mark.parametrize("stat", ["running_mean", "running_var"])
@pytest.mark.parametrize("layer", range(4))
def test_lfa_consts_follow_statistics_written_behind_the_version_counters(layer, stat, trigger):
    """What the BatchNorm kernels and a replayed captured step do to the running statistics: the values change, no
    version counter moves.  The constants are refolded once the module's training-pass count or the replay count says
    so (fused.eval_state_key)."""
    from torch_points3d_amd import fused, randla
    ker = _edge_mlps()
    old = randla._lfa_consts(ker.point_pos_nn, ker.attention_nn)
    bn = _edge_bns(ker)[layer]
    buf = getattr(bn, stat)
    version = buf._version
    buf.data.mul_(1.5).add_(0.25)
    assert buf._version == version  # the write was invisible to the counter, as a raw-pointer write is
    if trigger == "replay":
        fused.note_graph_replay()
    else:
        bn._tp3d_train_passes = getattr(bn, "_tp3d_train_passes", 0) + 1
    _refolded(ker, old)
