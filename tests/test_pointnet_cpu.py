"""torch_points3d_amd.pointnet without a GPU: the plain-torch composition (fused=False) against the reference's own
tensors (tests/golden/pointnet.npz, written by tests/golden/make_golden_pointnet.py), the state_dict layout, the
identity at initialisation, and the refusals of the fused operators.

Bars: stages rtol = atol = 1e-5; gradients rtol 1e-4, atol 1e-5 * |ref|max.  A bias whose gradient is zero in exact
arithmetic -- a Linear bias in front of a training-mode BatchNorm, or the BatchNorm bias in front of a pool whose
per-channel constant the next training-mode BatchNorm removes -- holds only rounding noise in every evaluation; it is
recognised by its float64 reference (norm below 1e-9 of its weight's gradient) and checked as
|grad| < 1e-4 * |weight gradient| + 1e-6, the rule of tests/test_gpu_pointnet2_mp.py."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden

STAGES = ["x_input_stn", "x_local_nn_1", "x_feat_stn", "x_local_nn_2", "global_feature", "out"]


def config():
    with open(os.path.join(GOLDEN, "pointnet_config.json")) as f:
        return json.load(f)


def build_seg(g, fused, dtype=torch.float32):
    from torch_points3d_amd.pointnet import PointNetSeg
    net = PointNetSeg(fused=fused, **config()["widths"])
    net.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("w/")}, strict=True)
    return net.to(dtype)


def build_features(g, fused):
    from torch_points3d_amd.pointnet import SegPointNetModel
    cfg = config()["features"]
    net = SegPointNetModel(cfg["pointnet"], cfg["seg_nn"], fused=fused)
    net.load_state_dict({k[len("feat/w/"):]: v for k, v in g.items() if k.startswith("feat/w/")}, strict=True)
    return net


def seg_pass(net, g, dev="cpu", dtype=torch.float32):
    """the fixture's training pass: (record of stages, x with its gradient)"""
    x = g["x"].to(dev, dtype).clone().requires_grad_(True)
    rec = {}
    net.train()
    out = net(x, g["batch"].to(dev), record=rec)
    rec["trans_input"], rec["trans_feat"] = net.input_stn.trans, net.feat_stn.trans
    rec["ortho_loss"] = net.feat_stn.get_orthogonal_regularization_loss()
    ((out * g["cot"].to(dev, dtype)).sum() + config()["ortho_weight"] * rec["ortho_loss"]).backward()
    return rec, x


def is_zero_gradient(g, prefix, name):
    """analytically zero bias gradients, recognised by the float64 reference (module docstring)"""
    if not name.endswith("bias"):
        return False
    w = g.get("f64/" + prefix + "grad/" + name[:-4] + "weight")
    return w is not None and float(abs(g["f64/" + prefix + "grad/" + name]).max()) < 1e-9 * float((w ** 2).sum() ** 0.5)


def check_gradients(net, g, prefix, x, close):
    checked = 0
    for name, p in list(net.named_parameters()) + [("", x)]:
        key = prefix + ("grad/" + name if name else "grad_x")
        if name and is_zero_gradient(g, prefix, name):
            wn = float(g[prefix + "grad/" + name[:-4] + "weight"].norm())
            assert float(p.grad.norm()) < 1e-4 * wn + 1e-6, name
            continue
        close(p.grad, key)
        checked += 1
    return checked


def _close(g, got, key, rtol, atol_scale, floor=0.0):
    ref = torch.as_tensor(g[key])
    torch.testing.assert_close(got.detach().cpu(), ref, rtol=rtol, atol=atol_scale * max(floor, float(ref.abs().max())),
                               msg=lambda m: key + ": " + m)


def test_composition_stages_match_reference_fixture():
    g = load_golden("pointnet")
    net = build_seg(g, fused=False)
    rec, _ = seg_pass(net, g)
    for key in STAGES + ["trans_input", "trans_feat", "ortho_loss"]:
        _close(g, rec[key], key, 1e-5, 1e-5, 1.0)


def close64(got, ref32, ref64, rtol, atol_scale, floor=0.0, what=""):
    """`_close64` of tests/test_gpu_ppnet.py: |got - ref64| <= max(atol + rtol |ref64|, 2 |ref32 - ref64|max), element-wise"""
    ref64 = torch.as_tensor(ref64).to(got.device).double()
    ref32 = torch.as_tensor(ref32).to(got.device).double()
    if ref64.numel() == 0:
        return
    err = (got.detach().double() - ref64).abs()
    own = float((ref32 - ref64).abs().max())
    bar = atol_scale * max(floor, float(ref64.abs().max())) + rtol * ref64.abs()
    print("%s: |got - ref64|max %.3g, |ref32 - ref64|max %.3g, |ref|max %.3g" % (what, float(err.max()), own,
                                                                                float(ref64.abs().max())))
    worst = float((err - torch.clamp(bar, min=2.0 * own)).max())
    assert worst <= 0.0, "%s: |got - ref64| exceeds max(bar, 2 |ref32 - ref64|max = %.3g) by %.3g" % (what, 2.0 * own, worst)


def test_composition_gradients_in_float64_match_reference_fixture():
    """The gradient bars (rtol 1e-4, atol 1e-5 |ref|max) against the reference's float64 pass, the composition evaluated
    in float64 as well.  In float32 the three-row training-mode BatchNorms of both `global_nn`s amplify the order in
    which two correct evaluations add their terms: the composition and the reference's float32 pass, the same torch
    operators on the same CPU, differ beyond the bar in a few entries of d input_stn.nn._global_nn.0.0.weight (|ref|max 63:
    the bar allows 6.3e-4 + 1e-4 |ref|), and the reference's float32 pass is itself 3.4e-3 from its float64 pass there
    (1.7e-2 at |ref|max 422 for the feature transformer's) -- the float32 test below measures against float64 for that reason."""
    g = load_golden("pointnet")
    net = build_seg(g, fused=False, dtype=torch.float64)
    rec, x = seg_pass(net, g, dtype=torch.float64)
    for key in STAGES + ["trans_input", "trans_feat", "ortho_loss"]:
        _close(g, rec[key], "f64/" + key, 1e-5, 1e-5, 1.0)
    assert check_gradients(net, g, "", x, lambda got, key: _close(g, got, "f64/" + key, 1e-4, 1e-5)) > 40


def test_composition_gradients_buffers_and_eval_match_reference_fixture():
    """float32: gradients by the float64 rule of tests/test_gpu_ppnet.py (within the bar of the float64 pass, or within
    twice the reference's own float32 distance to it); buffers and eval-mode scores at 1e-5"""
    g = load_golden("pointnet")
    net = build_seg(g, fused=False)
    _, x = seg_pass(net, g)
    assert check_gradients(net, g, "", x, lambda got, key: close64(got, g[key], g["f64/" + key], 1e-4, 1e-5, what=key)) > 40
    sd = net.state_dict()
    after = {k[len("after/"):]: v for k, v in g.items() if k.startswith("after/")}
    assert len(after) > 30
    for name, v in after.items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v), name
        else:
            _close(g, sd[name], "after/" + name, 1e-5, 1e-5, 1.0)
    net.eval()
    with torch.no_grad():
        _close(g, net(g["x"], g["batch"]), "eval/out", 1e-5, 1e-5, 1.0)


def test_features_model_matches_reference_fixture():
    g = load_golden("pointnet")
    net64 = build_features(g, fused=False).double().train()
    pos = g["x"][:, :3].double().requires_grad_(True)
    out = net64(pos, g["batch"])
    _close(g, out, "f64/feat/out", 1e-5, 1e-5, 1.0)
    (out * g["cot"].double()).sum().backward()
    assert check_gradients(net64, g, "feat/", pos, lambda got, key: _close(g, got, "f64/" + key, 1e-4, 1e-5)) > 10
    net = build_features(g, fused=False).train()
    pos = g["x"][:, :3].clone().requires_grad_(True)
    out = net(pos, g["batch"])
    _close(g, out, "feat/out", 1e-5, 1e-5, 1.0)
    (out * g["cot"]).sum().backward()
    assert check_gradients(net, g, "feat/", pos,
                           lambda got, key: close64(got, g[key], g["f64/" + key], 1e-4, 1e-5, what=key)) > 10
    net.eval()
    with torch.no_grad():
        _close(g, net(g["x"][:, :3], g["batch"]), "feat/eval/out", 1e-5, 1e-5, 1.0)
    labels = torch.arange(out.shape[0]) % out.shape[1]
    assert torch.equal(net.compute_loss(labels), torch.nn.functional.nll_loss(net.output, labels))


def test_state_dict_keys_are_the_reference_s():
    from torch_points3d_amd.pointnet import PointNet, PointNetSeg
    keys = config()["published_state_dict_keys"]
    assert len(keys) > 100
    assert list(PointNetSeg().state_dict().keys()) == keys
    net = PointNet(1, 4)  # FEAT = 1 -> input_nc = 4 columns, N_CLS = 4: the widths the reference's defaults spell out
    assert list(net.state_dict().keys()) == ["pointnet_seg." + k for k in keys]
    assert net.pointnet_seg.seg_nn[0][0].in_features == 1088 and net.pointnet_seg.input_stn.nn._local_nn[0][0].in_features == 4


def test_identity_at_initialisation_returns_the_input_exactly():
    from torch_points3d_amd.pointnet import PointNetSTN3D, PointNetSTNkD
    gen = torch.Generator().manual_seed(0)
    batch = torch.tensor([0] * 5 + [1] * 9 + [3] * 4)  # (cloud 2 is empty)
    for stn, C in ((PointNetSTN3D([6, 8, 16], [16, 8], fused=False), 6), (PointNetSTNkD(8, [8, 16], [16, 8], fused=False), 8)):
        x = torch.randn(18, C, generator=gen)
        assert not stn.fc_layer.weight.detach().any() and not stn.fc_layer.bias.detach().any()
        assert torch.equal(stn.train()(x, batch), x)
        assert stn.trans.shape == (4, stn.k, stn.k) and "identity" not in stn.state_dict()
    assert float(stn.get_internal_losses()["orthogonal_regularization_loss"]) == 0.0


def test_dense_layout_of_the_composition_matches_the_ragged_one():
    g = load_golden("pointnet")
    net = build_seg(g, fused=False).eval()
    x = g["x"][:3 * 64].reshape(3, 64, -1)
    batch = torch.arange(3).repeat_interleave(64)
    with torch.no_grad():
        dense = net(x, None)
        ragged = net(x.reshape(3 * 64, -1), batch)
    torch.testing.assert_close(dense.reshape(3 * 64, -1), ragged, rtol=1e-5, atol=1e-5)


def test_pointnet_model_loss_and_internal_loss():
    from torch_points3d_amd.kpconv_losses import collect_internal_losses
    from torch_points3d_amd.pointnet import IGNORE_LABEL, PointNet

    class Bag(object):
        pass

    torch.manual_seed(0)
    net = PointNet(2, 4, fused=False, input_stn=dict(local_nn=[8, 16], global_nn=[16, 8]), local_nn_1=[8, 8],
                   feat_stn=dict(k=8, local_nn=[8, 16], global_nn=[16, 8]), local_nn_2=[8, 16], seg_nn=[24, 8, 4])
    torch.nn.init.normal_(net.pointnet_seg.feat_stn.fc_layer.weight, std=0.1)
    data = Bag()
    data.pos, data.x, data.batch = torch.rand(30, 3), torch.randn(30, 2), torch.arange(3).repeat_interleave(10)
    out = net(data)
    assert out.shape == (30, 4) and list(collect_internal_losses(net)) == ["pointnet_seg.feat_stn.orthogonal_regularization_loss"]
    labels = torch.arange(30) % 4
    labels[::7] = IGNORE_LABEL
    loss = net.compute_loss(labels)
    ortho = net.pointnet_seg.feat_stn.get_orthogonal_regularization_loss()
    assert float(ortho) > 0.0
    want = torch.nn.functional.cross_entropy(out, labels, ignore_index=IGNORE_LABEL) + 0.001 * ortho
    torch.testing.assert_close(loss, want)
    loss.backward()
    assert float(net.pointnet_seg.feat_stn.fc_layer.weight.grad.abs().max()) > 0.0


def test_k_above_64_and_unsorted_batch_raise():
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.pointnet import PointNetSeg, PointNetSTNkD
    x = torch.randn(12, 65)
    batch = torch.arange(2).repeat_interleave(6)
    with pytest.raises(NotImplementedError, match="64"):
        tp.segment_transform(x, torch.zeros(2, 65, 65), batch=batch)
    with pytest.raises(NotImplementedError, match="64"):
        PointNetSTNkD(65, [65, 8], [8, 8], fused=True)(x, batch)
    assert PointNetSTNkD(65, [65, 8], [8, 8], fused=False)(x, batch).shape == x.shape  # the composition has no limit
    net = PointNetSeg(input_nc=4, input_stn_local_nn=[8], input_stn_global_nn=[8, 8], local_nn_1=[8], feat_stn_k=8,
                      feat_stn_local_nn=[8, 8], feat_stn_global_nn=[8, 8], local_nn_2=[8, 8], seg_nn=[16, 4], fused=False)
    unsorted = torch.tensor([0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="sorted"):
        net(torch.randn(12, 4), unsorted)


def test_cpu_tensors_are_refused_by_the_operators():
    from torch_points3d_amd import torchpoints as tp
    seg = torch.tensor([0, 4, 10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.segment_transform(torch.randn(10, 5), torch.randn(2, 3, 3), seg=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.segment_broadcast_cat(torch.randn(10, 5), torch.randn(2, 3), seg=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.segment_broadcast_cat(None, torch.randn(2, 3), seg=seg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.segment_mean_rows(torch.randn(10, 5), seg)


def test_tiling_constants_are_the_library_s():
    from torch_points3d_amd import _lib, torchpoints as tp
    h = _lib.load()
    assert h.tp3d_segment_tile_rows() == tp.SEG_TILE_ROWS and h.tp3d_segment_sum_chunk() == tp.SEG_SUM_CHUNK
    # the slices of the fixed-order sums: N / chunk + B of them, k * k (or C) floats each
    assert h.tp3d_segment_transform_wgrad_workspace_bytes(4096, 3, 64) == (4096 // tp.SEG_SUM_CHUNK + 3) * 64 * 64 * 4
    assert h.tp3d_segment_sum_workspace_bytes(1000, 5, 7) == (1000 // tp.SEG_SUM_CHUNK + 5) * 7 * 4
