"""PointNet's per-cloud row kernels (csrc/segment_rows.hip: torchpoints.segment_transform, segment_broadcast_cat,
segment_mean_rows) and the modules of torch_points3d_amd.pointnet on the GPU.

Operators: against the torch composition of the same call (`bmm` over `trans[batch]`, `g[batch]`, `torch.cat`, `index_add`)
evaluated in float64 on the device, by the rule of tests/test_gpu_ppnet.py's `_close64`:
    |hip - ref64| <= max(1e-5 |ref64| + 1e-5 max(1, |ref64|max), 2 |ref32 - ref64|max)
(gradients: 1e-4 |ref64| + 1e-5 |ref64|max), ref32 the same composition in float32.  The cloud sizes put seams at the
kernels' own tile edges: R = SEG_TILE_ROWS rows per workgroup of the transform, S = SEG_SUM_CHUNK rows per chunk of the
fixed-order sums.  Modules: against the reference's tensors (tests/golden/pointnet.npz) by the same rule, and against the
plain-torch composition (fused=False) on the device."""
import pytest
import torch

from conftest import load_golden
from test_pointnet_cpu import STAGES, build_features, build_seg, check_gradients, close64, config, seg_pass

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sizes():
    from torch_points3d_amd import torchpoints as tp
    R, S = tp.SEG_TILE_ROWS, tp.SEG_SUM_CHUNK
    return {"tile_seams": [1, R - 1, R, R + 1, 0, 2 * R + 3], "chunk_seams": [S - 1, S + 1, 0, 0, 2 * S],
            "single": [S + R + 1], "empty_ends": [0, R + 1, S + 2, 0]}


CLOUDS = ["tile_seams", "chunk_seams", "single", "empty_ends"]


def _clouds(name):
    sizes = torch.tensor(_sizes()[name])
    seg = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(sizes, 0)
    batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
    return seg.to(DEV), batch.to(DEV), sizes.numel(), int(seg[-1])


def _strided(t, pad):
    """the same values as rows of a wider buffer (row stride = columns + pad)"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def _transform_ref(x, T, batch, k, cot, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    T = T.to(dtype).clone().requires_grad_(True)
    out = torch.cat([torch.bmm(x[:, None, :k], T.index_select(0, batch))[:, 0], x[:, k:]], 1)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), x.grad, T.grad


def _transform_hip(hip, x, T, seg, cot):
    x = x.detach().requires_grad_(True)  # (a strided view stays one)
    T = T.clone().requires_grad_(True)
    out = hip.segment_transform(x, T, seg=seg)
    (out * cot).sum().backward()
    return out.detach(), x.grad, T.grad


@pytest.mark.parametrize("extra", [0, 3, 1])  # C = k, k + 3, k + 1 (the last breaks 16-byte row alignment)
@pytest.mark.parametrize("k", [1, 3, 5, 16, 64])
@pytest.mark.parametrize("clouds", CLOUDS)
def test_segment_transform_distance_to_float64(hip, clouds, k, extra):
    seg, batch, B, N = _clouds(clouds)
    C = k + extra
    gen = torch.Generator().manual_seed(100 * k + extra)
    x = torch.randn(N, C, generator=gen).to(DEV)
    T = (torch.randn(B, k, k, generator=gen) / k ** 0.5).to(DEV)
    cot = torch.randn(N, C, generator=gen).to(DEV)
    out32, dx32, dT32 = _transform_ref(x, T, batch, k, cot, torch.float32)
    out64, dx64, dT64 = _transform_ref(x, T, batch, k, cot, torch.float64)
    for pad in (0, 5):  # contiguous rows, and rows of a wider buffer (stride C + 5)
        xs, cs = (x, cot) if pad == 0 else (_strided(x, pad), _strided(cot, pad))
        out, dx, dT = _transform_hip(hip, xs, T, seg, cs)
        what = "%s k=%d C=%d stride=%d " % (clouds, k, C, C + pad)
        assert out.shape == (N, C) and dx.shape == (N, C) and dT.shape == (B, k, k)
        close64(out, out32, out64, 1e-5, 1e-5, 1.0, what + "out")
        close64(dx, dx32, dx64, 1e-4, 1e-5, what=what + "dx")  # (the transposed application)
        close64(dT, dT32, dT64, 1e-4, 1e-5, what=what + "dT")
        assert torch.equal(out[:, k:], x[:, k:]) and torch.equal(dx[:, k:], cot[:, k:])  # the pass-through columns
        empty = (seg[1:] == seg[:-1]).nonzero().flatten()
        assert not dT[empty].any()  # an empty cloud gives zeros
        again = _transform_hip(hip, xs, T, seg, cs)
        assert torch.equal(out, again[0]) and torch.equal(dx, again[1]) and torch.equal(dT, again[2])


@pytest.mark.parametrize("k", [1, 3, 5, 16, 64])
@pytest.mark.parametrize("clouds", CLOUDS)
def test_identity_matrices_return_the_input_exactly(hip, clouds, k):
    seg, batch, B, N = _clouds(clouds)
    x = torch.randn(N, k + 3, generator=torch.Generator().manual_seed(k)).to(DEV)
    eye = torch.eye(k, device=DEV).repeat(B, 1, 1)
    assert torch.equal(hip.segment_transform(x, eye, seg=seg), x)
    assert torch.equal(hip.segment_transform(x, eye, batch=batch) if clouds != "empty_ends" else x, x)
    assert torch.equal(hip._seg_transform(x, k + 3, eye, seg, k + 3, 1), x)  # transposed


@pytest.mark.parametrize("C2", [2, 16, 1024])
@pytest.mark.parametrize("C1", [0, 3, 64])
@pytest.mark.parametrize("clouds", CLOUDS)
def test_segment_broadcast_cat_is_exact_and_its_gradient_close_to_float64(hip, clouds, C1, C2):
    seg, batch, B, N = _clouds(clouds)
    gen = torch.Generator().manual_seed(C1 + C2)
    x = torch.randn(N, C1, generator=gen).to(DEV) if C1 else None
    g = torch.randn(B, C2, generator=gen).to(DEV)
    cot = torch.randn(N, C1 + C2, generator=gen).to(DEV)

    def run():
        xl = x.clone().requires_grad_(True) if C1 else None
        gl = g.clone().requires_grad_(True)
        out = hip.segment_broadcast_cat(xl, gl, seg=seg)
        (out * cot).sum().backward()
        return out.detach(), (xl.grad if C1 else None), gl.grad

    out, dx, dg = run()
    assert torch.equal(out, torch.cat([x, g[batch]], 1) if C1 else g[batch])
    if C1:
        assert torch.equal(dx, cot[:, :C1])
    dg32 = torch.zeros(B, C2, device=DEV).index_add(0, batch, cot[:, C1:])
    dg64 = torch.zeros(B, C2, device=DEV, dtype=torch.float64).index_add(0, batch, cot[:, C1:].double())
    close64(dg, dg32, dg64, 1e-4, 1e-5, what="%s C1=%d C2=%d dg" % (clouds, C1, C2))
    again = run()
    assert torch.equal(out, again[0]) and torch.equal(dg, again[2]) and (not C1 or torch.equal(dx, again[1]))
    if C1 and C2 == 16:  # rows of wider buffers
        out_s = hip.segment_broadcast_cat(_strided(x, 5), _strided(g, 3), seg=seg)
        assert torch.equal(out_s, out)


@pytest.mark.parametrize("C", [1, 6, 16, 1024])
@pytest.mark.parametrize("clouds", CLOUDS)
def test_segment_mean_rows_distance_to_float64(hip, clouds, C):
    seg, batch, B, N = _clouds(clouds)
    gen = torch.Generator().manual_seed(C)
    rows = torch.randn(N, C, generator=gen).to(DEV) + 0.5
    cot = torch.randn(B, C, generator=gen).to(DEV)
    counts = (seg[1:] - seg[:-1]).clamp(min=1)

    def ref(dtype):
        r = rows.to(dtype).clone().requires_grad_(True)
        out = torch.zeros(B, C, device=DEV, dtype=dtype).index_add(0, batch, r) / counts[:, None].to(dtype)
        (out * cot.to(dtype)).sum().backward()
        return out.detach(), r.grad

    def run(r):
        r = r.detach().requires_grad_(True)
        out = hip.segment_mean_rows(r, seg)
        (out * cot).sum().backward()
        return out.detach(), r.grad

    (out32, d32), (out64, d64) = ref(torch.float32), ref(torch.float64)
    for pad in (0, 5):
        r = rows if pad == 0 else _strided(rows, pad)
        out, d = run(r)
        what = "%s C=%d stride=%d " % (clouds, C, C + pad)
        close64(out, out32, out64, 1e-5, 1e-5, 1.0, what + "mean")
        close64(d, d32, d64, 1e-4, 1e-5, what=what + "d rows")
        assert not out[seg[1:] == seg[:-1]].any()
        again = run(r)
        assert torch.equal(out, again[0]) and torch.equal(d, again[1])


def test_segment_transform_never_holds_a_matrix_per_point(hip):
    """a condition, not a measurement: forward + backward at N = 4096, k = 64 raise the allocator's peak by less than a
    quarter of the (N, k, k) tensor the composition materialises; the composition raises it by more than that tensor"""
    N, k, B = 4096, 64, 4
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, k, generator=gen).to(DEV)
    T = torch.randn(B, k, k, generator=gen).to(DEV)
    cot = torch.randn(N, k, generator=gen).to(DEV)
    batch = torch.arange(B, device=DEV).repeat_interleave(N // B)
    seg = torch.arange(B + 1, device=DEV) * (N // B)
    per_point = N * k * k * 4

    def rise(fn):
        xl, Tl = x.clone().requires_grad_(True), T.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (fn(xl, Tl) * cot).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = rise(lambda a, b: hip.segment_transform(a, b, seg=seg))
    plain = rise(lambda a, b: torch.bmm(a[:, None, :], b[batch])[:, 0])
    print("peak rise: fused %.2f MiB, composition %.2f MiB, (N, k, k) fp32 = %.2f MiB" % (fused / 2 ** 20, plain / 2 ** 20,
                                                                                       per_point / 2 ** 20))
    assert fused < per_point / 4
    assert plain > per_point


def test_refusals_on_the_device(hip):
    x = torch.randn(10, 5, device=DEV)
    seg = torch.tensor([0, 4, 10], device=DEV)
    with pytest.raises(ValueError):
        hip.segment_transform(x, torch.zeros(3, 3, 3, device=DEV), seg=seg)  # three matrices for two clouds
    with pytest.raises(ValueError):
        hip.segment_transform(x, torch.zeros(2, 6, 6, device=DEV), seg=seg)  # k > C
    with pytest.raises(ValueError, match="sorted"):
        hip.segment_transform(x, torch.zeros(2, 3, 3, device=DEV), batch=torch.tensor([1] * 4 + [0] * 6, device=DEV))
    with pytest.raises(ValueError):
        hip.segment_broadcast_cat(x, torch.zeros(3, 2, device=DEV), seg=seg)


# ------------------------------------------------------------------------------------------------------------- modules
def test_fused_network_matches_reference_fixture():
    g = load_golden("pointnet")
    net = build_seg(g, fused=True).to(DEV)
    rec, x = seg_pass(net, g, DEV)
    for key in STAGES + ["trans_input", "trans_feat", "ortho_loss"]:
        close64(rec[key], g[key], g["f64/" + key], 1e-5, 1e-5, 1.0, key)
    assert check_gradients(net, g, "", x, lambda got, key: close64(got, g[key], g["f64/" + key], 1e-4, 1e-5, what=key)) > 40
    sd = net.state_dict()
    after = {k[len("after/"):]: v for k, v in g.items() if k.startswith("after/")}
    assert len(after) > 30
    for name, v in after.items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v), name
        else:
            close64(sd[name], v, g["f64/after/" + name], 1e-5, 1e-5, 1.0, "after/" + name)
    net.eval()
    with torch.no_grad():
        out = net(g["x"].to(DEV), g["batch"].to(DEV))
    close64(out, g["eval/out"], g["f64/eval/out"], 1e-5, 1e-5, 1.0, "eval/out")


def test_fused_features_model_matches_reference_fixture():
    g = load_golden("pointnet")
    net = build_features(g, fused=True).to(DEV).train()
    pos = g["x"][:, :3].to(DEV).requires_grad_(True)
    out = net(pos, g["batch"].to(DEV))
    close64(out, g["feat/out"], g["f64/feat/out"], 1e-5, 1e-5, 1.0, "feat/out")
    (out * g["cot"].to(DEV)).sum().backward()
    assert check_gradients(net, g, "feat/", pos,
                           lambda got, key: close64(got, g[key], g["f64/" + key], 1e-4, 1e-5, what=key)) > 10
    net.eval()
    with torch.no_grad():
        out = net(g["x"][:, :3].to(DEV), g["batch"].to(DEV))
    close64(out, g["feat/eval/out"], g["f64/feat/eval/out"], 1e-5, 1e-5, 1.0, "feat/eval/out")


def test_fused_network_agrees_with_the_composition_on_the_device():
    g = load_golden("pointnet")
    x, batch = g["x"].to(DEV), g["batch"].to(DEV)
    outs = []
    for fused in (True, False):
        net = build_seg(g, fused=fused).to(DEV).eval()
        with torch.no_grad():
            outs.append(net(x, batch))
    print("fused vs composition: max |diff| %.3g, |ref|max %.3g" % (float((outs[0] - outs[1]).abs().max()),
                                                                   float(outs[1].abs().max())))
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-5, atol=1e-5)


def test_dense_input_matches_the_ragged_call_on_the_same_points():
    g = load_golden("pointnet")
    net = build_seg(g, fused=True).to(DEV).eval()
    n = 64
    x = g["x"][:3 * n].to(DEV)
    batch = torch.arange(3, device=DEV).repeat_interleave(n)
    with torch.no_grad():
        dense = net(x.view(3, n, -1), None)
        ragged = net(x, batch)
    assert dense.shape == (3, n, ragged.shape[1])
    assert torch.equal(dense.reshape(3 * n, -1), ragged)
    plain = build_seg(g, fused=False).to(DEV).eval()
    with torch.no_grad():
        torch.testing.assert_close(plain(x.view(3, n, -1), None), dense, rtol=1e-5, atol=1e-5)


def test_reduced_width_pointnet_takes_optimiser_steps():
    """two steps: the first moves both zero-initialised `fc_layer`s off zero, the second then reaches every parameter of
    the two transformers' regressors.  Finite everywhere; non-zero everywhere except the Linear biases in front of a
    training-mode BatchNorm, whose gradient is zero in exact arithmetic."""
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.pointnet import IGNORE_LABEL, PointNet
    gen = torch.Generator().manual_seed(5)
    N, classes = 700, 4
    pos = torch.rand(N, 3, generator=gen).to(DEV)
    feats = torch.randn(N, 2, generator=gen).to(DEV)
    batch = torch.sort(torch.randint(0, 3, (N,), generator=gen))[0].to(DEV)
    labels = torch.randint(0, classes, (N,), generator=gen).to(DEV)
    labels[::11] = IGNORE_LABEL
    torch.manual_seed(3)
    net = PointNet(2, classes, input_stn=dict(local_nn=[16, 32], global_nn=[32, 16]), local_nn_1=[16, 16],
                   feat_stn=dict(k=16, local_nn=[16, 32], global_nn=[32, 16]), local_nn_2=[16, 64],
                   seg_nn=[80, 32, classes]).to(DEV).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    losses = []
    for step in range(2):
        opt.zero_grad()
        out = net(PDData(pos=pos, x=feats, batch=batch))
        assert out.shape == (N, classes) and bool(torch.isfinite(out).all())
        loss = net.compute_loss(labels)
        loss.backward()
        losses.append(float(loss))
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            if "fc_layer" in name or (step == 1 and not name.endswith(".0.bias")):
                assert float(p.grad.abs().max()) > 0.0, (step, name)
        opt.step()
    assert all(l == l and abs(l) < 1e4 for l in losses)
    assert float(net.loss_internal) > 0.0  # the feature transform has left the identity
