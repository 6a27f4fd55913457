"""tests/fp64_kernels.py (the kernels namespace of the float64 network references) against the CPU oracle: run in float32
it is the oracle's network -- the same indices, outputs within 1e-6 of the scale -- so a float64 run of it differs from
the oracle's fp32 pass only by the arithmetic's precision."""
import torch

import fp64_kernels
from oracle import tpk_ref
from torch_points3d_amd.dense import Data
from torch_points3d_amd.pointnet2 import PointNet2Unet
from golden_util import SMALL_SSG


def _cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, 3, generator=g) * 2 - 1, torch.randn(B, N, 4, generator=g)


def test_indices_equal_the_oracles():
    fp64_kernels.limit_threads()
    pos, _ = _cloud(2, 600, 3)
    fps = fp64_kernels.furthest_point_sample(pos.double(), 100)
    assert torch.equal(fps, tpk_ref.furthest_point_sample(pos, 100))
    new = pos.gather(1, fps.long().unsqueeze(-1).expand(2, 100, 3)).contiguous()
    idx, _ = fp64_kernels.ball_query(0.3, 24, pos.double(), new.double())
    assert torch.equal(idx, tpk_ref.ball_query(0.3, 24, pos, new)[0])
    d64, i64 = fp64_kernels.three_nn(pos.double(), new.double())
    d32, i32 = tpk_ref.three_nn(pos, new)
    assert torch.equal(i64, i32) and d64.dtype == torch.float64
    torch.testing.assert_close(d64.float(), d32, rtol=1e-6, atol=1e-7)
    f = torch.randn(2, 5, 100, dtype=torch.float64)
    w = torch.rand(2, 600, 3, dtype=torch.float64)
    want = (tpk_ref.grouping_operation(f.float(), i32) * w.float().unsqueeze(1)).sum(-1)
    torch.testing.assert_close(fp64_kernels.three_interpolate(f, i32, w).float(), want, rtol=1e-6, atol=1e-6)
    f = torch.randn(2, 5, 600, dtype=torch.float64)
    torch.testing.assert_close(fp64_kernels.grouping_operation(f, idx).float(), tpk_ref.grouping_operation(f.float(), idx))


def test_float32_network_matches_the_oracle_network():
    """train mode, forward and backward: stage by stage the oracle's network within 1e-6 of the scale"""
    fp64_kernels.limit_threads()
    pos, x = _cloud(2, 700, 5)
    nets = {}
    for name, k in (("oracle", tpk_ref), ("helper", fp64_kernels)):
        torch.manual_seed(0)
        nets[name] = PointNet2Unet(4, output_nc=6, config=SMALL_SSG, kernels=k, fused=False).train()
    nets["helper"].load_state_dict(nets["oracle"].state_dict())
    outs, grads = {}, {}
    for name, net in nets.items():
        xi = x.clone().requires_grad_(True)
        rec = {}
        hooks = [m.register_forward_hook(lambda mod, i, o, j=j: rec.update({"down%d" % j: o.x, "pos%d" % j: o.pos}))
                 for j, m in enumerate(net.down_modules)]
        out = net(Data(pos=pos, x=xi)).x
        for h in hooks:
            h.remove()
        rec["out"] = out
        (out * torch.linspace(-1, 1, out.numel()).view_as(out)).sum().backward()
        outs[name] = rec
        grads[name] = dict([("x", xi.grad)] + [(k, p.grad) for k, p in net.named_parameters()])
    for k, want in outs["oracle"].items():
        got = outs["helper"][k]
        if k.startswith("pos"):
            assert torch.equal(got, want), k
            continue
        scale = max(1.0, float(want.detach().abs().max()))
        assert float((got - want).abs().max()) <= 1e-6 * scale, (k, float((got - want).abs().max()), scale)
    want = grads["oracle"]
    for k, a in grads["helper"].items():
        # a BatchNorm bias gradient is a sum with cancellation (in front of the global max-pool it is ~1e-5 of its
        # layer's weight gradient): compared on the scale of that weight gradient
        ref = float(want[k].norm())
        if k.endswith(".bias") and k[:-4] + "weight" in want:
            ref = max(ref, float(want[k[:-4] + "weight"].norm()))
        assert float((a - want[k]).norm()) <= 1e-5 * ref, k  # measured <= 2e-6 (gather vs. scatter summation order)


def test_float64_network_runs_in_double():
    fp64_kernels.limit_threads()
    pos, x = _cloud(1, 400, 7)
    torch.manual_seed(0)
    net = PointNet2Unet(4, output_nc=6, config=SMALL_SSG, kernels=fp64_kernels, fused=False).double().train()
    out = net(Data(pos=pos.double(), x=x.double())).x
    assert out.dtype == torch.float64 and out.shape == (1, 6, 400) and bool(torch.isfinite(out).all())
