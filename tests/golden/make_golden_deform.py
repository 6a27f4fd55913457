"""Generator of tests/golden/kpconv_deform.npz: the REFERENCE's deformable kernel-point convolution on the CPU.

Runs, on top of the CPU oracle radius search and with the stand-in modules of make_golden.py,
  * `KPConv_deform_ops` (modules/KPConv/convolution_ops.py:110-235): three influences x modulations on / off;
  * `KPConvDeformableLayer` (modules/KPConv/kernels.py:107-256): not modulated with loss_mode "fitting", modulated
    with "permissive";
  * one `KPDualBlock` (modules/KPConv/blocks.py) with deformable=[False, True]
and stores inputs, parameters, outputs, the regularisers (modules/KPConv/losses.py) and the gradients of
sum(out * cotangent) + LAMBDA * (regularisers).  Data only.

The generator re-seeds until no (query, neighbour, kernel point) pair lies within 1e-5 (relative) of
d2 == extent^2 and no d2 is 0, so the tests on the fixture exclude nothing; the offset weights are scaled so that
some deformed kernel points leave the kernel radius (the permissive loss is the mean over those, NaN without any).
The block case is also re-seeded until every LeakyReLU input is at least KINK_MARGIN away from 0: an implementation
whose forward differs in the last bits must not land on the other side of a kink, where a gradient element changes by 90 %.

    python tests/golden/make_golden_deform.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import tpk_ref  # noqa: E402

LAMBDA = 0.1
MARGIN = 1e-5
KINK_MARGIN = 5e-5


class Unsafe(Exception):
    pass


def check_margin(sq_distances, extent):
    d2 = sq_distances.detach()
    ext2 = float(extent) ** 2
    if float(((d2 - ext2).abs() / ext2).min()) < MARGIN or float(d2.min()) <= 0.0:
        raise Unsafe()


def load_reference():
    mg.install_stubs()

    class _BILM(torch.nn.Module):
        pass

    class _NoSampler(object):
        def __init__(self, *a, **k):
            raise RuntimeError("the fixture has no strided block")

    mg._stub("torch_points3d.core.data_transform", GridSampling3D=_NoSampler)
    mg._stub("torch_points3d.models.base_model", BaseInternalLossModule=_BILM)
    try:
        import matplotlib  # noqa: F401
    except Exception:
        mg._stub("matplotlib").pyplot = mg._stub("matplotlib.pyplot")
    import torch_points3d.modules.KPConv.blocks as blocks
    import torch_points3d.modules.KPConv.convolution_ops as ops
    import torch_points3d.modules.KPConv.kernels as kernels
    import torch_points3d.modules.KPConv.losses as losses
    return ops, kernels, blocks, losses


def guard_deform_ops(kernels, ops):
    """every deformable convolution a layer runs is checked for the margin"""
    def guarded(q, s, nbr, x, K, off, mod, W, extent, infl, aggr):
        out, sq, dk = ops.KPConv_deform_ops(q, s, nbr, x, K, off, mod, W, extent, infl, aggr)
        check_margin(sq, extent)
        guarded.outside.append(float((dk.detach().norm(dim=-1) > 1.5 * extent).float().mean()))
        return out, sq, dk
    guarded.outside = []
    kernels.KPConv_deform_ops = guarded
    return guarded


def op_case(ops, losses, seed):
    g = torch.Generator().manual_seed(seed)
    M, Nq, Mn, Cin, Cout, KP = 170, 120, 25, 8, 12, 15
    support = torch.rand(M, 3, generator=g)
    query = support[torch.randperm(M, generator=g)[:Nq]].contiguous()
    infl = 0.12
    kp = mg_kernel_points() * (1.5 * infl)
    idx, _ = tpk_ref.ball_query(0.36, Mn, support, query, mode="partial_dense", batch_x=torch.zeros(M, dtype=torch.long),
                                batch_y=torch.zeros(Nq, dtype=torch.long))
    assert (idx == -1).any()
    feats = torch.randn(M, Cin, generator=g)
    W = torch.randn(KP, Cin, Cout, generator=g) * 0.2
    offsets = torch.randn(Nq, KP, 3, generator=g) * (0.4 * infl)
    mods = 2 * torch.sigmoid(torch.randn(Nq, KP, generator=g))
    cot = torch.randn(Nq, Cout, generator=g)
    rec = {"op/support": support, "op/query": query, "op/neighbors": idx, "op/features": feats, "op/K_points": kp,
           "op/K_values": W, "op/offsets": offsets, "op/modulations": mods, "op/cot": cot,
           "op/extent": torch.tensor([infl]), "op/lambda": torch.tensor([LAMBDA])}
    for influence in ("constant", "linear", "gaussian"):
        for use_mod in (False, True):
            f, w, o = (t.clone().requires_grad_(True) for t in (feats, W, offsets))
            m = mods.clone().requires_grad_(True) if use_mod else None
            out, sq, dk = ops.KPConv_deform_ops(query, support, idx.clone(), f, kp, o, m, w, infl, influence, "sum")
            check_margin(sq, infl)
            fit = losses.fitting_loss(sq, 1.5 * infl)
            rep = losses.repulsion_loss(dk, infl)
            ((out * cot).sum() + LAMBDA * (fit + rep)).backward()
            tag = "op/%s_%s/" % (influence, "mod" if use_mod else "plain")
            rec.update({tag + "out": out, tag + "kp_min_d2": sq.min(dim=1)[0], tag + "fitting": fit.reshape(1),
                        tag + "repulsion": rep.reshape(1), tag + "grad_features": f.grad, tag + "grad_K_values": w.grad,
                        tag + "grad_offsets": o.grad})
            if use_mod:
                rec[tag + "grad_modulations"] = m.grad
    return rec


def mg_kernel_points():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ref_plyutils", os.path.join(mg.REF, "torch_points3d/modules/KPConv/plyutils.py"))
    ply = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ply)
    kp = ply.read_ply(os.path.join(mg.REF, "torch_points3d/modules/KPConv/kernels/dispositions/k_015_center.ply"))
    return torch.from_numpy(np.vstack((kp["x"], kp["y"], kp["z"])).T.astype(np.float32))


def scale_offsets(module, factor):
    with torch.no_grad():
        for m in module.modules():
            if hasattr(m, "offset_weights"):
                m.offset_weights.mul_(factor)
                m.offset_bias.normal_(0.0, 0.3)


def layer_case(kernels, guard, seed, modulated, loss_mode):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    M, Nq, Mn, Cin, Cout = 170, 120, 25, 4, 8
    support = torch.rand(M, 3, generator=g)
    query = support[torch.randperm(M, generator=g)[:Nq]].contiguous()
    infl = 0.1
    idx, _ = tpk_ref.ball_query(5.0 * infl * 0.7, Mn, support, query, mode="partial_dense",
                                batch_x=torch.zeros(M, dtype=torch.long), batch_y=torch.zeros(Nq, dtype=torch.long))
    assert (idx == -1).any()
    layer = kernels.KPConvDeformableLayer(Cin, Cout, infl, modulated=modulated, loss_mode=loss_mode)
    scale_offsets(layer, 6.0)
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    feats = torch.randn(M, Cin, generator=g)
    cot = torch.randn(Nq, Cout, generator=g)
    f = feats.clone().requires_grad_(True)
    guard.outside = []
    out = layer(query, support, idx.clone(), f)
    if not 0.02 < guard.outside[-1] < 0.9:
        raise Unsafe()
    il = layer.get_internal_losses()
    reg = sum(v for v in il.values() if torch.is_tensor(v))
    ((out * cot).sum() + LAMBDA * reg).backward()
    tag = "layer_%s/" % ("mod" if modulated else "plain")
    rec = {tag + "support": support, tag + "query": query, tag + "neighbors": idx, tag + "features": feats,
           tag + "cot": cot, tag + "influence": torch.tensor([infl]), tag + "out": out, tag + "grad_features": f.grad,
           tag + "outside": torch.tensor([guard.outside[-1]])}
    for k, v in il.items():
        rec[tag + "loss." + k] = torch.as_tensor(float(v.detach() if torch.is_tensor(v) else v)).reshape(1)
    for k, v in sd.items():
        rec[tag + "sd." + k] = v
    for k, p in layer.named_parameters():
        if p.grad is not None:
            rec[tag + "grad." + k] = p.grad
    return rec


def dual_case(blocks, guard, seed):
    class _Data(mg._Bag):
        def clone(self):
            out = _Data()
            for k, v in self.__dict__.items():
                setattr(out, k, v.clone() if torch.is_tensor(v) else v)
            return out

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    N, grid, f = 400, 0.06, 4
    pos = torch.rand(N, 3, generator=g) * 0.7
    batch = torch.sort(torch.randint(0, 2, (N,), generator=g))[0]
    x = torch.cat([torch.ones(N, 1), torch.randn(N, 3, generator=g)], 1)
    dual = blocks.KPDualBlock(block_names=["SimpleBlock", "ResnetBBlock"], down_conv_nn=[[4, f], [f, 2 * f]],
                              grid_size=[grid, grid], prev_grid_size=[grid, grid], has_bottleneck=[False, True],
                              max_num_neighbors=[20, 30], deformable=[False, True], module_name="KPDualBlock", index=0)
    scale_offsets(dual, 6.0)
    dual.train()
    sd = {k: v.clone() for k, v in dual.state_dict().items()}
    xin = x.clone().requires_grad_(True)
    guard.outside = []
    pre = []
    hooks = [m.register_forward_hook(lambda mod, inp, res: pre.append(float(inp[0].detach().abs().min())))
             for m in set(m for m in dual.modules() if isinstance(m, torch.nn.LeakyReLU))]
    out = dual(_Data(pos=pos, batch=batch, x=xin))
    for h in hooks:
        h.remove()
    assert len(pre) == 4  # SimpleBlock, unary_1, the deformable SimpleBlock, unary_2
    if not 0.02 < guard.outside[-1] < 0.9 or min(pre) < KINK_MARGIN:
        raise Unsafe()
    cot = torch.randn(out.x.shape, generator=g)
    deform = dual.blocks[1].kp_conv.kp_conv
    il = deform.get_internal_losses()
    reg = sum(v for v in il.values() if torch.is_tensor(v))
    ((out.x * cot).sum() + LAMBDA * reg).backward()
    rec = {"dual/pos": pos, "dual/batch": batch, "dual/x": x, "dual/grid": torch.tensor([grid]),
           "dual/width": torch.tensor([f]), "dual/out_x": out.x, "dual/idx": out.idx_neighboors, "dual/cot": cot,
           "dual/grad_x": xin.grad}
    for k, v in il.items():
        rec["dual/loss." + k] = torch.as_tensor(float(v.detach() if torch.is_tensor(v) else v)).reshape(1)
    for k, v in sd.items():
        rec["dual/sd." + k] = v
    for k, v in dual.state_dict().items():
        if "running_" in k:
            rec["dual/after." + k] = v
    for k, p in dual.named_parameters():
        if p.grad is not None:
            rec["dual/grad." + k] = p.grad
    return rec


def first_safe(make, seed):
    for s in range(seed, seed + 200):
        try:
            rec = make(s)
            print("  seed %d" % s)
            return rec
        except Unsafe:
            continue
    raise RuntimeError("no seed gives a fixture with the required margins")


def main():
    ops, kernels, blocks, losses = load_reference()
    guard = guard_deform_ops(kernels, ops)
    rec = {}
    rec.update(first_safe(lambda s: op_case(ops, losses, s), 3100))
    rec.update(first_safe(lambda s: layer_case(kernels, guard, s, False, "fitting"), 3300))
    rec.update(first_safe(lambda s: layer_case(kernels, guard, s, True, "permissive"), 3500))
    rec.update(first_safe(lambda s: dual_case(blocks, guard, s), 3700))
    path = os.path.join(HERE, "kpconv_deform.npz")
    np.savez_compressed(path, **mg.to_np(rec))
    limit = os.path.getsize(os.path.join(HERE, "kpconv_blocks.npz"))
    size = os.path.getsize(path)
    assert size <= limit and size < (1 << 20), size
    print("wrote %s (%.1f KiB, %d arrays)" % (path, size / 1024.0, len(rec)))


if __name__ == "__main__":
    main()
