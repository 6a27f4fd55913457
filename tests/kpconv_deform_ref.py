"""Plain-torch restatement of the deformable kernel-point convolution -- test infrastructure, not product code.

It states the semantics the HIP kernels implement (csrc/kpconv_deform.hip), in the dtype of its inputs, on any device:
  rel = support[nbr] - query (shadow slot: the point 1e6), dk = K_points + offsets,
  d2 = (dx*dx + dy*dy) + dz*dz, in_range = any_k d2 < extent^2, h by influence, wf = mod * sum_n in_range * h * x,
  out = wf . K_values, kp_min_d2 = min over all slots of d2.
It is pinned against the reference's own KPConv_deform_ops by tests/golden/kpconv_deform.npz
(tests/test_kpconv_deform_cpu.py) and is the yardstick of the large-shape GPU tests.

`decide_d2`: squared distances (any float dtype) that take the DISCRETE decisions (in-range mask, constant influence,
the clamp of the linear influence) instead of this evaluation's own; the float64 evaluation uses the float32 ones so that
it is the exact value of the same piecewise-smooth function the float32 implementations evaluate.
"""
import torch


def deform_d2(query, support, nbr, kpts, offsets):
    M = support.shape[0]
    sup = torch.cat([support, torch.full_like(support[:1], 1e6)], 0)
    idx = torch.where((nbr < 0) | (nbr >= M), torch.full_like(nbr, M), nbr)
    rel = sup.index_select(0, idx.reshape(-1)).view(idx.shape[0], idx.shape[1], 3) - query[:, None, :]
    dk = kpts[None] + offsets
    diff = rel[:, :, None, :] - dk[:, None, :, :]
    sq = diff * diff
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2], idx, dk


def extent_squared(extent):
    """the threshold both sides compare fp32 distances with: the double product rounded to fp32"""
    return float(torch.tensor(float(extent) ** 2, dtype=torch.float32))


def torch_kpconv_deform(query, support, nbr, feats, kpts, offsets, mods, W, extent, influence, decide_d2=None):
    """-> (out (Nq, Cout), kp_min_d2 (Nq, KP), deformed kernel points (Nq, KP, 3))"""
    d2, idx, dk = deform_d2(query, support, nbr, kpts, offsets)
    dec = d2.detach() if decide_d2 is None else decide_d2
    ext2 = extent_squared(extent)
    near = dec < ext2
    in_range = near.any(2)
    if influence == "constant":
        h = near.to(d2.dtype)
    elif influence == "linear":
        pos = d2 > 0  # the pair at distance 0: weight 1, gradient defined as 0 (the reference: NaN)
        root = torch.sqrt(torch.where(pos, d2, torch.ones_like(d2)))
        lin = 1 - root / extent
        if decide_d2 is None:
            lin = lin.clamp(min=0)
        else:
            lin = torch.where(1 - torch.sqrt(dec) / torch.tensor(extent, dtype=dec.dtype) > 0, lin, torch.zeros_like(lin))
        h = torch.where(pos, lin, torch.ones_like(d2))
    elif influence == "gaussian":
        h = torch.exp(-d2 / (2 * (extent * 0.3) ** 2 + 1e-9))
    else:
        raise ValueError(influence)
    w = h * in_range[:, :, None].to(d2.dtype)
    fx = torch.cat([feats, torch.zeros_like(feats[:1])], 0)
    nf = fx.index_select(0, idx.reshape(-1)).view(idx.shape[0], idx.shape[1], -1)
    wf = torch.einsum("qnk,qnc->qkc", w, nf)
    if mods is not None:
        wf = wf * mods[:, :, None]
    out = torch.mm(wf.reshape(wf.shape[0], -1), W.reshape(-1, W.shape[-1]))
    return out, d2.min(dim=1)[0], dk


def boundary_rows(d2, extent, ulps=4):
    """(Nq,) bool: the query has a (neighbour, kernel point) pair within `ulps` fp32 ulp of d2 == extent^2, where the
    weight (constant), the mask or the derivative (linear) jumps"""
    ext2 = extent_squared(extent)
    tol = ulps * ext2 * 2.0 ** -23
    return ((d2 - ext2).abs() <= tol).reshape(d2.shape[0], -1).any(1)
