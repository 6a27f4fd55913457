"""KPConv rigid kernel-point convolution on MI355X.

Mirrors `KPConv_ops` (torch_points3d/modules/KPConv/convolution_ops.py:19-107) and `KPConvLayer`
(modules/KPConv/kernels.py:20-104): same arguments, same shadow-neighbour convention (-1 -> zero feature), same
influence / aggregation modes, same parameter names (`K_points`, `weight`).  Stage 1 (kernel-point weighted
neighbourhood features) and its backward are HIP kernels (csrc/kpconv.hip; the inverted neighbour table the backward
sums through is csrc/inverse_table.hip, the sum itself csrc/run_sum.hip); stage 2 is the single
(Nq, KP*Cin) x (KP*Cin, Cout) GEMM the reference's permute/matmul/sum amounts to; the kernel-weight gradient runs
on the split-K MFMA kernel (csrc/gemm_tn.hip).  Differentiable wrt `features` and `K_values` (what the reference
trains); positions and kernel points carry no gradient (kernels.py:57-59 sets requires_grad=False on K_points).

The deformable convolution (`KPConv_deform_ops`, convolution_ops.py:110-235; `KPConvDeformableLayer`,
kernels.py:107-256) runs on csrc/kpconv_deform.hip: per-query kernel points, in-range mask, modulations and the
fitting-loss distances in the forward kernel; gradients wrt features, offsets and modulations in one backward kernel.
The per-query device code, the argument checks and the kernel routing the two share are in csrc/kp_common.h; here they
share the device check, the buffers of the features gradient and the layers' base class.
"""
import contextlib

import torch
import torch.nn as nn

from . import _lib
from .fused import gemm_tn

_INFLUENCE = {"constant": 0, "linear": 1, "gaussian": 2}


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("torch_points3d_amd runs on MI355X only: got a %s tensor (no CPU fallback is provided)"
                               % t.device.type)


@contextlib.contextmanager
def _features_grad(nbr, M, Cin, dev, wanted=True):
    """What the gradient wrt the features needs around the backward call: yields `(dx, tail)`, the (M, Cin) result and the
    trailing `inverse, inverse_bytes, inverse_ready, workspace, workspace_bytes` arguments of the entry point (the
    inverse of the neighbour table and the `kpconv_bwd` scratch of per-slot gradient rows); on leaving the block the
    inverse the call has built is published.  `wanted=False`: no features gradient, all of it null."""
    if not wanted:
        yield None, (None, 0, 0, None, 0)
        return
    dx = torch.empty((M, Cin), dtype=torch.float32, device=dev)
    nbytes = _lib.load().tp3d_kpconv_grad_workspace_bytes(M, nbr.numel(), Cin)
    ws = _lib.workspace("kpconv_bwd", nbytes, dev)
    inv, inv_bytes, ready, token = _lib.neighbour_inverse(nbr, M, dev)
    yield dx, (_lib.ptr(inv), inv_bytes, ready, _lib.ptr(ws), nbytes)
    _lib.inverse_built(token, dev)


class _KPConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, K_values, query, support, nbr, kp, extent, influence, closest):
        dev = query.device
        x = features.detach().float().contiguous()
        W = K_values.detach().float().contiguous()
        Nq, Mn = nbr.shape
        M, Cin = x.shape
        KP = kp.shape[0]
        wf = torch.empty((Nq, KP * Cin), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.call("tp3d_kpconv_weighted_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(x),
                      _lib.ptr(kp), Nq, M, Mn, Cin, KP, float(extent), influence, closest, _lib.ptr(wf),
                      _lib.stream_ptr(dev))
        out = torch.mm(wf, W.reshape(KP * Cin, -1))  # the dense contraction: a plain library GEMM
        ctx.save_for_backward(query, support, nbr, kp, W, wf)
        ctx.cfg = (float(extent), influence, closest, M, Cin, KP, tuple(K_values.shape))
        return out

    @staticmethod
    def backward(ctx, d_out):
        query, support, nbr, kp, W, wf = ctx.saved_tensors
        extent, influence, closest, M, Cin, KP, wshape = ctx.cfg
        dev = d_out.device
        d_out = d_out.float().contiguous()
        Nq, Mn = nbr.shape
        dW = gemm_tn(wf, d_out).reshape(wshape) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            d_wf = torch.mm(d_out, W.reshape(KP * Cin, -1).t())  # (Nq, KP*Cin)
            with _lib.on_device(dev), _features_grad(nbr, M, Cin, dev) as (dx, tail):
                _lib.call("tp3d_kpconv_bwd_features_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(kp),
                          _lib.ptr(d_wf), Nq, M, Mn, Cin, KP, extent, influence, closest, _lib.ptr(dx), *tail,
                          _lib.stream_ptr(dev))
        return dx, dW, None, None, None, None, None, None, None


def KPConv_ops(query_points, support_points, neighbors_indices, features, K_points, K_values, KP_extent,
               KP_influence, aggregation_mode):
    if KP_influence not in _INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation_mode not in ("sum", "closest"):
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    _require_gpu(query_points, support_points, neighbors_indices, features, K_points, K_values)
    q = query_points.detach().float().contiguous()
    s = support_points.detach().float().contiguous()
    nbr = neighbors_indices.long().contiguous()
    kp = K_points.detach().float().contiguous()
    return _KPConv.apply(features, K_values, q, s, nbr, kp, float(KP_extent), _INFLUENCE[KP_influence],
                         int(aggregation_mode == "closest"))


class _KPConvDeform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, K_values, offsets, modulations, query, support, nbr, kp, extent, influence):
        dev = query.device
        x = features.detach().float().contiguous()
        W = K_values.detach().float().contiguous()
        off = offsets.detach().float().contiguous()
        mod = None if modulations is None else modulations.detach().float().contiguous()
        Nq, Mn = nbr.shape
        M, Cin = x.shape
        KP = kp.shape[0]
        wf = torch.empty((Nq, KP * Cin), dtype=torch.float32, device=dev)
        kp_min = torch.empty((Nq, KP), dtype=torch.float32, device=dev)
        kp_arg = torch.empty((Nq, KP), dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            _lib.call("tp3d_kpconv_deform_weighted_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(x),
                      _lib.ptr(kp), _lib.ptr(off), _lib.ptr(mod), Nq, M, Mn, Cin, KP, float(extent), influence,
                      _lib.ptr(wf), _lib.ptr(kp_min), _lib.ptr(kp_arg), _lib.stream_ptr(dev))
        out = torch.mm(wf, W.reshape(KP * Cin, -1))
        ctx.save_for_backward(query, support, nbr, kp, x, W, off, mod, wf, kp_arg)
        ctx.cfg = (float(extent), influence, M, Cin, KP, tuple(K_values.shape))
        return out, kp_min

    @staticmethod
    def backward(ctx, d_out, d_kp_min):
        query, support, nbr, kp, x, W, off, mod, wf, kp_arg = ctx.saved_tensors
        extent, influence, M, Cin, KP, wshape = ctx.cfg
        dev = d_out.device
        d_out = d_out.float().contiguous()
        Nq, Mn = nbr.shape
        need = ctx.needs_input_grad
        dW = gemm_tn(wf, d_out).reshape(wshape) if need[1] else None
        dx = d_off = d_mod = None
        if need[0] or need[2] or need[3]:
            d_wf = torch.mm(d_out, W.reshape(KP * Cin, -1).t())  # (Nq, KP*Cin)
            d_kp_min = None if d_kp_min is None else d_kp_min.float().contiguous()
            d_off = torch.empty((Nq, KP, 3), dtype=torch.float32, device=dev)
            d_mod = torch.empty((Nq, KP), dtype=torch.float32, device=dev) if mod is not None else None
            with _lib.on_device(dev), _features_grad(nbr, M, Cin, dev, need[0]) as (dx, tail):
                _lib.call("tp3d_kpconv_deform_bwd_f32", _lib.ptr(query), _lib.ptr(support), _lib.ptr(nbr), _lib.ptr(x),
                          _lib.ptr(kp), _lib.ptr(off), _lib.ptr(mod), _lib.ptr(d_wf), _lib.ptr(d_kp_min), _lib.ptr(kp_arg),
                          Nq, M, Mn, Cin, KP, extent, influence, _lib.ptr(dx), _lib.ptr(d_off), _lib.ptr(d_mod), *tail,
                          _lib.stream_ptr(dev))
            if not need[2]:
                d_off = None
            if not need[3]:
                d_mod = None
        return dx, dW, d_off, d_mod, None, None, None, None, None, None


def KPConv_deform_ops(query_points, support_points, neighbors_indices, features, K_points, offsets, modulations, K_values,
                      KP_extent, KP_influence, aggregation_mode):
    """Deformable kernel-point convolution with the reference's argument list (convolution_ops.py:110-235):
    offsets (Nq, KP, 3) move the kernel points of every query, a neighbour in range (`KP_extent`) of no deformed kernel
    point contributes nothing, `modulations` (Nq, KP) or None scale the weighted features.

    Returns `(features (Nq, Cout), kp_min_d2 (Nq, KP), deformed_K_points (Nq, KP, 3))`.  ONE deviation from the
    reference's triple: its second item is the whole (Nq, Mn, KP) tensor of squared distances, whose only consumer is
    `fitting_loss`, which takes the minimum over the neighbours first (losses.py:12); here that minimum (over all Mn
    slots, a shadow neighbour being the point (1e6, 1e6, 1e6)) is what the kernel returns, and
    `kpconv_losses.fitting_loss` accepts either form.

    Differentiable wrt `features`, `K_values`, `offsets` and `modulations`; a gradient arriving on `kp_min_d2` flows to
    `offsets` through the arg-min slot, one arriving on `deformed_K_points` through the plain addition.  No gradient
    through the in-range mask, the positions or `K_points`.  With linear influence the reference yields NaN for a
    pair at distance exactly 0 (backward of sqrt at 0 times 0); that term is defined as 0 here.
    `aggregation_mode="closest"` is not a valid call in the reference either (its argmin raises TypeError)."""
    if KP_influence not in _INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation_mode == "closest":
        raise NotImplementedError("KPConv_deform_ops: aggregation_mode='closest' is not defined for the deformable "
                                  "convolution (the reference raises on it as well); use 'sum'")
    if aggregation_mode != "sum":
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    _require_gpu(query_points, support_points, neighbors_indices, features, K_points, offsets, K_values, modulations)
    if support_points.shape[0] == 0 or neighbors_indices.shape[1] == 0:
        raise ValueError("KPConv_deform_ops needs at least one support point and one neighbour slot")
    q = query_points.detach().float().contiguous()
    s = support_points.detach().float().contiguous()
    nbr = neighbors_indices.long().contiguous()
    kp = K_points.detach().float().contiguous()
    out, kp_min_d2 = _KPConvDeform.apply(features, K_values, offsets, modulations, q, s, nbr, kp, float(KP_extent),
                                         _INFLUENCE[KP_influence])
    return out, kp_min_d2, offsets + kp


def default_kernel_points(num_points=15, iterations=400):
    """A kernel-point disposition in unit scale: one point at the centre, the others spread over the unit sphere by
    electrostatic repulsion from a Fibonacci lattice (deterministic).

    The reference loads a pre-optimised disposition from a data file (modules/KPConv/kernels/dispositions/*.ply via
    kernel_utils.load_kernels, kernels.py:51-56) and applies a random rotation; the file is not shipped with this
    build.  Any well-spread disposition is a valid initialisation, and a reference checkpoint's `K_points` replaces
    it on load_state_dict."""
    import numpy as np
    n = num_points - 1
    i = np.arange(n) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / n)
    theta = np.pi * (1.0 + 5.0 ** 0.5) * i
    p = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    for _ in range(iterations):
        d = p[:, None, :] - p[None, :, :]
        r2 = (d * d).sum(-1) + np.eye(n)
        f = (d / r2[..., None] ** 1.5).sum(1)
        p = p + 0.05 * f
        p /= np.linalg.norm(p, axis=1, keepdims=True)
    return torch.from_numpy(np.concatenate([np.zeros((1, 3)), p], axis=0).astype(np.float32))


class _KPConvBase(nn.Module):
    """What the rigid and the deformable layer share: the reference's constructor fields, the frozen `K_points`, the
    xavier-normal (KP, Cin, .) parameters and the `add_one` column of ones."""

    _INFLUENCE_TO_RADIUS = 1.5

    def __init__(self, num_inputs, num_outputs, point_influence, K_points, KP_influence, aggregation_mode, add_one):
        super().__init__()
        self.kernel_radius = self._INFLUENCE_TO_RADIUS * point_influence
        self.point_influence = point_influence
        self.add_one = add_one
        self.num_inputs = num_inputs + int(add_one)
        self.num_outputs = num_outputs
        self.KP_influence = KP_influence
        self.aggregation_mode = aggregation_mode
        K_points = torch.as_tensor(K_points, dtype=torch.float32)
        self.n_kernel_points = K_points.shape[0]
        self.K_points = nn.Parameter(K_points.clone(), requires_grad=False)

    def _xavier(self, width):
        w = torch.empty([self.n_kernel_points, self.num_inputs, width], dtype=torch.float32)
        nn.init.xavier_normal_(w)
        return nn.Parameter(w)

    def _features(self, support_points, x):
        if self.add_one:
            ones = torch.ones(support_points.shape[0], 1, dtype=torch.float32, device=support_points.device)
            x = ones if x is None else torch.cat([ones, x.float()], dim=-1)
        return x


class KPConvLayer(_KPConvBase):
    """Kernel-point convolution layer with the reference's parameters (`K_points` frozen, `weight` (KP, Cin, Cout)
    xavier-normal) and forward signature (modules/KPConv/kernels.py:20-104).  The kernel-point disposition file of the
    reference is not shipped here: pass `K_points` (KP, 3), e.g. taken from a reference checkpoint or generated by
    the reference's `load_kernels`."""

    def __init__(self, num_inputs, num_outputs, point_influence, K_points, KP_influence="linear",
                 aggregation_mode="sum", add_one=False, **kwargs):
        # **kwargs: n_kernel_points / fixed / dimension of the reference's YAML are implied by K_points here
        super().__init__(num_inputs, num_outputs, point_influence, K_points, KP_influence, aggregation_mode, add_one)
        self.weight = self._xavier(num_outputs)

    def forward(self, query_points, support_points, neighbors, x):
        x = self._features(support_points, x)
        return KPConv_ops(query_points, support_points, neighbors, x, self.K_points, self.weight, self.point_influence,
                          self.KP_influence, self.aggregation_mode)


class KPConvDeformableLayer(_KPConvBase):
    """Deformable kernel-point convolution layer with the reference's parameters and forward
    (modules/KPConv/kernels.py:107-256): `K_points` frozen, `offset_weights` (KP, Cin, 3 KP or 4 KP when `modulated`)
    xavier-normal, `offset_bias` zeros, `weight` (KP, Cin, Cout).  A rigid convolution with `offset_weights` predicts
    per-query offsets (in units of `point_influence`) and, when `modulated`, 2 * sigmoid modulations; the deformable
    convolution then runs with them.  The regularisers of the pass are left in `internal_losses`
    (`get_internal_losses()`): fitting + repulsion with `loss_mode="fitting"`, permissive with "permissive".
    `K_points` (KP, 3) is passed in, as for `KPConvLayer`."""

    PERMISSIVE_LOSS_KEY = "permissive_loss"
    FITTING_LOSS_KEY = "fitting_loss"
    REPULSION_LOSS_KEY = "repulsion_loss"

    def __init__(self, num_inputs, num_outputs, point_influence, K_points, KP_influence="linear", aggregation_mode="sum",
                 modulated=False, loss_mode="fitting", add_one=False, **kwargs):
        # **kwargs: n_kernel_points / fixed / dimension of the reference's YAML are implied by K_points here
        super().__init__(num_inputs, num_outputs, point_influence, K_points, KP_influence, aggregation_mode, add_one)
        self.modulated = modulated
        self.internal_losses = {self.PERMISSIVE_LOSS_KEY: 0.0, self.FITTING_LOSS_KEY: 0.0, self.REPULSION_LOSS_KEY: 0.0}
        self.loss_mode = loss_mode
        offset_dim = (4 if modulated else 3) * self.n_kernel_points
        self.offset_weights = self._xavier(offset_dim)
        self.offset_bias = nn.Parameter(torch.zeros(offset_dim, dtype=torch.float32))
        self.weight = self._xavier(num_outputs)

    def forward(self, query_points, support_points, neighbors, x):
        from . import kpconv_losses as _losses
        x = self._features(support_points, x)
        offset_feat = KPConv_ops(query_points, support_points, neighbors, x, self.K_points, self.offset_weights,
                                 self.point_influence, self.KP_influence, self.aggregation_mode) + self.offset_bias
        KP = self.n_kernel_points
        if self.modulated:
            offsets = offset_feat[:, :3 * KP].reshape(-1, KP, 3)
            modulations = 2 * torch.sigmoid(offset_feat[:, 3 * KP:])
        else:
            offsets = offset_feat.reshape(-1, KP, 3)
            modulations = None
        offsets = offsets * self.point_influence
        new_feat, kp_min_d2, K_points_deformed = KPConv_deform_ops(
            query_points, support_points, neighbors, x, self.K_points, offsets, modulations, self.weight,
            self.point_influence, self.KP_influence, self.aggregation_mode)
        if self.loss_mode == "fitting":
            self.internal_losses[self.FITTING_LOSS_KEY] = _losses.fitting_loss(kp_min_d2, self.kernel_radius)
            self.internal_losses[self.REPULSION_LOSS_KEY] = _losses.repulsion_loss(K_points_deformed, self.point_influence)
        elif self.loss_mode == "permissive":
            self.internal_losses[self.PERMISSIVE_LOSS_KEY] = _losses.permissive_loss(K_points_deformed, self.kernel_radius)
        else:
            raise NotImplementedError("Loss mode %s not recognised. Only permissive and fitting are valid" % self.loss_mode)
        return new_feat

    def get_internal_losses(self):
        return self.internal_losses

    def __repr__(self):
        return "KPConvDeformableLayer(InF: %i, OutF: %i, kernel_pts: %i, radius: %.2f, KP_influence: %s)" % (
            self.num_inputs, self.num_outputs, self.n_kernel_points, self.kernel_radius, self.KP_influence)
