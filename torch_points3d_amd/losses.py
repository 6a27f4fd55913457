"""Dirichlet loss on the HIP radius search: a free beneficiary of the kernel boundary.

Mirrors torch_points3d/core/losses/dirichlet_loss.py:9-77 (`DirichletLoss`, `dirichlet_loss`): dense clouds go through
`ball_query(r, 32, pos, pos, sort=True)` exactly like the reference (:51-55; pad-with-the-closest makes padded slots
contribute (f_i - f_i)^2 = 0); the sparse variant replaces torch_cluster's `radius` + `scatter_add` (:63-77) by the
partial-dense search, whose -1 slots are dropped.  Pinned by the reference's known answers (test/test_losses.py:16-38).
"""
import torch

from . import torchpoints as _tp

_MAX_NEIGHBOURS = 32


def _variance_estimator_dense(r, pos, f):
    nei_idx = _tp.ball_query(r, _MAX_NEIGHBOURS, pos, pos, sort=True)[0].reshape(pos.shape[0], -1).long()
    f_neighboors = f.gather(1, nei_idx).reshape(f.shape[0], f.shape[1], -1)
    return ((f.unsqueeze(-1) - f_neighboors) ** 2).sum(-1)


def _variance_estimator_sparse(r, pos, f, batch_idx):
    with torch.no_grad():
        idx = _tp.ball_query(r, _MAX_NEIGHBOURS, pos, pos, mode="partial_dense", batch_x=batch_idx, batch_y=batch_idx)[0]
        valid = idx >= 0
        safe = torch.where(valid, idx, torch.zeros_like(idx))
    return (((f[safe] - f.unsqueeze(-1)) ** 2) * valid).sum(-1)


def dirichlet_loss(r, pos, f, batch_idx=None, aggr=torch.mean):
    if batch_idx is None:
        assert f.dim() == 2 and pos.dim() == 3
        return 1 / 2.0 * aggr(_variance_estimator_dense(r, pos, f))
    assert f.dim() == 1 and pos.dim() == 2
    return 1 / 2.0 * aggr(_variance_estimator_sparse(r, pos, f, batch_idx))


class DirichletLoss(torch.nn.Module):
    """L2 norm of the gradient of a field f estimated from its change across neighbours within a radius r."""

    def __init__(self, r, aggr=torch.mean):
        super().__init__()
        self._r = r
        self._aggr = aggr

    def forward(self, pos, f, batch_idx=None):
        return dirichlet_loss(self._r, pos, f, batch_idx=batch_idx, aggr=self._aggr)


def huber_loss(error, delta=1.0):
    """Element-wise Huber penalty of core/losses/huber_loss.py:34-51: x^2 / 2 up to |x| = delta, linear with slope delta
    beyond."""
    mag = error.abs()
    q = mag.clamp(max=delta)
    return 0.5 * (q * q) + delta * (mag - q)


def nn_distance(pc1, pc2, l1smooth=False, delta=1.0, l1=False):
    """Nearest row of the other set, both ways (core/losses/huber_loss.py:4-31): pc1 (B, N, C), pc2 (B, M, C) ->
    (dist1 (B, N), idx1 (B, N), dist2 (B, M), idx2 (B, M)) under the squared (default), l1 or Huber distance summed over
    C.  The (B, N, M, C) differences come from broadcasting, so the reference's two `repeat`ed copies are never written;
    the arithmetic per element is the same."""
    diff = pc1[:, :, None, :] - pc2[:, None, :, :]
    if l1smooth:
        cost = huber_loss(diff, delta)
    elif l1:
        cost = diff.abs()
    else:
        cost = diff * diff
    cost = cost.sum(-1)
    dist1, idx1 = cost.min(dim=2)
    dist2, idx2 = cost.min(dim=1)
    return dist1, idx1, dist2, idx2
