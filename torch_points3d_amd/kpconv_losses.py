"""Regularisers of the deformable kernel-point convolution (reference modules/KPConv/losses.py), plain torch: they
are small (Nq, KP, .) reductions over what csrc/kpconv_deform.hip and the offset addition return."""
import torch


def fitting_loss(sq_distance, radius):
    """Every kernel point should have a neighbour close to it: mean over (query, kernel point) of the smallest squared
    distance, in units of radius^2.  `sq_distance`: the reference's (Nq, Mn, KP) tensor, or the (Nq, KP) minimum over
    the neighbours that `KPConv_deform_ops` of this package returns."""
    kpmin = sq_distance.min(dim=1)[0] if sq_distance.dim() == 3 else sq_distance
    return torch.mean(kpmin / (radius ** 2))


def repulsion_loss(deformed_kpoints, radius):
    """Deformed kernel points (Nq, KP, 3) closer than 1.5 to each other repel.  As in the reference, `radius` does not
    enter (losses.py:24 discards the normalised tensor) and the other points of a pair are constants."""
    n_points = deformed_kpoints.shape[1]
    repulsive_loss = 0
    for i in range(n_points):
        with torch.no_grad():
            other_points = torch.cat([deformed_kpoints[:, :i, :], deformed_kpoints[:, i + 1:, :]], dim=1)
        distances = torch.sqrt(torch.sum((other_points - deformed_kpoints[:, i:i + 1, :]) ** 2, dim=-1))
        repulsion_force = torch.sum(torch.pow(torch.relu(1.5 - distances), 2), dim=1)
        repulsive_loss = repulsive_loss + torch.mean(repulsion_force)
    return repulsive_loss


def permissive_loss(deformed_kpoints, radius):
    """Mean normalised norm of the deformed kernel points that left the kernel radius (NaN when none did, as in the
    reference)."""
    norm_deformed_normalized = torch.norm(deformed_kpoints, p=2, dim=-1) / float(radius)
    return torch.mean(norm_deformed_normalized[norm_deformed_normalized > 1.0])


def collect_internal_losses(model):
    """{module name + "." + key: loss} over every module of `model` that has `get_internal_losses()`."""
    out = {}
    for name, m in model.named_modules():
        if hasattr(m, "get_internal_losses"):
            for key, value in m.get_internal_losses().items():
                out[(name + "." if name else "") + key] = value
    return out


def internal_loss(model, weight=1.0):
    """Sum of the internal losses of the model's modules (what the reference's BaseModel.get_internal_loss adds to the
    task loss): each loss that is a tensor enters, the untouched 0.0 placeholders do not."""
    total = 0
    for value in collect_internal_losses(model).values():
        if torch.is_tensor(value):
            total = total + weight * value
    return total
