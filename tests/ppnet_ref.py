"""Plain-torch restatement of PosPool position pooling (reference modules/PPNet/ops.py:44-109), for any floating dtype
and device.  tests/test_ppnet_cpu.py pins it to the reference's own tensors (tests/golden/ppnet.npz); the GPU tests
evaluate it on the device in float64 (the yardstick) and in float32 (the distance a correct fp32 evaluation keeps from
the yardstick).  The caller's table is not modified."""
import torch


def dim_mat(feat_dim, dtype, device):
    """1000^(j / F), j < F: evaluated on the host in `dtype`, as a reference pass on the CPU evaluates it."""
    feat_range = torch.arange(feat_dim, dtype=dtype)
    return torch.pow(1.0 * 1000, (1.0 / feat_dim) * feat_range).to(device)


def geo_prior(rel, C, embedding):
    """(Nq, Mn, C) prior of the relative positions rel (Nq, Mn, 3)."""
    Nq, Mn = rel.shape[:2]
    if embedding == "xyz":
        return rel.unsqueeze(-1).expand(Nq, Mn, 3, C // 3).reshape(Nq, Mn, C)
    F = 1 if C == 9 else C // 6
    div = (100 * rel.unsqueeze(-1)) / dim_mat(F, rel.dtype, rel.device)  # (Nq, Mn, 3, F)
    emb = torch.cat([torch.sin(div), torch.cos(div)], -1).reshape(Nq, Mn, 6 * F)
    return torch.cat([emb, rel], -1) if C == 9 else emb


def pospool_ref(query, support, neighbors, features, radius, embedding="xyz", reduction="avg"):
    M, C = features.shape
    Nq, Mn = neighbors.shape
    idx = torch.where((neighbors < 0) | (neighbors >= M), torch.full_like(neighbors, M), neighbors)
    flat = idx.reshape(-1)
    pts = torch.cat([support, torch.zeros_like(support[:1])], 0).index_select(0, flat).view(Nq, Mn, 3)
    rows = torch.cat([features, torch.zeros_like(features[:1])], 0).index_select(0, flat).view(Nq, Mn, C)
    rel = (pts - query.unsqueeze(1)) / radius
    out = (geo_prior(rel, C, embedding) * rows).sum(1)
    if reduction == "avg":
        count = (idx < idx.max()).sum(-1) + 1e-5  # float32 whatever the dtype of the features, as in the reference
        out = out / count.unsqueeze(-1)
    elif reduction != "sum":
        raise NotImplementedError(reduction)
    return out
