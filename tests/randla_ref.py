"""Plain-torch restatement of the reference's RandlaKernel (modules/RandLANet/modules.py:9-54) on a kNN EDGE LIST, for
tests/test_gpu_randla_rows.py: cat -> MLP -> cat -> MLP -> softmax -> mul -> segment sum -> MLP, nothing else.  Only real
edges exist here, so every nn.BatchNorm1d takes its batch statistics over real edges -- which is what a fixed-k table
with -1 slots has to reproduce.  Module names match torch_points3d_amd.randla.RandlaKernel, so one state_dict serves
both; runs in whatever dtype the module was cast to."""
import torch
import torch.nn as nn


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(c, momentum=0.1)

    def forward(self, x):
        return self.batch_norm(x)


def _mlp(channels):
    return nn.Sequential(*[nn.Sequential(nn.Linear(channels[i - 1], channels[i]), _BN(channels[i]), nn.LeakyReLU(0.2))
                           for i in range(1, len(channels))])


class RandlaEdgeList(nn.Module):
    def __init__(self, point_pos_nn, attention_nn, global_nn):
        super().__init__()
        self.point_pos_nn = _mlp(point_pos_nn)
        self.attention_nn = _mlp(attention_nn)
        self.global_nn = _mlp(global_nn)

    def forward(self, x, pos_q, pos_s, edge_index):
        """edge_index (2, E): row 0 = support row j, row 1 = query row i (the reference's layout)"""
        j, i = edge_index[0], edge_index[1]
        pos_i, pos_j = pos_q[i], pos_s[j]
        x_j = pos_j if x is None else x[j]
        vij = pos_i - pos_j
        dij = torch.norm(vij, dim=1).unsqueeze(1)
        rij = self.point_pos_nn(torch.cat([pos_i, pos_j, vij, dij], dim=1))
        fij_hat = torch.cat([x_j, rij], dim=1)
        msg = torch.softmax(self.attention_nn(fij_hat), -1) * fij_hat
        agg = torch.zeros((pos_q.shape[0], msg.shape[1]), dtype=msg.dtype).index_add_(0, i, msg)
        return self.global_nn(agg)


def edge_list(nbr):
    """(2, E) real edges of a fixed-k table, query-major"""
    k = nbr.shape[1]
    flat = nbr.reshape(-1)
    keep = torch.nonzero(flat >= 0).reshape(-1)
    return torch.stack([flat[keep], torch.div(keep, k, rounding_mode="floor")], dim=0)
