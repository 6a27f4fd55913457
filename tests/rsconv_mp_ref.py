"""Plain-torch statement of the message-passing RSConv kernels (csrc/rsconv_mp.hip) and of the modules of
torch_points3d_amd/rsconv_mp.py, dtype-generic (float32 or float64) and device-generic, for the kernel tests to compare
against and for the fixture generator.  Test infrastructure: the product has no CPU path.  The FPS quota, the edge
helpers, segment_max and the shared modules are those of tests/pointnet2_mp_ref.py."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointnet2_mp_ref as mp

# the network of tests/golden/rsconv_mp.npz (tests/golden/make_golden_rsconv_mp.py): conf/models/segmentation/rsconv.yaml's
# RSConv_2LD form with narrow widths on clouds of 150, 97 and 64 points with x = None (FEAT = 3), the finder's cap of 64,
# and one stand-alone Convolution with 16 feature channels
GOLD_SIZES = (150, 97, 64)
GOLD_FEAT, GOLD_CLASSES, GOLD_CAP = 3, 5, 64
GOLD_CFG = dict(
    down_conv=dict(ratios=[0.25, 0.25], radius=[1.1, 1.2], local_nn=[[10, 8, GOLD_FEAT], [10, 16, 16]],
                   down_conv_nn=[[GOLD_FEAT, 8, 16], [16, 16, 32]]),
    innermost=dict(aggr="max", nn=[32 + 3, 64]),
    up_conv=dict(up_conv_nn=[[64 + 32, 32], [32 + 16, 32], [32, 32]], up_k=[1, 3, 3], skip=True),
    mlp_cls=dict(nn=[32, 32, 32, 32, 32], dropout=0.0))
GOLD_CONV = dict(local_nn=[10, 16, 16], global_nn=[16, 24], C=16, ratio=0.25, radius=0.9)


def _row_of(edge_start):
    nq = edge_start.numel() - 1
    return torch.repeat_interleave(torch.arange(nq, device=edge_start.device), edge_start[1:] - edge_start[:-1])


def relation_rows(pos_s, pos_q, edge_start, col, ld=None):
    """rows[e] = [ |d|, d = pos_q[i] - pos_s[col[e]], pos_q[i], pos_s[col[e]], 0 .. ] for the edges e of query i"""
    row = _row_of(edge_start)
    p_i, p_j = pos_q[row], pos_s[col]
    d = p_i - p_j
    rows = torch.cat([torch.norm(d, dim=1).unsqueeze(1), d, p_i, p_j], 1)
    if ld is not None and ld > rows.shape[1]:
        rows = torch.cat([rows, rows.new_zeros(rows.shape[0], ld - rows.shape[1])], 1)
    return rows


def msgmax(w, x, edge_start, col, C=None):
    """(out (Nq, C), argmax (Nq, C)) = segment_max(w[:, :C] * x[col, :C]): the composition the fused kernel replaces.
    The product is taken on the device of w; the max, a selection, walks the segments on the host."""
    C = x.shape[1] if C is None else C
    out, arg = mp.segment_max((w[:, :C] * x[col, :C]).cpu(), edge_start.cpu())
    return out.to(w.device), arg.to(w.device)


class Convolution(nn.Module):
    """out[i] = global_nn(relu(max over the edges of query i of local_nn(h_ij) * x_j)), x_j = pos_j without features"""

    def __init__(self, local_nn, global_nn=None):
        super().__init__()
        self.local_nn, self.global_nn = local_nn, global_nn

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        glob = mp._mlp_of(sd, "global_nn.") if "global_nn.0.0.weight" in sd else None
        return mp._loaded(cls(mp._mlp_of(sd, "local_nn."), glob), sd, dtype)

    def forward(self, x, pos, edges):
        (pos_s, pos_q), (edge_start, col) = pos, edges
        x = pos_s if x is None else x
        self.weights = self.local_nn(relation_rows(pos_s, pos_q, edge_start, col))
        msg = self.weights * x[col]
        self.margin = min(getattr(self, "margin", float("inf")), mp.pool_margin(msg, edge_start))
        out, self.arg = mp.segment_max(msg, edge_start)
        out = F.relu(out)
        return out if self.global_nn is None else self.global_nn(out)


class RSConvDown(nn.Module):
    """the sampled rows `idx` are the queries: source = pos, target = pos[idx]"""

    def __init__(self, local_nn, global_nn):
        super().__init__()
        self._conv = Convolution(local_nn, global_nn)

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        return mp._loaded(cls(mp._mlp_of(sd, "_conv.local_nn."), mp._mlp_of(sd, "_conv.global_nn.")), sd, dtype)

    def forward(self, x, pos, idx, edges):
        return self._conv(x, (pos, pos[idx]), edges)


class RSConvMP(mp.NestedMP):
    """pointnet2_mp_ref.NestedMP over RSConvDown: stages rs1 .. rs<n>, the one scale's edges of a level"""
    STAGE = "rs"

    @staticmethod
    def down_of(sd, prefix):
        return RSConvDown(mp._mlp_of(sd, prefix + "_conv.local_nn."), mp._mlp_of(sd, prefix + "_conv.global_nn."))

    @staticmethod
    def edges_of(plan, i):
        return plan["edges"][i][0]
