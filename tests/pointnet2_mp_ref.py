"""Plain-torch CPU statement of the message-passing PointNet++ kernels (csrc/pointconv.hip, tp3d_fps_ragged_f32's
quota), for the kernel tests to compare against and for the fixture generator.  Test infrastructure: the product has
no CPU path."""
import math

import numpy as np
import torch


# the network of tests/golden/pointnet2_mp.npz (tests/golden/make_golden_mp.py): conf/models/segmentation/pointnet2.yaml's
# `pointnet2` with narrow widths on clouds of 97, 160 and 64 points, and one two-scale SAModule (`pointnet2ms` form)
GOLD_SIZES = (97, 160, 64)
GOLD_FEAT, GOLD_CLASSES, GOLD_CAP = 4, 5, 16
GOLD_CFG = dict(
    down_conv=dict(ratios=[0.25, 0.25], radius=[0.75, 1.2], radius_num_points=[GOLD_CAP, GOLD_CAP],
                   down_conv_nn=[[GOLD_FEAT + 3, 16, 16, 32], [32 + 3, 32, 32, 64]]),
    up_conv=dict(up_conv_nn=[[128 + 64, 64], [64 + 32, 64, 32], [32 + GOLD_FEAT, 32, 32]], up_k=[1, 3, 3], skip=True),
    innermost=dict(aggr="max", nn=[64 + 3, 64, 128]),
    mlp_cls=dict(nn=[32, 32, 32, 32, 32], dropout=0.0))
GOLD_MS = dict(ratio=0.25, radius=[0.5, 0.75], radius_num_point=[8, GOLD_CAP], down_conv_nn=[GOLD_FEAT + 3, 16, 32])


def fps_quota(counts, ratio):
    """ceil(float32(n) * float32(ratio)) clamped to [0, n], one cloud at a time in numpy float32"""
    out = []
    for n in counts:
        q = int(math.ceil(float(np.float32(n) * np.float32(ratio))))
        out.append(max(0, min(int(n), q)))
    return out


def table_edges(table):
    """-1 padded (Nq, W) table -> (edge_start (Nq+1), col (E)): the entries >= 0, row-major, in slot order"""
    keep = table >= 0
    edge_start = torch.zeros(table.shape[0] + 1, dtype=torch.int64)
    edge_start[1:] = torch.cumsum(keep.sum(1), 0)
    return edge_start, table[keep]


def edge_rows(x, pos_s, pos_q, edge_start, col, ld=None):
    """rows[e] = [ x[col[e]] | pos_s[col[e]] - pos_q[query of e] | 0 .. ]"""
    nq = edge_start.numel() - 1
    row = torch.repeat_interleave(torch.arange(nq), edge_start[1:] - edge_start[:-1])
    parts = ([] if x is None else [x[col]]) + [pos_s[col] - pos_q[row]]
    rows = torch.cat(parts, 1)
    if ld is not None and ld > rows.shape[1]:
        rows = torch.cat([rows, rows.new_zeros(rows.shape[0], ld - rows.shape[1])], 1)
    return rows


def segment_max(rows, seg, C=None):
    """(out (S, C), argmax (S, C)): max over rows seg[s] .. seg[s+1]), first maximum wins; empty -> 0.0 / -1.
    Differentiable wrt rows (index_select of the winning rows)."""
    C = rows.shape[1] if C is None else C
    S = seg.numel() - 1
    outs, args = [], []
    for s in range(S):
        a, b = int(seg[s]), int(seg[s + 1])
        if a == b:
            outs.append(rows.new_zeros(C))
            args.append(torch.full((C,), -1, dtype=torch.int64))
            continue
        blk = rows[a:b, :C]
        top = blk.max(0)[0]
        first = (blk == top).to(torch.int64).argmax(0)  # argmax of a 0/1 tensor: the first 1
        outs.append(blk.gather(0, first.unsqueeze(0))[0])
        args.append(first + a)
    return torch.stack(outs), torch.stack(args)
