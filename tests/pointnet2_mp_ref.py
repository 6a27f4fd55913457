"""Plain-torch CPU statement of the message-passing PointNet++ kernels (csrc/pointconv.hip, tp3d_fps_ragged_f32's
quota), for the kernel tests to compare against and for the fixture generator, and (second half) of the modules of
torch_points3d_amd/pointnet2_mp.py, runnable in float32 or float64.  Test infrastructure: the product has no CPU path."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


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


# ------------------------------------------------------------------------------------------------ the modules, in torch
# Mirrors of torch_points3d_amd/pointnet2_mp.py written from its docstrings and the fixture's stage names: same attribute
# names, so a product module's state_dict loads as it is, widths are read off its weight shapes.  Every search result is
# an INPUT (teacher-forced): sample indices, CSR edges per scale, kNN tables.  tests/test_pointnet2_mp_cpu.py pins the
# float64 run of these classes against the fixture the reference's own classes wrote.
class _BN(nn.Module):
    def __init__(self, width, momentum=0.1):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(width, momentum=momentum)

    def forward(self, x):
        return self.batch_norm(x)


def _mlp(channels, bias=True):
    """[Linear -> BatchNorm1d (under .batch_norm) -> LeakyReLU(0.2)] per consecutive pair of widths"""
    return nn.Sequential(*[nn.Sequential(nn.Linear(channels[i - 1], channels[i], bias=bias), _BN(channels[i]),
                                         nn.LeakyReLU(0.2)) for i in range(1, len(channels))])


def _mlp_of(sd, prefix):
    """the MLP whose parameters sit under `prefix` of a state_dict: widths and bias from the Linear weights"""
    channels, bias, i = [], False, 0
    while "%s%d.0.weight" % (prefix, i) in sd:
        w = sd["%s%d.0.weight" % (prefix, i)]
        channels = channels or [w.shape[1]]
        channels.append(w.shape[0])
        bias = ("%s%d.0.bias" % (prefix, i)) in sd
        i += 1
    assert channels, "no MLP under %r" % prefix
    return _mlp(channels, bias=bias)


def pool_margin(rows, seg):
    """the closest contest of segment_max(rows, seg): the smallest distance between the largest and the second largest
    value of a (segment, column), over the segments of two rows or more (inf if there is none).  A margin of the order
    of float32 rounding means that a float32 evaluation may crown another row, and the gradient moves with it."""
    best = float("inf")
    for s in range(seg.numel() - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        if b - a >= 2:
            top = rows[a:b].detach().topk(2, 0)[0]
            best = min(best, float((top[0] - top[1]).min()))
    return best


def _loaded(module, sd, dtype):
    module.load_state_dict(sd, strict=True)
    return module.to(dtype).train()


class PointConv(nn.Module):
    """out[i] = global_nn(max over the edges of query i of local_nn(cat([x_j, pos_j - pos_i]))); no edge -> 0.0"""

    def __init__(self, local_nn=None, global_nn=None):
        super().__init__()
        self.local_nn, self.global_nn = local_nn, global_nn

    def forward(self, x, pos, edges):
        (pos_s, pos_q), (edge_start, col) = pos, edges
        rows = edge_rows(x, pos_s, pos_q, edge_start, col)
        if self.local_nn is not None:
            rows = self.local_nn(rows)
        self.margin = min(getattr(self, "margin", float("inf")), pool_margin(rows, edge_start))  # over all calls
        out = segment_max(rows, edge_start)[0]
        return out if self.global_nn is None else self.global_nn(out)


class SAModule(nn.Module):
    """the sampled rows `idx` are the queries; per scale its edges through the shared PointConv, scales concatenated"""

    def __init__(self, local_nn):
        super().__init__()
        self._conv = PointConv(local_nn=local_nn)

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        return _loaded(cls(_mlp_of(sd, "_conv.local_nn.")), sd, dtype)

    def forward(self, x, pos, idx, edges):
        """edges: one (edge_start, col) per scale -> x of the sampled level"""
        return torch.cat([self._conv(x, (pos, pos[idx]), e) for e in edges], -1)


class GlobalBaseModule(nn.Module):
    """MLP(cat[x, pos]), then the max over the rows of every cloud (`batch` sorted)"""

    def __init__(self, mlp):
        super().__init__()
        self.nn = mlp

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        return _loaded(cls(_mlp_of(sd, "nn.")), sd, dtype)

    def forward(self, x, pos, batch):
        seg = torch.zeros(int(batch.max()) + 2, dtype=torch.int64)
        seg[1:] = torch.cumsum(torch.bincount(batch), 0)
        rows = self.nn(torch.cat([x, pos], 1))
        self.margin = pool_margin(rows, seg)
        return segment_max(rows, seg)[0]


def knn_blend(x, pos_x, pos_y, idx):
    """inverse-squared-distance blend of the rows idx (Nq, k; -1 = no neighbour) of x, distances in pos_x's dtype"""
    keep = (idx >= 0).to(x.dtype).unsqueeze(-1)
    safe = idx.clamp(min=0)
    d2 = ((pos_x[safe] - pos_y.unsqueeze(1)) ** 2).sum(-1, keepdim=True)
    w = keep / torch.clamp(d2, min=1e-16)
    return (x[safe] * w).sum(1) / w.sum(1)


class FPModule(nn.Module):
    """kNN blend of the coarse features onto the skip level, cat with the skip features, MLP(bias=False)"""

    def __init__(self, mlp):
        super().__init__()
        self.nn = mlp

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        return _loaded(cls(_mlp_of(sd, "nn.")), sd, dtype)

    def forward(self, x, pos, x_skip, pos_skip, knn_idx):
        x = knn_blend(x, pos, pos_skip, knn_idx)
        return self.nn(x if x_skip is None else torch.cat([x, x_skip], 1))


class _Block(nn.Module):
    def __init__(self, up, down=None, submodule=None, inner=None):
        super().__init__()
        if inner is not None:
            self.inner = inner
        else:
            self.down, self.submodule = down, submodule
        self.up = up


class NestedMP(nn.Module):
    """the nested network: down module x n, GlobalBaseModule, FPModule x (n + 1), relu(lin1) -> lin2 -> lin3 ->
    log_softmax (no dropout).  forward returns every stage: <STAGE>1 .. <STAGE>n, glob, fp0 .. fp<n>, out.  A subclass
    names STAGE, builds the down module from the state_dict (`down_of(sd, prefix)`) and picks a level's edges from the
    plan (`edges_of(plan, i)`)."""
    STAGE = None

    def __init__(self, sd):
        super().__init__()
        n = 0
        while ("model." + "submodule." * n + "down._conv.local_nn.0.0.weight") in sd:
            n += 1
        self.levels = n
        deep = "model." + "submodule." * n
        block = _Block(FPModule(_mlp_of(sd, deep + "up.nn.")), inner=GlobalBaseModule(_mlp_of(sd, deep + "inner.nn.")))
        for i in range(n - 1, -1, -1):
            at = "model." + "submodule." * i
            block = _Block(FPModule(_mlp_of(sd, at + "up.nn.")), down=self.down_of(sd, at + "down."), submodule=block)
        self.model = block
        for name in ("lin1", "lin2", "lin3"):
            w = sd[name + ".weight"]
            setattr(self, name, nn.Linear(w.shape[1], w.shape[0]))

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float64):
        return _loaded(cls(sd), sd, dtype)

    def blocks(self):
        out, b = [], self.model
        for _ in range(self.levels + 1):
            out.append(b)
            b = getattr(b, "submodule", None)
        return out

    def margin(self):
        """the closest max-pool contest of the passes so far (pool_margin), over every pool of the network"""
        blocks = self.blocks()
        return min([b.down._conv.margin for b in blocks[:-1]] + [blocks[-1].inner.margin])

    def forward(self, x, pos, batch, plan):
        """plan (see `search_plan`): idx[i], edges[i] (one (edge_start, col) per scale) of level i, knn[j] the table of
        feature-propagation module j (fp0 is the innermost one); x may be None where the down module takes that"""
        blocks, n = self.blocks(), self.levels
        rec = {}
        lv = [(x, pos, batch)]
        for i in range(n):
            x_i, pos_i, batch_i = lv[-1]
            idx = plan["idx"][i]
            lv.append((blocks[i].down(x_i, pos_i, idx, self.edges_of(plan, i)), pos_i[idx], batch_i[idx]))
            rec["%s%d" % (self.STAGE, i + 1)] = lv[-1][0]
        x_n, pos_n, batch_n = lv[-1]
        cur = rec["glob"] = blocks[n].inner(x_n, pos_n, batch_n)
        cur_pos = pos_n.new_zeros(cur.shape[0], 3)
        for j in range(n + 1):
            x_s, pos_s, _ = lv[n - j]
            cur = rec["fp%d" % j] = blocks[n - j].up(cur, cur_pos, x_s, pos_s, plan["knn"][j])
            cur_pos = pos_s
        rec["out"] = F.log_softmax(self.lin3(self.lin2(F.relu(self.lin1(cur)))), dim=-1)
        return rec


class PointNet2MP(NestedMP):
    """NestedMP over SAModule: stages sa1 .. sa<n>, every scale's edges of a level"""
    STAGE = "sa"

    @staticmethod
    def down_of(sd, prefix):
        return SAModule(_mlp_of(sd, prefix + "_conv.local_nn."))

    @staticmethod
    def edges_of(plan, i):
        return plan["edges"][i]


def search_plan(oracle, pos, batch, ratios, radius, caps, up_k):
    """Every search of the network on float32 positions, by the CPU oracle: per level the furthest-point samples of every
    cloud (quota fps_quota) and one compacted partial-dense ball query per scale, then the kNN table of every
    feature-propagation module (the innermost one searches the pooled level: one row at the origin per cloud)."""
    plan = dict(idx=[], edges=[], knn=[], pos=[pos], batch=[batch])
    for ratio, rr, cc in zip(ratios, radius, caps):
        p, b = plan["pos"][-1], plan["batch"][-1]
        sizes = torch.bincount(b).tolist()
        idx, base = [], 0
        for n, q in zip(sizes, fps_quota(sizes, ratio)):
            if n and q:
                idx.append(oracle.furthest_point_sample(p[base:base + n].unsqueeze(0), q)[0] + base)
            base += n
        idx = torch.cat(idx)
        rr = rr if isinstance(rr, (list, tuple)) else [rr]
        cc = cc if isinstance(cc, (list, tuple)) else [cc] * len(rr)
        plan["idx"].append(idx)
        plan["edges"].append([table_edges(oracle.ball_query(r, c, p, p[idx], mode="partial_dense", batch_x=b,
                                                             batch_y=b[idx])[0]) for r, c in zip(rr, cc)])
        plan["pos"].append(p[idx])
        plan["batch"].append(b[idx])
    clouds = int(batch.max()) + 1
    cur_pos, cur_batch = torch.zeros(clouds, 3), torch.arange(clouds)
    for j, k in enumerate(up_k):
        p, b = plan["pos"][len(ratios) - j], plan["batch"][len(ratios) - j]
        plan["knn"].append(oracle.knn(k, cur_pos, p, cur_batch, b)[0])
        cur_pos, cur_batch = p, b
    return plan
