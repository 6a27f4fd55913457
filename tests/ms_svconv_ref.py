"""Plain-torch restatement of MS-SVConv ("MS-SVConv"): tests/sparseconv_ref.py extended to kernel_size 5, the
voxelisation of UnetMSparseConv3d._prepare_data, the multi-scale head and the models of models/registration/ms_svconv3d.py
and models/segmentation/ms_svconv3d.py with the reference's attribute names.  fp32 and float64, any device.

    k = 5, stride 1      F.conv3d(stride=1, padding=2) on the grid indexed [x, y, z], read at the output set
                         (offsets {-2 .. 2} * tensor stride per axis, x slowest, z fastest)

Everything else of the convolution family is sparseconv_ref's.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import sparseconv_ref as sr


# ------------------------------------------------------------------------------------------------------------- convolution
def offsets(ksize, ts):
    if ksize == 5:
        r = [-2, -1, 0, 1, 2]
        return [(a * ts, b * ts, c * ts) for a in r for b in r for c in r]  # x slowest, z fastest
    return sr.offsets(ksize, ts)


def kernel_map(C_in, C_out, ksize, ts):
    """(forward (Nout, K), inverse (Nin, K)) int32, as sparseconv_ref.kernel_map, also for ksize 5"""
    offs = offsets(ksize, ts)
    fwd = torch.stack([sr.lookup(C_out, o, C_in) for o in offs], 1)
    inv = torch.stack([sr.lookup(C_in, tuple(-v for v in o), C_out) for o in offs], 1)
    return fwd.int(), inv.int()


def conv(Fx, C_in, C_out, W, ksize, stride, ts, transposed=False):
    if ksize != 5:
        return sr.conv(Fx, C_in, C_out, W, ksize, stride, ts, transposed)
    assert stride == 1 and not transposed
    cin, cout = W.shape[-2], W.shape[-1]
    Wd = W.reshape(5, 5, 5, cin, cout)
    both = torch.cat([C_in.long(), C_out.long()], 0)
    B = int(both[:, 3].max()) + 1
    origin = torch.div(both[:, :3].min(0).values, ts, rounding_mode="floor") * ts
    shape = (both[:, :3].max(0).values - origin) // ts + 1
    g = sr._dense(Fx, C_in, ts, origin, shape.tolist(), B)
    out = F.conv3d(g, Wd.permute(4, 3, 0, 1, 2), stride=1, padding=2)
    return sr._read(out, C_out, ts, origin)


conv_by_table = sr.conv_by_table


class Conv3d(sr.Conv3d):
    def forward(self, x):
        if self.k == 5:
            return x.like(conv(x.F, x.C, x.C, self.kernel, 5, 1, x.s))
        return super().forward(x)


class ResNetDown(sr.ResNetDown):
    CONVOLUTION = Conv3d


class UNet(nn.Module):
    """the U-Net of applications/sparseconv3d.py from a resolved option dict; `N` absent = one block per stage"""

    def __init__(self, cfg):
        super().__init__()
        d, u = cfg["down_conv"], cfg["up_conv"]
        nd, nu = len(d["down_conv_nn"]), len(u["up_conv_nn"])
        dN, uN = d.get("N", [1] * nd), u.get("N", [1] * nu)
        self.down_modules = nn.ModuleList(ResNetDown(d["down_conv_nn"][i], d["kernel_size"][i], 1, d["stride"][i], dN[i],
                                                     d.get("block", "ResBlock")) for i in range(nd))
        self.up_modules = nn.ModuleList(sr.ResNetUp(u["up_conv_nn"][i], u["kernel_size"][i], 1, u["stride"][i], uN[i],
                                                    u.get("block", "ResBlock")) for i in range(nu))
        self.inner_modules = nn.ModuleList()

    def forward(self, Fx, C):
        x = sr.RefTensor(Fx, C)
        stack = []
        for m in self.down_modules[:-1]:
            x = m(x)
            stack.append(x)
        x = self.down_modules[-1](x)
        stack.append(None)
        for m in self.up_modules:
            x = m(x, stack.pop())
        return x.F


# ------------------------------------------------------------------------------------------------------------ voxelisation
def voxelize(pos, batch, grid_size, x, aggr=None):
    """UnetMSparseConv3d._prepare_data: coords = round(pos / grid_size) (half to even); voxel ids ascending in (batch, z, y, x)
    -- the order of voxel_grid's flat index made consecutive --, unique_pos_indices the highest point index of each voxel.
    Returns (coords (K, 3) int64, batch (K,), pos (K, 3), x (K, C), cluster (N,), unique_pos_indices (K,))."""
    coords = torch.round(pos / grid_size).long()
    key = torch.stack([batch.long(), coords[:, 2], coords[:, 1], coords[:, 0]], 1)
    uniq, cluster = torch.unique(key, dim=0, return_inverse=True)
    K = len(uniq)
    n = torch.arange(len(pos), device=pos.device)
    upi = torch.full((K,), -1, dtype=torch.long, device=pos.device).scatter_reduce(0, cluster, n, "amax", include_self=True)
    if aggr is None:
        xv = x[upi]
    elif aggr == "mean":
        cnt = torch.zeros(K, dtype=x.dtype, device=x.device).index_add_(0, cluster, torch.ones_like(x[:, 0]))
        xv = torch.zeros((K, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, cluster, x) / cnt.unsqueeze(1)
    elif aggr == "max":
        xv = torch.full((K, x.shape[1]), float("-inf"), dtype=x.dtype, device=x.device).scatter_reduce(
            0, cluster.unsqueeze(1).expand_as(x), x, "amax", include_self=True)
    else:
        raise NotImplementedError
    return coords[upi], batch[upi], pos[upi], xv, cluster, upi


# ------------------------------------------------------------------------------------------------------------------- head
def normalize(x, eps=1e-20):
    return x / (torch.norm(x, p=2, dim=1, keepdim=True) + eps)


def scale_fuse(xs, mode="cat", eps=1e-20):
    """(fused, [normalised scales]) by the reference's own formula (apply_nn of the three registration classes)"""
    hs = [normalize(x, eps) for x in xs]
    if mode == "cat":
        return torch.cat(hs, 1), hs
    if mode == "max":
        return torch.cat([h.unsqueeze(0) for h in hs], 0).max(0)[0], hs
    if mode == "mean":
        return torch.cat([h.unsqueeze(0) for h in hs], 0).mean(0), hs
    raise NotImplementedError


# ----------------------------------------------------------------------------------------------------------------- models
class _BN(nn.Module):
    """FastBatchNorm1d's layout: the statistics live under `.batch_norm`"""

    def __init__(self, c, momentum):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(c, momentum=momentum)

    def forward(self, x):
        return self.batch_norm(x)


def MLP(channels, bias=True, bn_momentum=0.1):
    """core/common_modules/base_modules.py MLP: Seq of Seq(Linear with bias, FastBatchNorm1d, LeakyReLU(0.2)), numbered from 0"""
    return nn.Sequential(*[nn.Sequential(nn.Linear(channels[i - 1], channels[i], bias=bias), _BN(channels[i], bn_momentum),
                                         nn.LeakyReLU(0.2)) for i in range(1, len(channels))])


def FC(widths, bn_momentum):
    return nn.Sequential(*[nn.Sequential(nn.Linear(widths[i - 1], widths[i], bias=False), _BN(widths[i], bn_momentum),
                                         nn.LeakyReLU(0.2)) for i in range(1, len(widths))])


class Unet(nn.Module):
    """UnetMSparseConv3d; forward(pos, batch, x, grid_size) -> (per-point features, the voxel tables)"""

    def __init__(self, backbone, pointnet_nn=None, pre_mlp_nn=None, post_mlp_nn=(64, 64, 32), add_pos=False, add_pre_x=False,
                 aggr=None):
        super().__init__()
        self.unet = UNet(backbone)
        self.pre_mlp = MLP(pre_mlp_nn) if pre_mlp_nn is not None else nn.Identity()
        self.pointnet = MLP(pointnet_nn) if pointnet_nn is not None else nn.Identity()
        self.post_mlp = MLP(list(post_mlp_nn))
        self.add_pos, self.add_pre_x, self.aggr = add_pos, add_pre_x, aggr

    def forward(self, pos, batch, x, grid_size):
        if self.add_pos:
            x = self.pointnet(torch.cat([x, pos - pos.mean(0)], 1))
        else:
            x = self.pointnet(x)
        pre_x = x
        coords, vb, vpos, vx, cluster, upi = voxelize(pos, batch, grid_size, x, self.aggr)
        vx = self.pre_mlp(vx)
        C = torch.cat([coords, vb.unsqueeze(1)], 1).int()
        out = self.unet(vx, C)[cluster]
        if self.add_pos:
            out = torch.cat([out, pos - pos.mean(0)], 1)
        if self.add_pre_x:
            out = torch.cat([out, pre_x], 1)
        return self.post_mlp(out), dict(coords=coords, cluster=cluster, unique_pos_indices=upi)


class MSNet(nn.Module):
    """MS_SparseConv3d (shared=False: one Unet per scale under `unet.<i>`), MS_SparseConv3d_Shared (mode "cat") and
    MS_SparseConv3d_Shared_Pool (mode "max" / "mean"); num_classes: MS_SparseConvModel's `head`"""

    def __init__(self, backbone, grid_size, mlp_nn, bn_momentum=0.02, shared=True, mode="cat", normalize_feature=True,
                 num_classes=None, **unet_args):
        super().__init__()
        self.grid_size, self.shared, self.mode, self.normalize_feature = list(grid_size), shared, mode, normalize_feature
        if shared:
            self.unet = Unet(backbone, **unet_args)
        else:
            self.unet = nn.ModuleList(Unet(backbone, **unet_args) for _ in self.grid_size)
        self.FC_layer = FC(mlp_nn, bn_momentum)
        if num_classes is not None:
            self.head = nn.Sequential(nn.Linear(mlp_nn[-1], num_classes))

    def apply_nn(self, pos, batch, x):
        outs, tables = [], []
        for i, gs in enumerate(self.grid_size):
            net = self.unet if self.shared else self.unet[i]
            o, t = net(pos, batch, x, gs)
            outs.append(o)
            tables.append(t)
        fused, hs = scale_fuse(outs, self.mode)
        out = self.FC_layer(fused)
        if self.normalize_feature:
            out = normalize(out)
        return out, hs, fused, tables


def pdist(A, B):
    return torch.sqrt(torch.sum((A.unsqueeze(1) - B.unsqueeze(0)).pow(2), 2) + 1e-7)


def hardest_negative_loss(F0, F1, pairs, sel0, sel1, pos_sel, pos_thresh, neg_thresh, num_pos, parts=None):
    """core/losses/metric_losses.py ContrastiveHardestNegativeLoss with the drawn selections given"""
    N0, N1 = len(F0), len(F1)
    hash_seed = max(N0, N1)
    sample = pairs[pos_sel] if len(pairs) > num_pos else pairs
    i0, i1 = sample[:, 0].long(), sample[:, 1].long()
    posF0, posF1 = F0[i0], F1[i1]
    D01, D10 = pdist(posF0, F1[sel1]), pdist(posF1, F0[sel0])
    D01min, D01ind = D01.min(1)
    D10min, D10ind = D10.min(1)
    D01ind, D10ind = sel1[D01ind], sel0[D10ind]
    keys = (pairs[:, 0] + pairs[:, 1] * hash_seed).long()
    mask0 = ~torch.isin(i0 + D01ind * hash_seed, keys)
    mask1 = ~torch.isin(D10ind + i1 * hash_seed, keys)
    pos_arg = (posF0 - posF1).pow(2).sum(1) - pos_thresh
    neg0 = torch.relu(neg_thresh - D01min[mask0]).pow(2)
    neg1 = torch.relu(neg_thresh - D10min[mask1]).pow(2)
    if parts is not None:
        s01, s10 = torch.sort(D01.pow(2), 1)[0], torch.sort(D10.pow(2), 1)[0]
        parts.append(dict(relu_args=torch.cat([pos_arg, neg_thresh - D01min[mask0], neg_thresh - D10min[mask1]]),
                          gap=torch.cat([s01[:, 1] - s01[:, 0], s10[:, 1] - s10[:, 0]])))
    return torch.relu(pos_arg).mean() + (neg0.mean() + neg1.mean()) / 2
