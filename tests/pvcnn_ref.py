"""Plain-torch restatement of the point-voxel operations ("Point-voxel ops (PVCNN)") and of the PVCNN network,
on top of the sparse-convolution restatement tests/sparseconv_ref.py.

Coordinates stay fp32 (the contract does its division and floor in fp32, so the integer tables are the same in every
evaluation); features, weights and parameters take the dtype asked for, float32 or float64, on any device.

    voxelise     index_add_ of the point rows into their voxel rows, divided by the count (0 rows for empty voxels)
    devoxelise   (F[idx8.clamp(0)] * w[..., None]).sum(1): the (N, 8, C) gather this project's kernel never writes
"""
import torch
import torch.nn as nn

import sparseconv_ref as ref


def quantize(pc, s):
    """(N, 4) float [x, y, z, batch] -> int32 [floor(x / s) * s, floor(y / s) * s, floor(z / s) * s, batch]"""
    return torch.cat([torch.floor(pc[:, :3] / s).int() * s, pc[:, 3:].int()], 1)


def voxel_set(q):
    """the distinct rows of q, ascending (batch, x, y, z)"""
    return ref.down_coords(q, 1).to(q.device)


def lookup1(q, C):
    """(N,) int32: the row of C equal to q, -1 where absent"""
    return ref.lookup(q, (0, 0, 0), C).int()


def lookup8(q, s, C):
    """(N, 8) int32: the rows of C at q + {0, s}^3, x slowest, z fastest"""
    return torch.stack([ref.lookup(q, o, C) for o in ref.offsets(2, s)], 1).int()


def trilinear_weights(pc, idx8, s, dtype=torch.float32, nearest=False):
    """-> (weights (N, 8) of dtype, idx8 as used): torchsparse's calc_ti_weights followed by the `nearest` rule"""
    p = pc[:, :3].to(dtype)
    pf = (torch.floor(pc[:, :3] / s) * s).to(dtype)
    pn = pf + s
    a = torch.stack([pn - p, p - pf], -1)  # (N, axis, d)
    w = torch.stack([a[:, 0, k >> 2] * a[:, 1, (k >> 1) & 1] * a[:, 2, k & 1] for k in range(8)], 1)
    w = w / float(s) ** 3
    w = torch.where(idx8 < 0, torch.zeros_like(w), w)
    w = w / (w.sum(1, keepdim=True) + 1e-8)
    if nearest:
        w = w.clone()
        w[:, 1:] = 0.0
        idx8 = idx8.clone()
        idx8[:, 1:] = -1
    return w, idx8


def counts(idx, n_voxels):
    hit = idx[idx >= 0].long()
    return torch.bincount(hit, minlength=n_voxels).int()


def voxelize(Fx, idx, n_voxels):
    """mean of the point rows per voxel; points with idx -1 are dropped, a voxel without a point gets zeros"""
    hit = torch.nonzero(idx >= 0).squeeze(1)
    out = torch.zeros((n_voxels, Fx.shape[1]), dtype=Fx.dtype, device=Fx.device).index_add_(0, idx[hit].long(), Fx[hit])
    return out / counts(idx, n_voxels).clamp(min=1).to(Fx.dtype).unsqueeze(1)


def devoxelize(Fx, idx8, w):
    return (Fx[idx8.clamp(min=0).long()] * w.to(Fx.dtype).unsqueeze(-1)).sum(1)


# ---------------------------------------------------------------------------------------------------------- the network
class RefPoints(object):
    """the PointTensor of the restatement: tables per tensor stride, shared by derived tensors"""

    def __init__(self, Fx, C, tables=None):
        self.F, self.C = Fx, C
        self.tables = {} if tables is None else tables

    def like(self, Fx):
        return RefPoints(Fx, self.C, self.tables)


def initial_voxelize(z, init_res, after_res):
    z.C = torch.cat([(z.C[:, :3] * init_res) / after_res, z.C[:, -1].view(-1, 1)], 1)
    q = quantize(z.C, 1)
    C = voxel_set(q)
    z.tables[("idx", 1)] = lookup1(q, C)
    return ref.RefTensor(voxelize(z.F, z.tables[("idx", 1)], len(C)), C, 1)


def point_to_voxel(x, z):
    if ("idx", x.s) not in z.tables:
        z.tables[("idx", x.s)] = lookup1(quantize(z.C, x.s), x.C)
    return ref.RefTensor(voxelize(z.F, z.tables[("idx", x.s)], len(x.C)), x.C, x.s, x.sets)


def voxel_to_point(x, z, nearest=False):
    if ("idx8", x.s) not in z.tables:
        idx8 = lookup8(quantize(z.C, x.s), x.s, x.C)
        w, idx8 = trilinear_weights(z.C, idx8, x.s, x.F.dtype, nearest)
        z.tables[("idx8", x.s)], z.tables[("w", x.s)] = idx8, w
    return z.like(devoxelize(x.F, z.tables[("idx8", x.s)], z.tables[("w", x.s)]))


def _conv(inc, outc, ks, stride=1, transpose=False):
    return ref.Conv3d(inc, outc, kernel_size=ks, stride=stride, transposed=transpose)


class BasicConvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, transpose=False):
        super().__init__()
        self.net = nn.Sequential(_conv(inc, outc, ks, stride, transpose), ref.BatchNorm(outc), ref.ReLU())

    def forward(self, x):
        return self.net(x)


class ResidualBlock(nn.Module):
    def __init__(self, inc, outc, ks=3):
        super().__init__()
        self.net = nn.Sequential(_conv(inc, outc, ks), ref.BatchNorm(outc), ref.ReLU(), _conv(outc, outc, ks), ref.BatchNorm(outc))
        self.downsample = nn.Sequential() if inc == outc else nn.Sequential(_conv(inc, outc, 1), ref.BatchNorm(outc))

    def forward(self, x):
        return x.like(torch.relu(self.net(x).F + self.downsample(x).F))


class Net(nn.Module):
    """PVCNN of modules/PVCNN/pvcnn.py with its attribute names (state_dict keys); dropout left out (p = 0)"""

    def __init__(self, cr, vres, num_features, num_classes):
        super().__init__()
        self.vres = vres
        cs = [int(cr * x) for x in [32, 32, 64, 128, 256, 256, 128, 96, 96]]
        self.stem = nn.Sequential(_conv(num_features, cs[0], 3), ref.BatchNorm(cs[0]), ref.ReLU(),
                                  _conv(cs[0], cs[0], 3), ref.BatchNorm(cs[0]), ref.ReLU())
        for i in range(4):
            setattr(self, "stage%d" % (i + 1), nn.Sequential(BasicConvolutionBlock(cs[i], cs[i], 2, 2),
                                                             ResidualBlock(cs[i], cs[i + 1]), ResidualBlock(cs[i + 1], cs[i + 1])))
            setattr(self, "up%d" % (i + 1), nn.ModuleList([
                BasicConvolutionBlock(cs[4 + i], cs[5 + i], 2, 2, transpose=True),
                nn.Sequential(ResidualBlock(cs[5 + i] + cs[3 - i], cs[5 + i]), ResidualBlock(cs[5 + i], cs[5 + i]))]))
        self.classifier = nn.Sequential(nn.Linear(cs[8], num_classes))
        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cs[0], cs[4]), nn.BatchNorm1d(cs[4]), nn.ReLU()),
            nn.Sequential(nn.Linear(cs[4], cs[6]), nn.BatchNorm1d(cs[6]), nn.ReLU()),
            nn.Sequential(nn.Linear(cs[6], cs[8]), nn.BatchNorm1d(cs[8]), nn.ReLU())])

    def forward(self, Fx, C):
        """C (N, 4) float [x, y, z, batch]"""
        z = RefPoints(Fx, C.float())
        x0 = self.stem(initial_voxelize(z, 1.0, self.vres))
        z0 = voxel_to_point(x0, z)
        x1 = self.stage1(point_to_voxel(x0, z0))
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        z1 = voxel_to_point(x4, z0)
        z1.F = z1.F + self.point_transforms[0](z0.F)
        y1 = self.up1[1](ref.cat(self.up1[0](point_to_voxel(x4, z1)), x3))
        y2 = self.up2[1](ref.cat(self.up2[0](y1), x2))
        z2 = voxel_to_point(y2, z1)
        z2.F = z2.F + self.point_transforms[1](z1.F)
        y3 = self.up3[1](ref.cat(self.up3[0](point_to_voxel(y2, z2)), x1))
        y4 = self.up4[1](ref.cat(self.up4[0](y3), x0))
        z3 = voxel_to_point(y4, z2)
        z3.F = z3.F + self.point_transforms[2](z2.F)
        return self.classifier(z3.F)
