"""PVCNN (SPVCNN): the point-voxel network of the torchsparse backend on MI355X.

Mirrors torch_points3d/modules/PVCNN/utils.py (`initial_voxelize`, `point_to_voxel`, `voxel_to_point`), blocks.py
(`BasicConvolutionBlock`, `BasicDeconvolutionBlock`, `ResidualBlock`) and pvcnn.py (`PVCNN`) together with torchsparse's
`PointTensor`: same signatures, caching rules, side effects and attribute names, hence state_dict keys.  The voxel side
is this project's sparse convolution (sparseconv.py); the three point-voxel functions are autograd Functions over
csrc/pointvoxel.hip ("Point-voxel ops (PVCNN)").

A voxelisation is the per-voxel mean of the point features (0 for a voxel without a point), a devoxelisation the
trilinear interpolation over the 8 voxels around a point with the weights renormalised over the corners that exist.
The tables (point -> voxel row, point -> 8 corner rows, weights, counts) depend on geometry only: they are built once per
tensor stride, cached on the PointTensor under the reference's attribute names and shared by every tensor derived from
it, and so are their inverted forms (`inverted`), which the voxel-side sums read -- a backward pass builds no table.
Gradients flow to features only.  There is no CPU path.
"""
import torch
import torch.nn as nn

from . import _lib
from . import sparseconv as sc
from .kpconv import _require_gpu
from .sparseconv import SparseTensor

__all__ = ["PointTensor", "initial_voxelize", "point_to_voxel", "voxel_to_point", "BasicConvolutionBlock",
           "BasicDeconvolutionBlock", "ResidualBlock", "PVCNN", "pvcnn"]

LONG_RUN = 64  # PV_LONG_RUN of csrc/pointvoxel.hip: a longer run of slots is summed in 16 pieces


class PointTensor(object):
    """torchsparse's PointTensor: F (N, C) fp32, C (N, 4) float [x, y, z, batch]; `idx_query` / `weights` (devoxelisation)
    and `additional_features["idx_query" | "counts"]` (voxelisation) are dicts keyed by tensor stride, `inverted` holds
    the inverted tables keyed by ("voxelize" | "devoxelize", stride); all are shared by reference between derived tensors."""

    def __init__(self, feats, coords, idx_query=None, weights=None):
        self.F = feats
        self.C = coords
        self.idx_query = idx_query if idx_query is not None else {}
        self.weights = weights if weights is not None else {}
        self.additional_features = {"idx_query": {}, "counts": {}}
        self.inverted = {}

    def to(self, device):
        self.F = self.F.to(device)
        self.C = self.C.to(device)
        return self

    def _derived(self, feats):
        out = PointTensor(feats, self.C, idx_query=self.idx_query, weights=self.weights)
        out.additional_features = self.additional_features
        out.inverted = self.inverted
        return out


# ------------------------------------------------------------------------------------------------------ kernel launches
def _quantize(pc, s):
    """(N, 4) float [x, y, z, batch] -> (N, 4) int32 [floor(x / s) * s, floor(y / s) * s, floor(z / s) * s, batch]"""
    dev = pc.device
    q = torch.empty(pc.shape, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_pv_quantize_f32", _lib.ptr(pc), pc.shape[0], int(s), _lib.ptr(q), _lib.stream_ptr(dev))
    return q


def _trilinear(pc, idx8, n_voxels, s, nearest):
    dev = pc.device
    w = torch.empty(idx8.shape, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_pv_trilinear_f32", _lib.ptr(pc), _lib.ptr(idx8), pc.shape[0], int(n_voxels), int(s), int(bool(nearest)),
                  _lib.ptr(w), _lib.stream_ptr(dev))
    return w


def _invert(table, n_voxels):
    """(start (n_voxels + 1), order (slots)) int32: per voxel row the slots p * K + k that point at it, ascending"""
    dev = table.device
    N, K = table.shape
    start = torch.empty((n_voxels + 1,), dtype=torch.int32, device=dev)
    order = torch.empty((N * K,), dtype=torch.int32, device=dev)
    nbytes = _lib.load().tp3d_pv_invert_workspace_bytes(N, K)
    ws = _lib.workspace("pv_invert", nbytes, dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_pv_invert_i32", _lib.ptr(table), N, K, int(n_voxels), _lib.ptr(start), _lib.ptr(order), _lib.ptr(ws), nbytes,
                  _lib.stream_ptr(dev))
    return start, order


def _gather(src, table, w, scale):
    dev = src.device
    out = torch.empty((table.shape[0], src.shape[1]), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_pv_gather_f32", _lib.ptr(src), _lib.ptr(table), _lib.ptr(w), _lib.ptr(scale), table.shape[0], table.shape[1],
                  src.shape[0], src.shape[1], _lib.ptr(out), _lib.stream_ptr(dev))
    return out


def _runsum(src, start, order, w, scale, K):
    dev = src.device
    n_voxels = start.shape[0] - 1
    out = torch.empty((n_voxels, src.shape[1]), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_pv_runsum_f32", _lib.ptr(src), _lib.ptr(start), _lib.ptr(order), _lib.ptr(w), _lib.ptr(scale), n_voxels, K,
                  src.shape[0], src.shape[1], _lib.ptr(out), _lib.stream_ptr(dev))
    return out


class _Voxelize(torch.autograd.Function):
    """out[v] = mean of feats over the points of voxel v (idx (N, 1)); backward: d_feats[p] = dy[idx[p]] / count"""

    @staticmethod
    def forward(ctx, feats, idx, start, order, inv_count):
        feats = feats.detach().float().contiguous()
        ctx.save_for_backward(idx, inv_count)
        return _runsum(feats, start, order, None, inv_count, 1)

    @staticmethod
    def backward(ctx, dy):
        idx, inv_count = ctx.saved_tensors
        return _gather(dy.float().contiguous(), idx, None, inv_count), None, None, None, None


class _Devoxelize(torch.autograd.Function):
    """out[p] = sum_k w[p, k] feats[idx8[p, k]]; backward: d_feats[v] = sum over the slots of v of w * dy[p]"""

    @staticmethod
    def forward(ctx, feats, idx8, weights, start, order):
        feats = feats.detach().float().contiguous()
        ctx.save_for_backward(weights, start, order)
        return _gather(feats, idx8, weights, None)

    @staticmethod
    def backward(ctx, dy):
        weights, start, order = ctx.saved_tensors
        return _runsum(dy.float().contiguous(), start, order, weights, None, 8), None, None, None, None


def _voxelize_tables(z, q, target, s):
    """point -> voxel row table of stride s against the coordinate set `target`, its counts and inverted form, cached"""
    idx = sc._search(q, q.shape[0], 1, 1, 1, target)
    start, order = _invert(idx, target.n)
    counts = start[1:] - start[:-1]
    z.additional_features["idx_query"][s] = idx.view(-1)
    z.additional_features["counts"][s] = counts
    z.inverted[("voxelize", s)] = (start, order, 1.0 / counts.clamp(min=1).float())


def _voxelize(z, s):
    idx = z.additional_features["idx_query"][s]
    start, order, inv_count = z.inverted[("voxelize", s)]
    return _Voxelize.apply(z.F, idx.view(-1, 1), start, order, inv_count)


# --------------------------------------------------------------------------------------- modules/PVCNN/utils.py
def initial_voxelize(z, init_res, after_res):
    """z: PointTensor -> SparseTensor of tensor stride 1 on the voxels floor(z.C * init_res / after_res), rows ascending
    (batch, x, y, z); z.C is replaced by the scaled float coordinates."""
    _require_gpu(z.F, z.C)
    new_float_coord = torch.cat([(z.C[:, :3] * init_res) / after_res, z.C[:, -1].view(-1, 1)], 1).float().contiguous()
    q = _quantize(new_float_coord, 1)
    voxels = sc._build_set(q, 1, 1)  # down = 1: the distinct coordinates
    _voxelize_tables(z, q, voxels, 1)
    z.C = new_float_coord
    return SparseTensor(_voxelize(z, 1), voxels.coords, 1, {1: voxels}, {})


def point_to_voxel(x, z):
    """x: SparseTensor, z: PointTensor -> SparseTensor on x's voxels with the per-voxel mean of z.F"""
    _require_gpu(x.C, z.F, z.C)
    if z.additional_features is None or z.additional_features.get("idx_query") is None \
            or z.additional_features["idx_query"].get(x.s) is None:
        target = x._set(x.s)
        if target is None:
            raise RuntimeError("point_to_voxel: no coordinate set of tensor stride %d" % x.s)
        _voxelize_tables(z, _quantize(z.C.float().contiguous(), x.s), target, x.s)
    return SparseTensor(_voxelize(z, x.s), x.C, x.s, x.cmaps, x.kmaps, x.clouds)


def voxel_to_point(x, z, nearest=False):
    """x: SparseTensor, z: PointTensor -> PointTensor with x.F interpolated trilinearly at the points"""
    _require_gpu(x.F, x.C, z.C)
    if z.idx_query is None or z.weights is None or z.idx_query.get(x.s) is None or z.weights.get(x.s) is None:
        target = x._set(x.s)
        if target is None:
            raise RuntimeError("voxel_to_point: no coordinate set of tensor stride %d" % x.s)
        pc = z.C.float().contiguous()
        q = _quantize(pc, x.s)
        idx8 = sc._search(q, q.shape[0], 2, x.s, 1, target)
        weights = _trilinear(pc, idx8, target.n, x.s, nearest)
        z.idx_query[x.s] = idx8
        z.weights[x.s] = weights
        z.inverted[("devoxelize", x.s)] = _invert(idx8, target.n)
    start, order = z.inverted[("devoxelize", x.s)]
    return z._derived(_Devoxelize.apply(x.F, z.idx_query[x.s], z.weights[x.s], start, order))


# -------------------------------------------------------------------------------------- modules/PVCNN/blocks.py
def _conv3d(inc, outc, kernel_size=3, stride=1, dilation=1, transpose=False):
    """torchsparse's spnn.Conv3d(..., transpose=...) on this project's sparse convolution"""
    return sc.Conv3d(inc, outc, kernel_size=kernel_size, stride=stride, dilation=dilation, transposed=transpose)


class BasicConvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(_conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), sc.BatchNorm(outc),
                                 sc.ReLU(True))

    def forward(self, x):
        return self.net(x)


class BasicDeconvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1):
        super().__init__()
        self.net = nn.Sequential(_conv3d(inc, outc, kernel_size=ks, stride=stride, transpose=True), sc.BatchNorm(outc),
                                 sc.ReLU(True))

    def forward(self, x):
        return self.net(x)


class ResidualBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(_conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), sc.BatchNorm(outc),
                                 sc.ReLU(True), _conv3d(outc, outc, kernel_size=ks, dilation=dilation, stride=1),
                                 sc.BatchNorm(outc))
        self.downsample = (nn.Sequential() if (inc == outc and stride == 1) else
                           nn.Sequential(_conv3d(inc, outc, kernel_size=1, dilation=1, stride=stride), sc.BatchNorm(outc)))
        self.relu = sc.ReLU(True)

    def forward(self, x):
        return self.relu(self.net(x) + self.downsample(x))


# --------------------------------------------------------------------------------------- modules/PVCNN/pvcnn.py
class PVCNN(nn.Module):
    """forward: PointTensor, or an object with x, pos, batch -> (N, num_classes) scores in the input's point order"""

    def __init__(self, option, model_type, dataset, modules):
        super().__init__()
        cr = option.cr
        self.vres = option.vres
        self.num_classes = dataset.num_classes
        self.num_features = dataset.feature_dimension

        cs = [32, 32, 64, 128, 256, 256, 128, 96, 96]
        cs = [int(cr * x) for x in cs]

        self.stem = nn.Sequential(_conv3d(self.num_features, cs[0], kernel_size=3, stride=1), sc.BatchNorm(cs[0]), sc.ReLU(True),
                                  _conv3d(cs[0], cs[0], kernel_size=3, stride=1), sc.BatchNorm(cs[0]), sc.ReLU(True))
        for i in range(4):
            setattr(self, "stage%d" % (i + 1), nn.Sequential(
                BasicConvolutionBlock(cs[i], cs[i], ks=2, stride=2, dilation=1),
                ResidualBlock(cs[i], cs[i + 1], ks=3, stride=1, dilation=1),
                ResidualBlock(cs[i + 1], cs[i + 1], ks=3, stride=1, dilation=1)))
        for i in range(4):
            setattr(self, "up%d" % (i + 1), nn.ModuleList([
                BasicDeconvolutionBlock(cs[4 + i], cs[5 + i], ks=2, stride=2),
                nn.Sequential(ResidualBlock(cs[5 + i] + cs[3 - i], cs[5 + i], ks=3, stride=1, dilation=1),
                              ResidualBlock(cs[5 + i], cs[5 + i], ks=3, stride=1, dilation=1))]))
        self.classifier = nn.Sequential(nn.Linear(cs[8], self.num_classes))
        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cs[0], cs[4]), nn.BatchNorm1d(cs[4]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[4], cs[6]), nn.BatchNorm1d(cs[6]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[6], cs[8]), nn.BatchNorm1d(cs[8]), nn.ReLU(True))])

        self.weight_initialization()
        self.dropout = nn.Dropout(0.3, True)
        self.loss_names = ["loss_seg"]

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    @staticmethod
    def _input(data):
        """models/segmentation/pvcnn.py set_input: coordinates are cat([pos, batch]), float"""
        if isinstance(data, PointTensor):
            return PointTensor(data.F, data.C.float())
        batch = data.batch.unsqueeze(-1) if data.batch.dim() == 1 else data.batch
        return PointTensor(data.x, torch.cat([data.pos.float(), batch.float()], -1))

    def forward(self, x):
        z = self._input(x)

        x0 = initial_voxelize(z, 1.0, self.vres)

        x0 = self.stem(x0)
        z0 = voxel_to_point(x0, z, nearest=False)

        x1 = point_to_voxel(x0, z0)
        x1 = self.stage1(x1)
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        z1 = voxel_to_point(x4, z0)
        z1.F = z1.F + self.point_transforms[0](z0.F)

        y1 = point_to_voxel(x4, z1)
        y1.F = self.dropout(y1.F)
        y1 = self.up1[0](y1)
        y1 = sc.cat(y1, x3)
        y1 = self.up1[1](y1)

        y2 = self.up2[0](y1)
        y2 = sc.cat(y2, x2)
        y2 = self.up2[1](y2)
        z2 = voxel_to_point(y2, z1)
        z2.F = z2.F + self.point_transforms[1](z1.F)

        y3 = point_to_voxel(y2, z2)
        y3.F = self.dropout(y3.F)
        y3 = self.up3[0](y3)
        y3 = sc.cat(y3, x1)
        y3 = self.up3[1](y3)

        y4 = self.up4[0](y3)
        y4 = sc.cat(y4, x0)
        y4 = self.up4[1](y4)
        z3 = voxel_to_point(y4, z2)
        z3.F = z3.F + self.point_transforms[2](z2.F)

        self.output = self.classifier(z3.F)
        return self.output


class _Option(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def pvcnn(cr=1.0, vres=0.05, num_features=3, num_classes=13):
    """PVCNN without the option objects (conf/models/segmentation/pvcnn.yaml: cr 1, vres = the dataset's grid size)"""
    return PVCNN(_Option(cr=cr, vres=vres), "PVCNN", _Option(num_classes=num_classes, feature_dimension=num_features), None)
