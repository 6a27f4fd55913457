"""Generator of tests/golden/pvcnn.npz and pvcnn_config.json: the REFERENCE's own PVCNN on the CPU.

torch_points3d/modules/PVCNN/{pvcnn,blocks,utils}.py import torchsparse, which cannot be installed next to this code.  This
script places dense-torch stand-ins in sys.modules for `torchsparse`, `torchsparse.nn`, `torchsparse.nn.functional`,
`torchsparse.sparse_tensor`, `torchsparse.point_tensor`, `torchsparse.utils.kernel_region` and `torchsparse.utils.helpers`
(which must export `torch`: the reference's utils.py gets it through `from torchsparse.utils.helpers import *`), then runs
the reference's own `PVCNN` -- its `initial_voxelize`, `point_to_voxel`, `voxel_to_point`, blocks and forward -- in train
mode with cr = 0.125, vres = 0.5, 5 input features, 7 classes and dropout.p = 0: state_dict, inputs, logits, running
statistics after the step, input and parameter gradients for a stored cotangent, an eval-mode pass, and the same in
float64 (`f64/`).  To stay inside the size limit of a committed file the initial parameters are multiples of 1 / 64 stored
exactly as int8 (`state_q/`), and a parameter gradient of more than 512 elements is stored as every 31st element of its
flat form.  The stand-ins restate torchsparse 1.x FROM MEMORY (hash = an injective key, hash query = sorted
search, spvoxelize = per-voxel mean, calc_ti_weights / spdevoxelize = trilinear interpolation, KernelRegion(2, s)
offsets {0, s} with x slowest and z fastest, Conv3d = the dense equivalents of tests/sparseconv_ref.py); torchsparse
itself was never run.  Data only: the stand-ins live here, never in the fixture.

Safety conditions (asserted here and again in tests/test_pvcnn_cpu.py): every coordinate of pos / vres is at least 1e-3
from an integer, and every ReLU input is at least KINK_MARGIN from 0 -- re-seeded until that holds.

    python tests/golden/make_golden_pvcnn.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import sparseconv_ref as dense  # noqa: E402

KINK_MARGIN = 5e-5
COORD_MARGIN = 1e-3
STATE_SCALE = 64     # every initial parameter is a multiple of 1 / 64 in [-127 / 64, 127 / 64]: stored exactly as int8
PGRAD_STRIDE = 31    # a parameter gradient of more than PGRAD_FULL elements is stored as its flat [::PGRAD_STRIDE] samples
PGRAD_FULL = 512     # (the 340 000 parameters' gradients in fp32 and float64 would not fit a committed file)
CONFIG = dict(cr=0.125, vres=0.5, num_features=5, num_classes=7, points=[720, 700])
_state = {"dtype": torch.float32, "relu_min": float("inf"), "check": True}


class Unsafe(Exception):
    pass


def _saw_relu_input(t):
    m = float(t.detach().abs().min())
    _state["relu_min"] = min(_state["relu_min"], m)
    if _state["check"] and m < KINK_MARGIN:
        raise Unsafe("ReLU input %.3g from 0" % m)


# ------------------------------------------------------------------------------------------------- torchsparse stand-ins
class SparseTensor(dense.RefTensor):
    def __init__(self, feats, coords, stride=1):
        super().__init__(feats, coords, stride)
        self.kernel_maps = {}

    coord_maps = property(lambda self: self.sets, lambda self, v: setattr(self, "sets", v))

    def check(self):
        assert torch.unique(self.C, dim=0).shape[0] == self.C.shape[0]

    def like(self, Fx):
        t = SparseTensor(Fx, self.C, self.s)
        t.sets = self.sets
        return t

    def __add__(self, other):
        return self.like(self.F + other.F)


class PointTensor(object):
    def __init__(self, feat, coords, idx_query=None, weights=None):
        self.F, self.C = feat, coords
        self.idx_query = idx_query if idx_query is not None else {}
        self.weights = weights if weights is not None else {}
        self.additional_features = {"idx_query": {}, "counts": {}}


class Conv3d(dense.Conv3d):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transpose=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, transposed=transpose)

    def forward(self, x):
        out = super().forward(x)
        t = SparseTensor(out.F, out.C, out.s)
        t.sets = out.sets
        return t


class ReLU(torch.nn.Module):
    def __init__(self, inplace=True):
        super().__init__()

    def forward(self, x):
        _saw_relu_input(x.F)
        return x.like(torch.relu(x.F))


_R, _O = 1 << 16, 1 << 15


def sphash(coords, offsets=None):
    """an injective int64 key of (x, y, z, batch) rows; with offsets (K, 3): (K, N)"""
    c = coords.long()

    def key(xyz):
        return ((c[:, 3] * _R + xyz[:, 0] + _O) * _R + xyz[:, 1] + _O) * _R + xyz[:, 2] + _O

    if offsets is None:
        return key(c[:, :3])
    return torch.stack([key(c[:, :3] + o.long()) for o in offsets], 0)


def sphashquery(queries, references):
    ks, order = torch.sort(references)
    flat = queries.reshape(-1)
    pos = torch.searchsorted(ks, flat).clamp(max=ks.numel() - 1)
    out = torch.where(ks[pos] == flat, order[pos], torch.full_like(pos, -1))
    return out.reshape(queries.shape)


def spcount(idx, n):
    return torch.bincount(idx[idx >= 0].long(), minlength=n).int()


def spvoxelize(feat, idx, cnt):
    hit = torch.nonzero(idx >= 0).squeeze(1)
    out = torch.zeros((cnt.shape[0], feat.shape[1]), dtype=feat.dtype).index_add_(0, idx[hit].long(), feat[hit])
    return out / cnt.clamp(min=1).to(feat.dtype).unsqueeze(1)


def spdevoxelize(feat, idx, w):
    return (feat[idx.clamp(min=0).long()] * w.to(feat.dtype).unsqueeze(-1)).sum(1)


def calc_ti_weights(coords, idx_query, scale=1.0):
    """(8, N): in the dtype of the pass (the reference computes them in the coordinates' fp32)"""
    dt = _state["dtype"]
    with torch.no_grad():
        p = coords[:, :3]
        pf = (torch.floor(p / scale) * scale if scale != 1 else torch.floor(p)).to(dt)
        p = p.to(dt)
        pc = pf + scale
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        xf, yf, zf = pf[:, 0], pf[:, 1], pf[:, 2]
        xc, yc, zc = pc[:, 0], pc[:, 1], pc[:, 2]
        w = torch.stack([(xc - x) * (yc - y) * (zc - z), (xc - x) * (yc - y) * (z - zf), (xc - x) * (y - yf) * (zc - z),
                         (xc - x) * (y - yf) * (z - zf), (x - xf) * (yc - y) * (zc - z), (x - xf) * (yc - y) * (z - zf),
                         (x - xf) * (y - yf) * (zc - z), (x - xf) * (y - yf) * (z - zf)], 0)
        if scale != 1:
            w = w / scale ** 3
        w[idx_query == -1] = 0
        w = w / (w.sum(0) + 1e-8)
    return w


class KernelRegion(object):
    def __init__(self, kernel_size=3, tensor_stride=1, dilation=1):
        assert kernel_size == 2 and dilation == 1
        self.ts = tensor_stride

    def get_kernel_offset(self):
        r = [0, self.ts]
        return torch.tensor([[a, b, c] for a in r for b in r for c in r], dtype=torch.int32)  # x slowest, z fastest


def install_torchsparse():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    ts = mod("torchsparse", SparseTensor=SparseTensor, PointTensor=PointTensor,
             cat=lambda ts_: ts_[0].like(torch.cat([t.F for t in ts_], 1)))
    ts.nn = mod("torchsparse.nn", Conv3d=Conv3d, BatchNorm=dense.BatchNorm, ReLU=ReLU)
    ts.nn.functional = mod("torchsparse.nn.functional", sphash=sphash, sphashquery=sphashquery, spcount=spcount,
                           spvoxelize=spvoxelize, spdevoxelize=spdevoxelize, calc_ti_weights=calc_ti_weights)
    mod("torchsparse.sparse_tensor", SparseTensor=SparseTensor)
    mod("torchsparse.point_tensor", PointTensor=PointTensor)
    ts.utils = mod("torchsparse.utils")
    mod("torchsparse.utils.kernel_region", KernelRegion=KernelRegion, __all__=["KernelRegion"])
    mod("torchsparse.utils.helpers", torch=torch, __all__=["torch"])


def load_reference():
    mg.install_stubs()
    install_torchsparse()
    from torch_points3d.modules.PVCNN import pvcnn
    return pvcnn


# ------------------------------------------------------------------------------------------------------------- the case
def cloud(g):
    """two clouds on thin shells of radius 4.5 and 3.5 voxels (several points per voxel: the fewer voxel rows, the fewer
    re-seeds the ReLU margin costs) plus a dense blob; every pos / vres sits in [0.05, 0.95] of its voxel"""
    vres = CONFIG["vres"]
    pos, batch = [], []
    for b, n in enumerate(CONFIG["points"]):
        d = torch.randn(n, 3, generator=g)
        d = d / d.norm(dim=1, keepdim=True)
        p = d * ((4.5 if b == 0 else 3.5) + torch.rand(n, 1, generator=g))
        p[: n // 6] = torch.rand(n // 6, 3, generator=g) * 3.0 - 1.5  # the blob: several points per voxel, full corners
        cell = torch.floor(p) + 0.05 + 0.9 * torch.rand(n, 3, generator=g)
        pos.append(cell * vres)
        batch.append(torch.full((n,), b))
    pos, batch = torch.cat(pos), torch.cat(batch)
    perm = torch.randperm(len(pos), generator=g)
    return pos[perm].contiguous(), batch[perm].contiguous()


def coord_margin(pos, vres):
    v = pos / vres
    return float((v - torch.round(v)).abs().min())


def init(module, g):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() > 1:
                v = torch.randn(p.shape, generator=g) * (0.25 if name.endswith("kernel") else (1.0 / p.shape[1]) ** 0.5)
            elif name.endswith("bn.weight") or (".1.weight" in name and "point_transforms" in name):
                v = 0.5 + torch.rand(p.shape, generator=g)
            elif name.endswith("bn.bias") or (".1.bias" in name and "point_transforms" in name):
                # BatchNorm shifts of 0.75 .. 1.5 either way: every ReLU still passes and blocks a fair share of its inputs,
                # and far fewer of them fall near 0 (with shifts around 0 the margin costs tens of thousands of re-seeds)
                v = (0.75 + 0.75 * torch.rand(p.shape, generator=g)) * (torch.randint(0, 2, p.shape, generator=g) * 2 - 1)
            else:
                v = torch.randn(p.shape, generator=g) * 0.3
            p.copy_(torch.round(v * STATE_SCALE).clamp(-127, 127) / STATE_SCALE)
    return module


def sample(t):
    """what the fixture keeps of a parameter gradient"""
    return t if t.numel() <= PGRAD_FULL else t.reshape(-1)[::PGRAD_STRIDE]


def make(pvcnn):
    opt = mg._Bag(cr=CONFIG["cr"], vres=CONFIG["vres"])
    data = mg._Bag(num_classes=CONFIG["num_classes"], feature_dimension=CONFIG["num_features"])
    net = pvcnn.PVCNN(opt, "PVCNN", data, None)
    net.dropout.p = 0.0
    for m in net.modules():  # the plain ReLUs of point_transforms
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_pre_hook(lambda mod, inp: _saw_relu_input(inp[0]))
    return net


def run(net, x, pos, batch, dtype):
    _state["dtype"] = dtype
    coords = torch.cat([pos, batch.unsqueeze(-1).to(pos.dtype)], -1)  # models/segmentation/pvcnn.py set_input
    return net(mg._Bag(F=x, C=coords))


def case(pvcnn, seed):
    g = torch.Generator().manual_seed(seed)
    pos, batch = cloud(g)
    assert coord_margin(pos, CONFIG["vres"]) >= COORD_MARGIN
    x = torch.randn(len(pos), CONFIG["num_features"], generator=g)
    net = init(make(pvcnn), g).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    _state["relu_min"], _state["check"] = float("inf"), True
    xin = x.clone().requires_grad_(True)
    out = run(net, xin, pos, batch, torch.float32)  # raises Unsafe at the first ReLU input inside the margin
    cot = torch.randn(out.shape, generator=g)
    (out * cot).sum().backward()
    rec = {"pos": pos, "batch": batch, "x": x, "cot": cot, "out": out.detach(), "grad_x": xin.grad,
           "relu_min": np.array([_state["relu_min"]])}
    for k, v in state.items():
        if v.is_floating_point():
            q = torch.round(v * STATE_SCALE)
            assert bool((q / STATE_SCALE == v).all()) and float(q.abs().max()) <= 127
            rec["state_q/" + k] = q.to(torch.int8)
        else:
            rec["state/" + k] = v
    for k, v in net.state_dict().items():
        if "running_" in k:
            rec["after/" + k] = v.clone()
    for k, p in net.named_parameters():
        rec["pgrad/" + k] = sample(p.grad).clone()
    _state["check"] = False  # (eval-mode inputs differ from the train-mode ones; no gradient is taken there)
    with torch.no_grad():
        rec["eval/out"] = run(net.eval(), x, pos, batch, torch.float32)

    n64 = make(pvcnn).double().train()
    n64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    x64 = x.double().requires_grad_(True)
    out64 = run(n64, x64, pos, batch, torch.float64)
    (out64 * cot.double()).sum().backward()
    rec["f64/out"], rec["f64/grad_x"] = out64.detach().numpy(), x64.grad.numpy()
    for k, p in n64.named_parameters():
        rec["f64/pgrad/" + k] = sample(p.grad).clone().numpy()
    with torch.no_grad():
        rec["f64/eval/out"] = run(n64.eval(), x.double(), pos, batch, torch.float64).numpy()
    return rec


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    pvcnn = load_reference()
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    while True:
        try:
            rec = case(pvcnn, seed)
            break
        except Unsafe as e:
            if seed % 50 == 0:
                print("seed %d: %s" % (seed, e), flush=True)
            seed += 1
    rec["seed"] = np.array([seed])
    path = os.path.join(HERE, "pvcnn.npz")
    np.savez_compressed(path, **mg.to_np(rec))
    assert os.path.getsize(path) < 1 << 20
    with open(os.path.join(HERE, "pvcnn_config.json"), "w") as f:
        json.dump(dict(CONFIG, kink_margin=KINK_MARGIN, coord_margin=COORD_MARGIN, state_scale=STATE_SCALE,
                       pgrad_stride=PGRAD_STRIDE, pgrad_full=PGRAD_FULL), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote pvcnn.npz (seed %d, %d arrays, %d bytes, least |ReLU input| %.3g) and pvcnn_config.json"
          % (seed, len(rec), os.path.getsize(path), float(rec["relu_min"][0])))


if __name__ == "__main__":
    main()
