"""Generator of tests/golden/sparseconv.npz and sparseconv_config.json: the REFERENCE's own sparse blocks on the CPU.

torch_points3d/modules/SparseConv3d/nn sets `Conv3d`, `Conv3dTranspose`, `BatchNorm`, `ReLU`, `cat`, `SparseTensor` to
None when no backend imports.  This script assigns dense-torch stand-ins to those globals (the dense equivalents of
DESIGN.md, "Sparse voxel convolution": every convolution scatters to a dense grid and runs F.conv3d /
F.conv_transpose3d) and then runs the reference's own `ResBlock`, `BottleneckBlock`, `ResNetDown` (stride 2), `ResNetUp`
(with a skip) of modules/SparseConv3d/modules.py and one down-down-up-up chain, all in train mode: state_dict, inputs,
outputs, running statistics after the step, input and parameter gradients for a stored cotangent, and the same pass in
float64 (`f64/`).  Re-seeded until every ReLU input is at least KINK_MARGIN away from 0.  The JSON holds the resolved
numbers of applications/conf/sparseconv3d/*.yaml.  Data only: the stand-ins live here, never in the fixture.

    python tests/golden/make_golden_sparseconv.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import sparseconv_ref as dense  # noqa: E402

KINK_MARGIN = 5e-5
_relu_inputs = []


class Unsafe(Exception):
    pass


class _Tensor(dense.RefTensor):
    def like(self, Fx):
        return _Tensor(Fx, self.C, self.s, self.sets)

    def __add__(self, other):  # the reference's blocks write `out += shortcut`
        return self.like(self.F + other.F)


class _Conv3d(dense.Conv3d):
    def forward(self, x):
        out = super().forward(x)
        return _Tensor(out.F, out.C, out.s, out.sets)


class _Conv3dTranspose(_Conv3d):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transpose=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, transposed=True)


class _ReLU(torch.nn.Module):
    def forward(self, x):
        _relu_inputs.append(float(x.F.detach().abs().min()))
        return x.like(torch.relu(x.F))


def load_reference():
    mg.install_stubs()
    import torch_points3d.modules.SparseConv3d.nn as snn
    snn.Conv3d, snn.Conv3dTranspose, snn.BatchNorm, snn.ReLU = _Conv3d, _Conv3dTranspose, dense.BatchNorm, _ReLU
    snn.cat = lambda *a: a[0].like(torch.cat([t.F for t in a], 1))
    snn.SparseTensor = _Tensor
    import torch_points3d.modules.SparseConv3d.modules as modules
    return modules


def coords(g, n=110, lo=-4, hi=4):
    c = torch.cat([torch.randint(lo, hi, (n, 3), generator=g), torch.randint(0, 2, (n, 1), generator=g)], 1)
    c = torch.unique(c, dim=0)
    return c[torch.randperm(len(c), generator=g)].int().contiguous()


def init(module, g):
    for p in module.parameters():
        with torch.no_grad():
            p.copy_(torch.randn(p.shape, generator=g) * (0.25 if p.dim() > 1 else 0.3))
    for name, p in module.named_parameters():
        if name.endswith("bn.weight"):
            with torch.no_grad():
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
    return module


def record(rec, tag, make, run, C, cin, g):
    """run(module, tensor) -> output tensor; fp32 pass, then the same pass of a float64 copy"""
    module = init(make(), g).train()
    x = torch.randn(len(C), cin, generator=g)
    state = {k: v.clone() for k, v in module.state_dict().items()}
    del _relu_inputs[:]
    xin = x.clone().requires_grad_(True)
    out = run(module, _Tensor(xin, C))
    if _relu_inputs and min(_relu_inputs) < KINK_MARGIN:
        raise Unsafe("%s: ReLU input %.3g from 0" % (tag, min(_relu_inputs)))
    cot = torch.randn(out.F.shape, generator=g)
    (out.F * cot).sum().backward()
    m64 = make().double().train()
    m64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    x64 = x.double().requires_grad_(True)
    out64 = run(m64, _Tensor(x64, C))
    (out64.F * cot.double()).sum().backward()
    rec[tag + "coords"], rec[tag + "x"], rec[tag + "cot"] = C, x, cot
    rec[tag + "out"], rec[tag + "out_coords"], rec[tag + "grad_x"] = out.F.detach(), out.C, xin.grad
    rec[tag + "f64/out"], rec[tag + "f64/grad_x"] = out64.F.detach().numpy(), x64.grad.numpy()
    for k, v in state.items():
        rec[tag + "state/" + k] = v
    for k, v in module.state_dict().items():
        if "running_" in k:
            rec[tag + "after/" + k] = v.clone()
    for (k, p), (_, p64) in zip(module.named_parameters(), m64.named_parameters()):
        rec[tag + "pgrad/" + k] = p.grad
        rec[tag + "f64/pgrad/" + k] = p64.grad.numpy()


class Chain(torch.nn.Module):
    """down (stride 2) - down (stride 2) - up (stride 2) - up (stride 2, skip = the first down stage)"""

    def __init__(self, modules):
        super().__init__()
        self.d1 = modules.ResNetDown(down_conv_nn=[4, 8], kernel_size=3, stride=2, N=1)
        self.d2 = modules.ResNetDown(down_conv_nn=[8, 8], kernel_size=3, stride=2, N=1)
        self.u1 = modules.ResNetUp(up_conv_nn=[8, 8], kernel_size=3, stride=2, N=1)
        self.u2 = modules.ResNetUp(up_conv_nn=[16, 4], kernel_size=3, stride=2, N=1)

    def forward(self, x):
        a = self.d1(x)
        b = self.d2(a)
        return self.u2(self.u1(b, None), a)


def cases(modules, snn, seed):
    g = torch.Generator().manual_seed(seed)
    C = coords(g)
    rec = {}
    record(rec, "resblock/", lambda: modules.ResBlock(4, 8, snn.Conv3d), lambda m, t: m(t), C, 4, g)
    record(rec, "resblock_t/", lambda: modules.ResBlock(8, 8, snn.Conv3dTranspose), lambda m, t: m(t), C, 8, g)
    record(rec, "bottleneck/", lambda: modules.BottleneckBlock(8, 16, snn.Conv3d), lambda m, t: m(t), C, 8, g)
    record(rec, "down/", lambda: modules.ResNetDown(down_conv_nn=[4, 8], kernel_size=3, stride=2, N=1), lambda m, t: m(t), C, 4,
           g)

    class UpWithSkip(torch.nn.Module):  # the coarse input comes from a parameter-free stride-2 sum (kernel of ones)
        def __init__(self):
            super().__init__()
            self.up = modules.ResNetUp(up_conv_nn=[4 + 4, 8], kernel_size=2, stride=2, N=1)

        def forward(self, t):
            pool = snn.Conv3d(4, 4, kernel_size=2, stride=2).to(t.F.dtype)
            with torch.no_grad():
                pool.kernel.copy_(torch.eye(4, dtype=t.F.dtype).repeat(8, 1, 1) * 0.5)
            pool.kernel.requires_grad_(False)
            coarse = pool(t)
            return self.up(coarse, coarse.like(torch.tanh(coarse.F)))  # (the skip lives on the stage's INPUT set)

    record(rec, "up/", UpWithSkip, lambda m, t: m(t), C, 4, g)
    record(rec, "chain/", lambda: Chain(modules), lambda m, t: m(t), C, 4, g)
    return rec


def resolved_yaml(path):
    import yaml
    doc = yaml.safe_load(open(path))
    names = {k: v for k, v in doc.get("define_constants", {}).items()}

    def res(v):
        if isinstance(v, list):
            return [res(u) for u in v]
        if isinstance(v, dict):
            return {k: res(u) for k, u in v.items()}
        if isinstance(v, str):
            if v in names and isinstance(names[v], str):
                return names[v]
            try:
                return eval(v, {"__builtins__": {}}, {k: u for k, u in names.items() if not isinstance(u, str)})
            except Exception:
                return v  # FEAT, module names
        return v

    return {k: res(v) for k, v in doc.items() if k != "define_constants"}


def main():
    modules = load_reference()
    import torch_points3d.modules.SparseConv3d.nn as snn
    seed = 0
    while True:
        try:
            rec = cases(modules, snn, seed)
            break
        except Unsafe as e:
            print("seed %d: %s" % (seed, e))
            seed += 1
    rec["seed"] = np.array([seed])
    np.savez_compressed(os.path.join(HERE, "sparseconv.npz"), **mg.to_np(rec))
    conf = os.path.join(mg.REF, "torch_points3d", "applications", "conf", "sparseconv3d")
    cfg = {n: resolved_yaml(os.path.join(conf, n + ".yaml")) for n in ("unet_2", "unet_4", "encoder_2", "encoder_4")}
    with open(os.path.join(HERE, "sparseconv_config.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote sparseconv.npz (seed %d, %d arrays) and sparseconv_config.json" % (seed, len(rec)))


if __name__ == "__main__":
    main()
