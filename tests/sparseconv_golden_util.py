"""The cases of tests/golden/sparseconv.npz (make_golden_sparseconv.py) rebuilt from either the restatement
(tests/sparseconv_ref.py) or the project's modules (torch_points3d_amd.sparseconv), with the recorded weights."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparseconv.npz")
CASES = ["resblock", "resblock_t", "bottleneck", "down", "up", "chain"]
_cache = {}


def load():
    if "z" not in _cache:
        z = np.load(GOLDEN)
        _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def case(tag):
    """{key without the tag: tensor (float64 arrays stay numpy)}"""
    out = {}
    for k, v in load().items():
        if k.startswith(tag + "/"):
            out[k[len(tag) + 1:]] = v if v.dtype == np.float64 else torch.from_numpy(v)
    return out


def _like(t, feats):
    return t.like(feats) if hasattr(t, "like") else t._like(feats)


class _Up(torch.nn.Module):
    def __init__(self, L):
        super().__init__()
        self.up = L.ResNetUp([4 + 4, 8], kernel_size=2, stride=2, N=1) if L.__name__ == "sparseconv_ref" else \
            L.ResNetUp(up_conv_nn=[4 + 4, 8], kernel_size=2, stride=2, N=1)
        self._L = L

    def forward(self, t):
        pool = self._L.Conv3d(4, 4, kernel_size=2, stride=2).to(t.F.device).to(t.F.dtype)
        with torch.no_grad():
            pool.kernel.copy_(torch.eye(4, dtype=t.F.dtype).repeat(8, 1, 1) * 0.5)
        pool.kernel.requires_grad_(False)
        coarse = pool(t)
        return self.up(coarse, _like(coarse, torch.tanh(coarse.F)))


class _Chain(torch.nn.Module):
    def __init__(self, L):
        super().__init__()
        down = (lambda nn_: L.ResNetDown(nn_, kernel_size=3, stride=2, N=1)) if L.__name__ == "sparseconv_ref" else \
            (lambda nn_: L.ResNetDown(down_conv_nn=nn_, kernel_size=3, stride=2, N=1))
        up = (lambda nn_: L.ResNetUp(nn_, kernel_size=3, stride=2, N=1)) if L.__name__ == "sparseconv_ref" else \
            (lambda nn_: L.ResNetUp(up_conv_nn=nn_, kernel_size=3, stride=2, N=1))
        self.d1, self.d2, self.u1, self.u2 = down([4, 8]), down([8, 8]), up([8, 8]), up([16, 4])

    def forward(self, x):
        a = self.d1(x)
        b = self.d2(a)
        return self.u2(self.u1(b, None), a)


def build(tag, L):
    ref = L.__name__ == "sparseconv_ref"
    if tag == "resblock":
        return L.ResBlock(4, 8, L.Conv3d)
    if tag == "resblock_t":
        return L.ResBlock(8, 8, L.Conv3dTranspose)
    if tag == "bottleneck":
        return L.BottleneckBlock(8, 16, L.Conv3d)
    if tag == "down":
        return L.ResNetDown([4, 8], kernel_size=3, stride=2, N=1) if ref else \
            L.ResNetDown(down_conv_nn=[4, 8], kernel_size=3, stride=2, N=1)
    return _Up(L) if tag == "up" else _Chain(L)


def run(tag, L, make_tensor, device="cpu", dtype=torch.float32):
    """-> (module after one train-mode step, input leaf, output tensor object, fixture dict); gradients are populated"""
    g = case(tag)
    m = build(tag, L).to(device).to(dtype).train()
    state = {k[len("state/"):]: (v.to(dtype) if v.is_floating_point() else v) for k, v in g.items() if k.startswith("state/")}
    m.load_state_dict(state, strict=True)
    x = g["x"].to(device).to(dtype).requires_grad_(True)
    out = m(make_tensor(x, g["coords"].to(device)))
    (out.F * g["cot"].to(device).to(dtype)).sum().backward()
    return m, x, out, g
