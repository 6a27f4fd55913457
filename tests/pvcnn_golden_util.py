"""tests/golden/pvcnn.npz (make_golden_pvcnn.py: the reference's own PVCNN over dense stand-ins for torchsparse) as tensors,
and one train-mode step of a network -- the restatement tests/pvcnn_ref.py or torch_points3d_amd.pvcnn -- on it."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pvcnn.npz")
CONFIG = os.path.join(HERE, "golden", "pvcnn_config.json")
_cache = {}


def config():
    if "cfg" not in _cache:
        with open(CONFIG) as f:
            _cache["cfg"] = json.load(f)
    return _cache["cfg"]


def load():
    """{key: tensor}; float64 arrays stay numpy, int16 indices are widened"""
    if "z" not in _cache:
        z = np.load(GOLDEN)
        out = {}
        for k in z.files:
            v = z[k]
            if v.dtype == np.float64:
                out[k] = v
            else:
                out[k] = torch.from_numpy(v.astype(np.int64) if v.dtype == np.int16 else v)
        _cache["z"] = out
    return _cache["z"]


def state_dict(dtype=torch.float32):
    """the recorded initial state: parameters are multiples of 1 / state_scale stored as int8"""
    g, scale = load(), config()["state_scale"]
    sd = {k[len("state_q/"):]: v.to(dtype) / scale for k, v in g.items() if k.startswith("state_q/")}
    sd.update({k[len("state/"):]: v for k, v in g.items() if k.startswith("state/")})
    return sd


def sample(t):
    """what the fixture keeps of a parameter gradient"""
    cfg = config()
    return t if t.numel() <= cfg["pgrad_full"] else t.reshape(-1)[::cfg["pgrad_stride"]]


class Data(object):
    def __init__(self, x, pos, batch):
        self.x, self.pos, self.batch = x, pos, batch


def train_step(net, forward, device="cpu", dtype=torch.float32):
    """loads the recorded state, runs forward(net, x, pos, batch) in train mode and backpropagates the recorded cotangent
    -> (input leaf, output)"""
    g = load()
    net.to(device).to(dtype).train()
    net.load_state_dict(state_dict(dtype), strict=True)
    x = g["x"].to(device).to(dtype).requires_grad_(True)
    out = forward(net, x, g["pos"].to(device), g["batch"].to(device))
    (out * g["cot"].to(device).to(dtype)).sum().backward()
    return x, out
