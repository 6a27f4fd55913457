"""MS-SVConv timings: the 5x5x5 first layer on the wide kernels, on the generic kernels and as the torch composition over the
SAME kernel-map table (per offset index_select -> matmul -> index_add_), forward and weight gradient, at (Cin, Cout) =
(1, 32) and (4, 32) on the two-sheet surface of tools/bench_pvcnn.py voxelised to about 40 000 - 60 000 voxels (with the
mean number of present offsets per row); `scale_fuse` forward and forward + backward at S = 3, C = 32, N = 100 000 against the
torch composition; MS_SparseConv3d_Shared with the MS_SVCONV_B2cm_X2_3head numbers on 2 x 20 000 points, forward and one
training step.  HIP events around every call, median of --runs (30) calls after a warm-up, with the spread (max - min) of
the samples: "auto" should route to the wide kernels exactly where they beat the generic route by more than that spread.
Needs a GPU (no fallback).

    python tools/bench_ms_svconv.py [--points 100000] [--runs 30] [--out profiles/ms_svconv_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pvcnn import surface_points  # noqa: E402
from bench_sparseconv import composed  # noqa: E402


def timed(fn, runs, warmup=3):
    """(median ms, max - min ms) of `runs` calls between HIP events"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 4), round(max(out) - min(out), 4)


class _Data(object):
    def __init__(self, pos, batch, x):
        self.pos, self.batch, self.x = pos, batch, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_svconv_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ms_svconv needs a GPU: nothing is measured without one")
    from torch_points3d_amd import _lib, ms_svconv as ms, sparseconv as sc, torchpoints as tp
    dev = torch.device("cuda:0")
    result = {"workload": "ms_svconv", "runs": args.runs, "timer": "hip events, median (spread = max - min)"}

    # ---- the first layer
    pc = surface_points(args.points).to(dev)
    v = ms.voxelize(pc[:, :3].contiguous(), pc[:, 3].long(), 1.0, torch.ones(len(pc), 1, device=dev))
    C = torch.cat([v.coords.int(), v.batch.int().unsqueeze(1)], 1).contiguous()
    n = len(C)
    table = sc.SparseTensor(torch.zeros(n, 1, device=dev), C)._kmap(5, 1, 1).forward
    result["voxels"] = n
    result["present_offsets_per_row"] = round(float((table >= 0).sum(1).float().mean()), 2)
    h = _lib.load()
    result["first_layer"] = []
    for cin, cout in ((1, 32), (4, 32)):
        g = torch.Generator().manual_seed(cin)
        x = torch.randn(n, cin, generator=g).to(dev)
        W = (torch.randn(125, cin, cout, generator=g) * 0.1).to(dev)
        dy = torch.randn(n, cout, generator=g).to(dev)
        y = torch.empty(n, cout, device=dev)
        dW = torch.empty_like(W)
        s = _lib.stream_ptr(dev)
        ws = {}
        for name, q in (("wide", h.tp3d_sparse_wgrad_wide_workspace_floats), ("generic", h.tp3d_sparse_wgrad_workspace_floats)):
            f = q(n, 125, cin, cout)
            ws[name] = (torch.empty(max(f, 1), device=dev), f)
        calls = {
            "forward_wide": lambda: _lib.call("tp3d_sparse_conv_wide_f32", _lib.ptr(x), _lib.ptr(table), _lib.ptr(W), n, n, 125, cin,
                                              cout, _lib.ptr(y), s),
            "forward_generic": lambda: _lib.call("tp3d_sparse_conv_f32", _lib.ptr(x), _lib.ptr(table), _lib.ptr(W), n, n, 125, cin,
                                                 cout, 0, _lib.ptr(y), s),
            "forward_torch": lambda: composed(x, W, table, n),
            "wgrad_wide": lambda: _lib.call("tp3d_sparse_wgrad_wide_f32", _lib.ptr(x), _lib.ptr(dy), _lib.ptr(table), n, n, 125, cin,
                                            cout, _lib.ptr(dW), _lib.ptr(ws["wide"][0]), ws["wide"][1], s),
            "wgrad_generic": lambda: _lib.call("tp3d_sparse_wgrad_f32", _lib.ptr(x), _lib.ptr(dy), _lib.ptr(table), n, n, 125, cin,
                                               cout, _lib.ptr(dW), _lib.ptr(ws["generic"][0]), ws["generic"][1], s),
            "wgrad_torch": lambda: torch.stack([
                torch.zeros(cin, cout, device=dev) if not bool((table[:, k] >= 0).any()) else
                x.index_select(0, table[table[:, k] >= 0, k].long()).t() @ dy[table[:, k] >= 0] for k in range(125)]),
        }
        row = {"cin": cin, "cout": cout}
        for name, fn in calls.items():
            row[name + "_ms"], row[name + "_spread_ms"] = timed(fn, args.runs)
        result["first_layer"].append(row)
        print(json.dumps(row), flush=True)

    # ---- the multi-scale head
    S, Cc, N = 3, 32, 100000
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(N, Cc, generator=g).to(dev).requires_grad_(True) for _ in range(S)]
    cot = torch.randn(N, S * Cc, generator=g).to(dev)

    def torch_fuse():
        return torch.cat([x / (torch.norm(x, p=2, dim=1, keepdim=True) + 1e-20) for x in xs], 1)

    def step(fuse):
        for x in xs:
            x.grad = None
        (fuse() * cot).sum().backward()

    fuse = {"S": S, "C": Cc, "N": N}
    with torch.no_grad():
        fuse["forward_hip_ms"], fuse["forward_hip_spread_ms"] = timed(lambda: tp.scale_fuse(xs, "cat"), args.runs)
        fuse["forward_torch_ms"], fuse["forward_torch_spread_ms"] = timed(torch_fuse, args.runs)
    fuse["fwd_bwd_hip_ms"], fuse["fwd_bwd_hip_spread_ms"] = timed(lambda: step(lambda: tp.scale_fuse(xs, "cat")), args.runs)
    fuse["fwd_bwd_torch_ms"], fuse["fwd_bwd_torch_spread_ms"] = timed(lambda: step(torch_fuse), args.runs)
    result["scale_fuse"] = fuse
    print(json.dumps(fuse), flush=True)

    # ---- the model
    def cloud(npts, seed):
        gg = torch.Generator().manual_seed(seed)
        uv = torch.rand(npts, 2, generator=gg) * 3.0
        p = torch.stack([uv[:, 0], uv[:, 1], 0.3 * torch.sin(3 * uv[:, 0]) * torch.cos(2 * uv[:, 1])], 1)
        return _Data((p + 0.004 * torch.randn(npts, 3, generator=gg)).to(dev), torch.zeros(npts, dtype=torch.long, device=dev),
                     torch.ones(npts, 1, device=dev))

    d0, d1 = cloud(20000, 1), cloud(20000, 2)
    gg = torch.Generator().manual_seed(3)
    match = torch.stack([torch.randperm(20000, generator=gg)[:5000], torch.randperm(20000, generator=gg)[:5000]], 1).to(dev)
    torch.manual_seed(0)
    net = ms.build("MS_SVCONV_B2cm_X2_3head").to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)

    def train_step():
        opt.zero_grad(set_to_none=True)
        net(d0, d1, match)
        net.loss.backward()
        opt.step()

    model = {"config": "MS_SVCONV_B2cm_X2_3head", "points": [20000, 20000], "routes": {}}
    for route in ("wide", "generic"):
        sc.WIDE_ROUTE = route
        r = {}
        with torch.no_grad():
            r["forward_ms"], r["forward_spread_ms"] = timed(lambda: net(d0), max(5, args.runs // 3))
        r["train_step_ms"], r["train_step_spread_ms"] = timed(train_step, max(5, args.runs // 3))
        model["routes"][route] = r
    sc.WIDE_ROUTE = "auto"
    result["model"] = model
    print(json.dumps(model), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
