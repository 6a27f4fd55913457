"""PosPool / PPNet timings: the position-pooling operator (forward, forward + backward) at the first-stage shape of
conf/models/segmentation/ppnet.yaml -- 65536 points, 26 neighbours, C = 72 (in_feat: the input block and the bottleneck
of the first ResnetBBlock) and C = 36 (the same stage at in_feat = 36), sin_cos / avg -- against the plain-torch
composition tests/ppnet_ref.py in fp32 on the same device, and the full `PPNet` forward at 65536 points.  The two sides are timed alternately, each window ends in a device synchronise, the
median over the rounds is reported, and their outputs are compared first.  A window runs at least --iters calls and at
least --window-s seconds (the call count is fixed per function after the warm-up), so that a sub-millisecond operator
is not timed over a few milliseconds.  Needs a GPU (no fallback).

    python tools/bench_ppnet.py [--n 65536] [--iters 20] [--window-s 0.3] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_kpconv import synthetic_cloud  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(fns, iters, rounds, window_s, warmup=3):
    """(median ms per call, max - min over the rounds, calls per window) of every function, the windows interleaved"""
    calls = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        calls[k] = max(iters, int(window_s * 1e3 / max(window(fn, 3), 1e-3)) + 1)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, calls[k]))
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: round(max(v) - min(v), 4) for k, v in times.items()}, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--neighbors", type=int, default=26)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window-s", type=float, default=0.3, help="least length of a timed window in seconds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grid", type=float, default=0.04)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppnet needs a GPU: nothing is measured without one")
    from ppnet_ref import pospool_ref
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.ppnet import PPNet, pospool
    dev = torch.device("cuda:0")
    pos, batch = synthetic_cloud(args.n, 1, args.grid)
    pos, batch = pos.to(dev), batch.to(dev)
    radius = 2.5 * args.grid
    nbr = tp.ball_query(radius, args.neighbors, pos, pos, mode="partial_dense", batch_x=batch, batch_y=batch)[0]
    result = {"workload": "ppnet", "points": pos.shape[0], "neighbors": args.neighbors, "radius": radius,
              "slots_filled": round(float((nbr >= 0).float().mean()), 3), "rounds": args.rounds, "window_s": args.window_s,
              "operator": []}
    for C in (36, 72):
        gen = torch.Generator().manual_seed(C)
        x = torch.randn(pos.shape[0], C, generator=gen).to(dev).requires_grad_(True)
        cot = torch.randn(pos.shape[0], C, generator=gen).to(dev)

        def hip_fwd():
            with torch.no_grad():
                return pospool(pos, pos, nbr, x, radius, "sin_cos", "avg")

        def ref_fwd():
            with torch.no_grad():
                return pospool_ref(pos, pos, nbr, x, radius, "sin_cos", "avg")

        def hip_train():
            x.grad = None
            (pospool(pos, pos, nbr, x, radius, "sin_cos", "avg") * cot).sum().backward()
            return x.grad

        def ref_train():
            x.grad = None
            (pospool_ref(pos, pos, nbr, x, radius, "sin_cos", "avg") * cot).sum().backward()
            return x.grad

        diff_out = float((hip_fwd() - ref_fwd()).abs().max())
        diff_grad = float((hip_train() - ref_train()).abs().max())
        ms, spread, calls = alternate({"hip_fwd": hip_fwd, "torch_fwd": ref_fwd, "hip_fwd_bwd": hip_train,
                                       "torch_fwd_bwd": ref_train}, args.iters, args.rounds, args.window_s)
        result["operator"].append({"C": C, "embedding": "sin_cos", "reduction": "avg", "ms": ms, "spread_ms": spread,
                                   "calls_per_window": calls, "max_abs_diff_out": diff_out, "max_abs_diff_grad": diff_grad,
                                   "speedup_fwd": round(ms["torch_fwd"] / ms["hip_fwd"], 2),
                                   "speedup_fwd_bwd": round(ms["torch_fwd_bwd"] / ms["hip_fwd_bwd"], 2)})
    torch.manual_seed(0)
    net = PPNet(4, 13, args.grid, in_feat=72).to(dev).eval()
    feats = torch.randn(pos.shape[0], 4).to(dev)

    def net_fwd():
        with torch.no_grad():
            return net(PDData(pos=pos, batch=batch, x=feats))

    ms, spread, calls = alternate({"forward": net_fwd}, max(args.iters // 4, 3), args.rounds, args.window_s)
    result["net"] = {"in_feat": 72, "classes": 13, "ms": ms["forward"], "spread_ms": spread["forward"],
                     "calls_per_window": calls["forward"], "points_per_s": round(pos.shape[0] / ms["forward"] * 1e3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
