"""PointNet timings: every fused per-cloud operator (csrc/segment_rows.hip) against its torch composition on the same
device, forward and forward + backward, at B = 8 clouds of unequal sizes and N = 65536 rows --
  * the spatial transformer's application at k = 3 (C = 6) and k = 64: `segment_transform` vs `bmm` over `trans[batch]`;
  * the global feature's way back at (C1, C2) = (64, 1024): `segment_broadcast_cat` vs `cat([x, g[batch]], 1)`;
  * the mean pool at C = 1024: `segment_mean_rows` vs `index_add` / counts --
then `PointNetSeg` at the widths of conf/models/segmentation/pointnet.yaml (FEAT = 3, 13 classes), forward (eval) and a
training step (forward, cross entropy + internal loss, backward, SGD), fused=True against fused=False, and the peak
memory of both sides of every pair.  Each call is bracketed by HIP events after a warm-up; the median of --iters (30)
calls is reported with the spread.  The two sides' outputs are compared first.  Needs a GPU (no fallback).

    python tools/bench_pointnet.py [--n 65536] [--iters 30] [--out profiles/pointnet_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=5):
    """(median ms, min ms, max ms, peak MiB above the standing allocation) of fn over `iters` event-bracketed calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "peak_mib": round(peak, 2)}


def pair(name, shape, fused, plain, leaves, cot, iters):
    """forward and forward + backward of both sides; `fused` / `plain` map the leaves to the output"""
    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(*leaves)
        return run

    def train(fn):
        def run():
            for t in leaves:
                if t is not None:
                    t.grad = None
            (fn(*leaves) * cot).sum().backward()
        return run

    diff = float((fwd(fused)() - fwd(plain)()).abs().max())
    row = {"operator": name, "shape": shape, "max_abs_diff_out": diff,
           "hip_fwd": timed(fwd(fused), iters), "torch_fwd": timed(fwd(plain), iters),
           "hip_fwd_bwd": timed(train(fused), iters), "torch_fwd_bwd": timed(train(plain), iters)}
    row["speedup_fwd"] = round(row["torch_fwd"]["ms"] / row["hip_fwd"]["ms"], 2)
    row["speedup_fwd_bwd"] = round(row["torch_fwd_bwd"]["ms"] / row["hip_fwd_bwd"]["ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet needs a GPU: nothing is measured without one")
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.pointnet import PointNetSeg
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    N, B = args.n, 8
    weights = torch.tensor([1.0, 3.0, 0.5, 2.0, 1.5, 0.7, 2.3, 1.0])
    sizes = (weights / weights.sum() * N).long()
    sizes[-1] += N - int(sizes.sum())
    batch = torch.repeat_interleave(torch.arange(B), sizes).to(dev)
    seg, _, _ = tp._segments(batch)
    counts = sizes.to(dev).clamp(min=1).float()
    result = {"workload": "pointnet", "rows": N, "clouds": B, "cloud_sizes": sizes.tolist(), "iters": args.iters,
              "timer": "HIP events around one call, median", "operators": []}

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev).requires_grad_(True)

    for k, C in ((3, 6), (64, 64)):
        x, T, cot = leaf(N, C), leaf(B, k, k, scale=k ** -0.5), torch.randn(N, C, generator=gen).to(dev)
        result["operators"].append(pair(
            "segment_transform", {"k": k, "C": C}, lambda x, T: tp.segment_transform(x, T, seg=seg),
            lambda x, T, k=k: torch.cat([torch.bmm(x[:, None, :k], T[batch])[:, 0], x[:, k:]], 1), (x, T), cot, args.iters))
    x, g, cot = leaf(N, 64), leaf(B, 1024), torch.randn(N, 1088, generator=gen).to(dev)
    result["operators"].append(pair("segment_broadcast_cat", {"C1": 64, "C2": 1024},
                                    lambda x, g: tp.segment_broadcast_cat(x, g, seg=seg),
                                    lambda x, g: torch.cat([x, g[batch]], 1), (x, g), cot, args.iters))
    rows, cot = leaf(N, 1024), torch.randn(B, 1024, generator=gen).to(dev)
    result["operators"].append(pair(
        "segment_mean_rows", {"C": 1024}, lambda r: tp.segment_mean_rows(r, seg),
        lambda r: torch.zeros(B, 1024, device=dev).index_add(0, batch, r) / counts[:, None], (rows,), cot, args.iters))
    del x, g, rows, cot

    classes = 13
    feats = torch.randn(N, 6, generator=gen).to(dev)
    labels = torch.randint(0, classes, (N,), generator=gen).to(dev)
    torch.manual_seed(0)
    nets = {True: PointNetSeg(input_nc=6, seg_nn=[1088, 512, 256, 128, classes], fused=True).to(dev)}
    nets[False] = PointNetSeg(input_nc=6, seg_nn=[1088, 512, 256, 128, classes], fused=False).to(dev)
    nets[False].load_state_dict(nets[True].state_dict())
    result["net"] = {"model": "PointNetSeg at the YAML widths", "input_nc": 6, "classes": classes}
    for fused, net in nets.items():
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)

        def fwd(net=net):
            net.eval()
            with torch.no_grad():
                return net(feats, batch)

        def step(net=net, opt=opt):
            net.train()
            opt.zero_grad(set_to_none=True)
            out = net(feats, batch)
            loss = torch.nn.functional.cross_entropy(out, labels) + 0.001 * net.feat_stn.get_orthogonal_regularization_loss()
            loss.backward()
            opt.step()

        side = "hip" if fused else "torch"
        result["net"][side + "_forward"] = timed(fwd, args.iters, warmup=3)
        result["net"][side + "_train_step"] = timed(step, args.iters, warmup=3)
    for what in ("forward", "train_step"):
        result["net"]["speedup_" + what] = round(result["net"]["torch_" + what]["ms"] / result["net"]["hip_" + what]["ms"], 2)
    result["not_timed"] = ["the dense (B, n, C) layout", "SegPointNetModel (PointNet_Features)", "k between 4 and 64 other than 64",
                           "more than one GPU"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
