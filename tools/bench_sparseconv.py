"""Sparse voxel convolution timings: the fused gather-GEMM (forward, forward + backward) against the composition that
uses the SAME kernel-map tables -- per offset index_select -> matmul -> index_add_ -- on a synthetic surface of about
10^5 voxels, kernel_size 3 stride 1 at C = 32 / 64 / 128 and the stride-2 level below it; the full `unet_4` forward and
training step; the coordinate-set and kernel-map build on its own.  HIP events around every call, median of --runs
(30) calls after a warm-up.  A dense conv3d is not a baseline.  Needs a GPU (no fallback).

    python tools/bench_sparseconv.py [--voxels 100000] [--runs 30] [--out profiles/sparseconv_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(voxels):
    """integer voxels of two wavy sheets (one cloud each), about `voxels` rows together"""
    side = int((voxels / 2) ** 0.5)
    u = torch.arange(side)
    gx, gy = torch.meshgrid(u, u, indexing="ij")
    rows = []
    for b in range(2):
        z = (12.0 * torch.sin(gx / 17.0 + b) * torch.cos(gy / 23.0) + 0.07 * gx).round().long()
        rows.append(torch.stack([gx.reshape(-1) - side // 2, gy.reshape(-1) - side // 2, z.reshape(-1),
                                 torch.full((side * side,), b)], 1))
    return torch.unique(torch.cat(rows), dim=0).int()


def timed(fn, runs, warmup=3):
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
    return round(statistics.median(out), 4)


def composed(x, W, table, n_out):
    """the same product from torch ops over the same table"""
    y = torch.zeros((n_out, W.shape[2]), dtype=x.dtype, device=x.device)
    for k in range(W.shape[0]):
        rows = torch.nonzero(table[:, k] >= 0).squeeze(1)
        if rows.numel():
            y.index_add_(0, rows, x.index_select(0, table[rows, k].long()) @ W[k])
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparseconv needs a GPU: nothing is measured without one")
    from torch_points3d_amd import sparseconv as sc
    dev = torch.device("cuda:0")
    C = surface(args.voxels).to(dev)
    result = {"workload": "sparseconv", "voxels": int(C.shape[0]), "runs": args.runs, "timer": "hip events, median", "levels": []}

    def build():
        st = sc.SparseTensor(torch.zeros(C.shape[0], 1, device=dev), C)
        st._kmap(3, 1, 1)
        st._kmap(3, 1, 2)
        return st

    result["kernel_map_build_ms"] = timed(build, args.runs)  # input set, stride-2 set, the k3s1 and k3s2 maps
    st0 = build()
    result["coarse_voxels"] = st0.cmaps[2].n
    result["slots_filled_k3s1"] = round(float((st0.kmaps[(3, 1, 1)].forward >= 0).float().mean()), 3)
    for stride in (1, 2):
        km = st0.kmaps[(3, 1, stride)]
        for width in (32, 64, 128):
            gen = torch.Generator().manual_seed(width)
            x = torch.randn(km.n_in, width, generator=gen).to(dev).requires_grad_(True)
            W = (torch.randn(27, width, width, generator=gen) * 0.05).to(dev).requires_grad_(True)
            cot = torch.randn(km.n_out, width, generator=gen).to(dev)

            def hip_fwd():
                with torch.no_grad():
                    return sc._GatherConv.apply(x, W, km.forward, km.inverse)

            def torch_fwd():
                with torch.no_grad():
                    return composed(x, W, km.forward, km.n_out)

            def hip_train():
                x.grad = W.grad = None
                (sc._GatherConv.apply(x, W, km.forward, km.inverse) * cot).sum().backward()

            def torch_train():
                x.grad = W.grad = None
                (composed(x, W, km.forward, km.n_out) * cot).sum().backward()

            diff = float((hip_fwd() - torch_fwd()).abs().max())
            ms = {"hip_fwd": timed(hip_fwd, args.runs), "torch_fwd": timed(torch_fwd, args.runs),
                  "hip_fwd_bwd": timed(hip_train, args.runs), "torch_fwd_bwd": timed(torch_train, args.runs)}
            result["levels"].append({"stride": stride, "C": width, "rows_in": km.n_in, "rows_out": km.n_out, "ms": ms,
                                     "max_abs_diff_out": diff, "ratio_fwd": round(ms["torch_fwd"] / ms["hip_fwd"], 2),
                                     "ratio_fwd_bwd": round(ms["torch_fwd_bwd"] / ms["hip_fwd_bwd"], 2)})
    torch.manual_seed(0)
    net = sc.SparseConv3dUnet("unet_4", input_nc=3).to(dev)
    feats = torch.randn(C.shape[0], 3, device=dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)

    def net_fwd():
        with torch.no_grad():
            return net(sc.SparseTensor(feats, C))

    def net_step():
        opt.zero_grad(set_to_none=True)
        net(sc.SparseTensor(feats, C)).square().mean().backward()
        opt.step()

    net.eval()
    fwd_ms = timed(net_fwd, args.runs)
    net.train()
    result["unet_4"] = {"input_nc": 3, "forward_ms": fwd_ms, "train_step_ms": timed(net_step, args.runs),
                        "note": "every call builds its coordinate sets and kernel maps anew"}
    result["not_timed"] = ["kernel_size 2 levels", "the transposed convolutions on their own", "BottleneckBlock networks",
                           "encoder_4", "C = 256 (the deepest level) on its own", "more than two clouds per batch"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
