"""Point-voxel timings: the fused devoxelise / voxelise (forward, forward + backward) against the torch composition of
tests/pvcnn_ref.py over the SAME tables -- an (N, 8, C) gather and index_add_ -- on a synthetic surface of --points
(100 000) points, C = 32 / 96 at tensor strides 1 and 16; the table builds (coordinates, lookups, weights, inversion) on
their own; `PVCNN(cr = 1)` forward and training step on that cloud.  HIP events around every call, median of --runs (30)
calls after a warm-up.  Needs a GPU (no fallback).

    python tools/bench_pvcnn.py [--points 100000] [--runs 30] [--out profiles/pvcnn_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparseconv import timed  # noqa: E402


def surface_points(n):
    """two wavy sheets (one cloud each) of n points together, about two points per unit voxel, both sides of 0"""
    g = torch.Generator().manual_seed(0)
    half = n // 2
    side = (half / 2.0) ** 0.5
    rows = []
    for b in range(2):
        uv = (torch.rand(half, 2, generator=g) - 0.5) * side
        z = 12.0 * torch.sin(uv[:, 0] / 17.0 + b) * torch.cos(uv[:, 1] / 23.0) + 0.07 * uv[:, 0] + torch.rand(half, generator=g)
        rows.append(torch.cat([uv, z.unsqueeze(1), torch.full((half, 1), float(b))], 1))
    return torch.cat(rows)[torch.randperm(2 * half, generator=g)].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pvcnn needs a GPU: nothing is measured without one")
    import pvcnn_ref as pref
    from torch_points3d_amd import pvcnn as pv
    from torch_points3d_amd import sparseconv as sc
    dev = torch.device("cuda:0")
    pc = surface_points(args.points).to(dev)
    result = {"workload": "pvcnn", "points": int(pc.shape[0]), "runs": args.runs, "timer": "hip events, median", "levels": []}
    for s in (1, 16):
        Cs = pref.voxel_set(pref.quantize(pc, s))

        def tables():
            z = pv.PointTensor(torch.zeros(pc.shape[0], 1, device=dev), pc)
            x = sc.SparseTensor(torch.zeros(Cs.shape[0], 1, device=dev), Cs, s)
            pv.point_to_voxel(x, z)
            pv.voxel_to_point(x, z)
            return z, x

        build_ms = timed(lambda: tables(), args.runs)  # voxel set, both lookups, weights, both inversions, two 1-wide passes
        z0, x0 = tables()
        idx = z0.additional_features["idx_query"][s]
        idx8, w = z0.idx_query[s], z0.weights[s]
        cnt = z0.additional_features["counts"][s]
        for width in (32, 96):
            g = torch.Generator().manual_seed(width)
            Fp = torch.randn(pc.shape[0], width, generator=g).to(dev).requires_grad_(True)
            Fv = torch.randn(Cs.shape[0], width, generator=g).to(dev).requires_grad_(True)
            cot_p, cot_v = torch.randn_like(Fp), torch.randn_like(Fv)
            ops = {
                "devoxelize": (lambda: pv._Devoxelize.apply(Fv, idx8, w, *z0.inverted[("devoxelize", s)]),
                               lambda: pref.devoxelize(Fv, idx8, w), Fv, cot_p),
                "voxelize": (lambda: pv._Voxelize.apply(Fp, idx.view(-1, 1), *z0.inverted[("voxelize", s)]),
                             lambda: pref.voxelize(Fp, idx, Cs.shape[0]), Fp, cot_v),
            }
            for name, (hip, comp, leaf, cot) in ops.items():
                def fwd(fn):
                    with torch.no_grad():
                        return fn()

                def train(fn):
                    leaf.grad = None
                    (fn() * cot).sum().backward()

                ms = {"hip_fwd": timed(lambda: fwd(hip), args.runs), "torch_fwd": timed(lambda: fwd(comp), args.runs),
                      "hip_fwd_bwd": timed(lambda: train(hip), args.runs), "torch_fwd_bwd": timed(lambda: train(comp), args.runs)}
                result["levels"].append({"op": name, "stride": s, "C": width, "voxels": int(Cs.shape[0]),
                                         "longest_run": int(cnt.max()), "ms": ms,
                                         "max_abs_diff_out": float((fwd(hip) - fwd(comp)).abs().max()),
                                         "ratio_fwd": round(ms["torch_fwd"] / ms["hip_fwd"], 2),
                                         "ratio_fwd_bwd": round(ms["torch_fwd_bwd"] / ms["hip_fwd_bwd"], 2)})
        result.setdefault("table_build_ms", {})[str(s)] = build_ms
    torch.manual_seed(0)
    net = pv.pvcnn(1.0, 1.0, 3, 13).to(dev)
    feats = torch.randn(pc.shape[0], 3, device=dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)

    def net_fwd():
        with torch.no_grad():
            return net(pv.PointTensor(feats, pc))

    def net_step():
        opt.zero_grad(set_to_none=True)
        net(pv.PointTensor(feats, pc)).square().mean().backward()
        opt.step()

    net.eval()
    fwd_ms = timed(net_fwd, args.runs)
    net.train()
    result["pvcnn_cr1"] = {"num_features": 3, "num_classes": 13, "vres": 1.0, "forward_ms": fwd_ms,
                           "train_step_ms": timed(net_step, args.runs),
                           "note": "every call builds its voxel set, coordinate sets, kernel maps and point-voxel tables anew"}
    result["not_timed"] = ["nearest = True", "C not a multiple of 4 (the one-float-per-lane route)", "tensor strides 2, 4, 8 on their own",
                           "the point_transforms (library GEMM) on their own", "more than two clouds per batch"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
