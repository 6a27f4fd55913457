"""Region growing of PointGroup: the device call (torchpoints.region_grow_csr, csrc/region_grow.hip) against the path
`torch_points_kernels.region_grow` takes for the same device tensors (per label: partial-dense ball query with nsample
300, the (n, 300) int64 table copied to the host, the walk in libtp3d_cpu.so, every cluster copied back).

The scene is synthetic and voxelised: --clouds (4) clouds of filled boxes on a lattice of step h with about --points
(60 000) non-stuff points each over a floor of stuff points, radius = 1.5 h, PointGroup's nsample 300 and
min_cluster_size 10.  region_grow_csr: HIP events, median of --runs (30) calls; region_grow: wall clock around the call
and a synchronise, median of --host-runs (3).  A second device timing takes the same points with a random label per
voxel and min_cluster_size 1: many components of a few points, the worst case of the one-workgroup scan of the runs.
Needs a GPU (no fallback).

    python tools/bench_region_grow.py [--out profiles/region_grow_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparseconv import timed  # noqa: E402

H = 0.02
STUFF = 0


def scene(clouds, points, seed=0):
    """(pos (N,3) f32, labels (N), batch (N)): per cloud a 160 x 160 floor of stuff voxels and filled boxes of 4..24
    voxels per side with labels 1..8 until `points` non-stuff voxels are taken; one point per voxel, shuffled per cloud"""
    rng = np.random.RandomState(seed)
    pos, labels, batch = [], [], []
    for b in range(clouds):
        grid = np.zeros((160, 160, 64), dtype=np.int8)  # 0: empty, else label + 1
        grid[:, :, 0] = STUFF + 1
        while int((grid > STUFF + 1).sum()) < points:
            size = rng.randint(4, 25, size=3)
            lo = [rng.randint(0, grid.shape[a] - size[a]) for a in range(3)]
            lo[2] = max(lo[2], 1)
            grid[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = rng.randint(1, 9) + 1
        vox = np.argwhere(grid > 0)
        lab = grid[grid > 0].astype(np.int64) - 1
        perm = rng.permutation(len(vox))
        pos.append((vox[perm] * H + rng.uniform(-H / 64, H / 64, size=vox.shape)).astype(np.float32))
        labels.append(lab[perm])
        batch.append(np.full(len(vox), b, dtype=np.int64))
    return (torch.from_numpy(np.concatenate(pos)), torch.from_numpy(np.concatenate(labels)),
            torch.from_numpy(np.concatenate(batch)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_grow needs a GPU: nothing is measured without one")
    import torch_points_kernels as tpk
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    pos, labels, batch = [t.to(dev) for t in scene(args.clouds, args.points)]
    radius, nsample, min_size = 1.5 * H, 300, 10
    ignore = torch.tensor([-1, STUFF], device=dev)

    def device_call():
        return tp.region_grow_csr(pos, labels, batch, ignore_labels=ignore, radius=radius, nsample=nsample,
                                  min_cluster_size=min_size)

    def host_call():
        return tpk.region_grow(pos, labels, batch, ignore_labels=ignore, radius=radius, nsample=nsample,
                               min_cluster_size=min_size)

    cs = device_call()
    device_ms = timed(device_call, args.runs)
    host_ms, found = [], None
    for _ in range(args.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = host_call()
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    host_ms = round(statistics.median(host_ms), 3)
    same = [c.tolist() for c in cs.to_list()] == [sorted(c.tolist()) for c in found]
    kept = ~torch.isin(labels, ignore)
    table_bytes = int(kept.sum()) * nsample * 8  # the (n, nsample) int64 tables of all labels together
    # the serial tail: one workgroup scans the runs, so the same points with a random label per voxel (components of a
    # few points, min_cluster_size 1: every run is kept) show what many tiny components cost
    g = torch.Generator().manual_seed(1)
    noisy = torch.where(kept, torch.randint(1, 9, labels.shape, generator=g).to(dev), labels)

    def tiny_call():
        return tp.region_grow_csr(pos, noisy, batch, ignore_labels=ignore, radius=radius, nsample=nsample, min_cluster_size=1)

    tiny = tiny_call()
    tiny_ms = timed(tiny_call, args.runs)
    result = {"workload": "region_grow", "clouds": args.clouds, "points": int(pos.shape[0]),
              "non_stuff_points": int(kept.sum()), "lattice_step": H, "radius": radius, "nsample": nsample,
              "min_cluster_size": min_size, "clusters": len(cs), "clustered_points": int(cs.members.numel()),
              "route": cs.route, "same_clusters_as_host_path": bool(same),
              "ms": {"region_grow_csr": device_ms, "region_grow_host_path": host_ms},
              "timer": {"region_grow_csr": "hip events, median of %d" % args.runs,
                        "region_grow_host_path": "wall clock + synchronise, median of %d" % args.host_runs},
              "ratio": round(host_ms / device_ms, 2), "table_copy_bytes_saved": table_bytes,
              "device_to_host_bytes": 32,
              "many_small_components": {"clusters": len(tiny), "min_cluster_size": 1, "route": tiny.route,
                                        "region_grow_csr_ms": tiny_ms}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
