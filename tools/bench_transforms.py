"""Batch-building timings on one MI355X: the kernels of csrc/transforms.hip (torchpoints.region_cut / elastic_distort,
transforms.SceneSampler) against
  * the same cut as a torch composition on the device: a broadcast mask and `nonzero` per region, and
  * the host path the reference takes (wall clock, median of 5 runs): `KDTree.query_radius` on a prebuilt tree where
    sklearn imports (numpy brute force otherwise), indexing, the host-to-device copy of the sample; for the warp
    scipy's convolve + RegularGridInterpolator per cloud where scipy imports, plus the copy.
Shapes: one area of 10^6 points (40 x 40 x 5 m); B = 8 spheres and B = 8 cylinders of radius 2 at random points; the
2 m grid of test spheres; `outside_all` with 10 spheres; elastic_distort on 8 x 65 536 rows at granularity 0.2 / 0.8; a
full SceneSampler.sample(8) followed by the ScanNet-sparse augmentation chain.
Device calls are bracketed by HIP events after a warm-up; the median of --iters (30) calls is reported with the spread.
Calls without `capacity` include their one host read.  The baseline is never the code under test.  Needs a GPU.

    python tools/bench_transforms.py [--iters 30] [--out profiles/transforms_bench.json]
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


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def wall(fn, runs=5):
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3)


def optional(name):
    try:
        return __import__(name, fromlist=["x"])
    except ImportError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transforms needs a GPU: nothing is measured without one")
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd import transforms as TR
    from torch_points3d_amd.dense import Data
    neighbors, ndimage, interpolate = optional("sklearn.neighbors"), optional("scipy.ndimage"), optional("scipy.interpolate")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    N, R = 1000000, 2.0
    pos_h = torch.rand(N, 3, generator=gen) * torch.tensor([40.0, 40.0, 5.0])
    y_h = torch.randint(0, 13, (N,), generator=gen)
    rgb_h = torch.rand(N, 3, generator=gen)
    pos, y, rgb = pos_h.to(dev), y_h.to(dev), rgb_h.to(dev)
    pos_np = pos_h.numpy()
    result = {"workload": "transforms", "iters": args.iters, "points": N,
              "timer": "HIP events around one call, median; host paths: wall clock, median of 5",
              "host_search": "sklearn KDTree.query_radius (tree prebuilt, not timed)" if neighbors else "numpy brute force"}
    tree3 = neighbors.KDTree(pos_np, leaf_size=50) if neighbors else None
    tree2 = neighbors.KDTree(pos_np[:, :2], leaf_size=50) if neighbors else None

    def host_query(c, kind):
        if neighbors:
            return (tree3.query_radius(c[None], r=R) if kind == "sphere" else tree2.query_radius(c[None, :2], r=R))[0]
        d = pos_np - c
        return np.nonzero((d[:, :2] ** 2).sum(1) + (0 if kind == "cylinder" else d[:, 2] ** 2) <= R * R)[0]

    def host_sample(centres, kind):
        for c in centres:
            ind = torch.from_numpy(host_query(c, kind))
            _ = (pos_h[ind] - torch.from_numpy(c)).to(dev), y_h[ind].to(dev), rgb_h[ind].to(dev)

    def composed(centres_d, kind):
        out = []
        for b in range(centres_d.shape[0]):
            d = pos - centres_d[b]
            d2 = (d[:, :2] ** 2).sum(1) if kind == "cylinder" else (d ** 2).sum(1)
            ind = torch.nonzero(d2 <= R * R)[:, 0]
            out.append((ind, pos[ind] - centres_d[b]))
        return out

    # ---- B = 8 spheres / cylinders at random points: cut + gather of pos, y, rgb
    result["cut"] = []
    for kind in ("sphere", "cylinder"):
        rows = torch.randint(0, N, (8,), generator=gen)
        c_h, c_d = pos_np[rows.numpy()], pos[rows.to(dev)]

        def device_cut(capacity=None):
            cut = tp.region_cut(pos, c_d, R, kind=kind, closed=True, align_origin=True, capacity=capacity)
            return cut, y.index_select(0, cut.index), rgb.index_select(0, cut.index)

        cut = device_cut()[0]
        ref = composed(c_d, kind)
        # (the composition's predicate is fp32: a row within rounding of the radius may differ, so this is recorded)
        ref_index = torch.cat([r[0] for r in ref])
        same = bool(ref_index.shape == cut.index.shape and torch.equal(cut.index, ref_index))
        T = int(cut.status[0])
        k = timed(device_cut, args.iters)
        kc = timed(lambda: device_cut(capacity=T + 1024), args.iters)
        t = timed(lambda: composed(c_d, kind), args.iters)
        h = wall(lambda: host_sample(c_h, kind))
        result["cut"].append({"kind": kind, "B": 8, "radius": R, "rows_out": T, "equals_torch_composition": same, "kernel": k,
                              "kernel_with_capacity": kc,
                              "torch_device": t, "host_path_ms": h, "speedup_vs_torch_device": round(t["ms"] / k["ms"], 2),
                              "speedup_vs_host_path": round(h / k["ms"], 1)})

    # ---- the 2 m grid of test spheres (every region of one area)
    grid = TR.GridSphereSampling(R, R, center=False)
    area = Data(pos=pos, y=y)
    centres, cb = grid.centres(area)
    K = centres.shape[0]
    per_call = max(1, min(K, (2 ** 31 - 1) // N))
    seg = torch.tensor([0, N], device=dev)

    def all_regions():
        total = 0
        for lo in range(0, K, per_call):
            cut = tp.region_cut(pos, centres[lo:lo + per_call].contiguous(), R, closed=True, with_pos=False)
            total += cut.index.shape[0]
        return total

    rows_out = all_regions()
    sub = centres[:32].contiguous()
    sub_h = sub.cpu().numpy()
    result["grid_spheres"] = {"regions": K, "rows_out": rows_out, "calls": -(-K // per_call),
                              "kernel": timed(all_regions, max(3, args.iters // 10), warmup=1),
                              "first_32_regions": {"torch_device": timed(lambda: composed(sub, "sphere"), 5, warmup=1),
                                                   "host_path_ms": wall(lambda: host_sample(sub_h, "sphere"), runs=3),
                                                   "kernel": timed(lambda: tp.region_cut(pos, sub, R, closed=True), args.iters)},
                              "note": "the baselines loop over regions: timed on the first 32 only, the kernel on those "
                                      "and on all of them"}

    # ---- outside_all with 10 spheres (RandomSphereDropout's shape)
    rows = torch.randint(0, N, (10,), generator=gen)
    c_d, c_h = pos[rows.to(dev)], pos_np[rows.numpy()]

    def composed_drop():
        keep = torch.ones(N, dtype=torch.bool, device=dev)
        for b in range(10):
            keep &= ((pos - c_d[b]) ** 2).sum(1) >= R * R
        return torch.nonzero(keep)[:, 0]

    def host_drop():
        keep = np.ones(N, dtype=bool)
        for c in c_h:
            keep[host_query(c, "sphere")] = False
        m = torch.from_numpy(keep)
        _ = pos_h[m].to(dev), y_h[m].to(dev), rgb_h[m].to(dev)

    drop = tp.region_cut(pos, c_d, R, mode="outside_all", seg=seg)
    same = bool(torch.equal(drop.index, composed_drop()))
    k, t, h = timed(lambda: tp.region_cut(pos, c_d, R, mode="outside_all", seg=seg), args.iters), timed(composed_drop, args.iters), wall(host_drop)
    result["outside_all"] = {"spheres": 10, "rows_out": int(drop.status[0]), "equals_torch_composition": same, "kernel": k,
                             "torch_device": t, "host_path_ms": h, "speedup_vs_torch_device": round(t["ms"] / k["ms"], 2),
                             "speedup_vs_host_path": round(h / k["ms"], 1),
                             "note": "index list only; the host path also gathers and copies pos, y, rgb"}

    # ---- elastic distortion: 8 clouds of 65 536 rows in a 4 m sphere, the YAML's granularities
    B, n = 8, 65536
    cloud = (torch.rand(B * n, 3, generator=gen) * 4.0)
    cloud_d = cloud.to(dev)
    eseg = torch.arange(B + 1, dtype=torch.int64) * n
    eseg_d = eseg.to(dev)
    result["elastic"] = []
    for g, mag in ((0.2, 0.4), (0.8, 1.6)):
        _, grids = tp.elastic_distort(cloud, eseg, g, mag, generator=torch.Generator().manual_seed(1), return_grids=True)
        noise = torch.randn(int(grids.goff[-1]), generator=torch.Generator().manual_seed(1))
        noise_d = noise.to(dev)

        def host_warp():
            """the warp with scipy's routines, cloud by cloud, and the copy of the result: two rounds of a 3-tap mean
            per spatial axis (correlate1d, zero padding), interpn over the operator's own axis table"""
            third = np.float32(1) / np.float32(3)
            for b in range(B):
                coords = cloud[b * n:(b + 1) * n].numpy()
                d = grids.dims[b]
                nz = noise[grids.goff[b]:grids.goff[b + 1]].numpy().reshape(d[0], d[1], d[2], 3)
                for _ in range(2):
                    for axis in range(3):
                        nz = ndimage.correlate1d(nz, [third, third, third], axis=axis, mode="constant", cval=0.0)
                axes = [np.linspace(start, stop, int(m)) for (start, _, stop), m in zip(grids.axes[b], d)]
                shift = interpolate.interpn(axes, nz, coords, method="linear", bounds_error=False, fill_value=0.0)
                _ = torch.from_numpy((coords + shift * mag).astype(np.float32)).to(dev)

        k = timed(lambda: tp.elastic_distort(cloud_d, eseg_d, g, mag, noise=noise_d), args.iters)
        h = wall(host_warp, runs=3) if ndimage and interpolate else None
        result["elastic"].append({"clouds": B, "rows_per_cloud": n, "granularity": g, "grid": grids.dims[0].tolist(), "kernel": k,
                                  "host_path_ms": h, "speedup_vs_host_path": None if h is None else round(h / k["ms"], 1),
                                  "note": "kernel: bounds reduction + its host read + blur + warp; no torch-composition "
                                          "baseline was written for the warp"})

    # ---- a full sample(8) + the ScanNet-sparse augmentation chain
    half = N // 2
    sampler = TR.SceneSampler([Data(pos=pos[:half], y=y[:half], rgb=rgb[:half]), Data(pos=pos[half:], y=y[half:], rgb=rgb[half:])],
                              radius=R, kind="sphere", sample_per_epoch=3000)
    chain = [TR.ElasticDistortion(granularity=[0.2, 0.8], magnitude=[0.4, 1.6]),
             TR.Random3AxisRotation(rot_x=8, rot_y=8, rot_z=180), TR.RandomSymmetry(axis=[True, True, False]),
             TR.RandomScaleAnisotropic(scales=[0.9, 1.1]), TR.RandomNoise(sigma=0.01, clip=0.05)]
    g2 = torch.Generator().manual_seed(2)

    def sample_only():
        return sampler.sample(8, g2)

    def sample_and_augment():
        data = sampler.sample(8, g2)
        for t in chain:
            data = t(data, g2)
        return data

    result["sample_and_chain"] = {"B": 8, "radius": R, "areas": 2, "centres": int(sampler.centres.shape[0]),
                                  "sample": timed(sample_only, args.iters), "sample_and_chain": timed(sample_and_augment, args.iters),
                                  "host_sample_ms": wall(lambda: host_sample(pos_np[torch.randint(0, N, (8,), generator=gen).numpy()], "sphere")),
                                  "chain": "ElasticDistortion[0.2, 0.8] -> Random3AxisRotation(8, 8, 180) -> RandomSymmetry(x, y) "
                                           "-> RandomScaleAnisotropic(0.9, 1.1) -> RandomNoise(0.01, 0.05)",
                                  "note": "host_sample_ms: 8 KDTree spheres + gather + copy, without any augmentation"}
    result["not_timed"] = ["more than one GPU", "the reference's host augmentation chain as a whole", "box / ellipsoid crops",
                           "GridCylinderSampling", "building the KDTree (host path) and the centre table (SceneSampler)"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
