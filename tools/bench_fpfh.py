"""FPFH on the device: what each piece costs, the grid search next to the whole-cloud scan it replaces, and the whole
call next to the numpy path on the host.

  fragment   one cloud of --points (100000) rows on two noisy 3 m x 3 m sheets 1 m apart (sigma 0.01): a 0.3 ball holds
             ~1500 rows, more than the 1024 candidate slots of a wave, so the search compacts by selection
  defaults   conf/fpfh.yaml: radius 0.3, max_nn 256, radius_normal 0.093, max_nn_normal 17
  k128       the same at (0.3, 128)
  batch      8 fragments of --points / 5 rows in one call, at the defaults
  pieces     hybrid_search for the normals and for the features, normals_from_neighbours, spfh_counts, fpfh (all rows,
             float32), and the whole FPFH() call (all rows)
  knn256     torchpoints.knn(256) on the fragment: above k = 128 it scans the whole cloud, the only in-tree search that
             could feed max_nn = 256 before hybrid_search; median of --knn-runs (3) after one warm-up call
  knn128     torchpoints.knn(128), served from the grid, for the k128 row (no radius cut applied)
  numpy      the whole FPFH() call on CPU tensors at --points / 5 rows, defaults: wall clock, one run

HIP events, 3 warm-up calls, the median of --runs (30) calls, inputs resident.  Needs a GPU.

    python tools/bench_fpfh.py [--out profiles/fpfh_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparseconv import timed  # noqa: E402


def two_sheets(n, seed):
    g = np.random.default_rng(seed)
    p = g.random((n, 3)) * 3.0
    p[:, 2] = 0.01 * g.standard_normal(n) + (np.arange(n) % 2)
    return torch.from_numpy(p.astype(np.float32))


class Bag(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def pieces(tp, F, pos, batch, cfg, runs):
    r, k, rn, kn = cfg["radius"], cfg["max_nn"], cfg["radius_normal"], cfg["max_nn_normal"]
    idn, _, cn = tp.hybrid_search(pos, pos, rn, kn, batch, batch)
    idx, _, count = tp.hybrid_search(pos, pos, r, k, batch, batch)
    normals = tp.normals_from_neighbours(pos, idn, cn)
    counts = tp.spfh_counts(pos, normals, idx, count)
    f = F.FPFH(r, k, rn, kn)
    bag = Bag(pos=pos, batch=batch)
    row = {"rows": pos.shape[0], "clouds": 1 if batch is None else int(batch.max()) + 1, "config": cfg,
           "mean_count_normals": round(float(cn.float().mean()), 2), "mean_count": round(float(count.float().mean()), 2),
           "rows_cut_by_max_nn": round(float((count == k).float().mean()), 4),
           "search_normals_ms": timed(lambda: tp.hybrid_search(pos, pos, rn, kn, batch, batch), runs),
           "search_ms": timed(lambda: tp.hybrid_search(pos, pos, r, k, batch, batch), runs),
           "normals_ms": timed(lambda: tp.normals_from_neighbours(pos, idn, cn), runs),
           "spfh_counts_ms": timed(lambda: tp.spfh_counts(pos, normals, idx, count), runs),
           "fpfh_ms": timed(lambda: tp.fpfh(pos, normals, idx, count, counts), runs),
           "whole_call_ms": timed(lambda: f(bag), runs)}
    row["pair_features_per_s"] = round(float((count - 1).clamp(min=0).sum()) / (row["spfh_counts_ms"] * 1e-3), 0)
    a, b = f(bag), f(bag)
    row["repeat_bit_equal"] = bool(torch.equal(a, b))
    return row, (idx, count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--knn-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fpfh needs a GPU: nothing is measured without one")
    from torch_points3d_amd import fpfh as F
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    cfg = F.fpfh_config()
    result = {"workload": "fpfh", "timer": "hip events, 3 warm-up calls, median of %d (knn: 1 warm-up, median of %d)" % (
        args.runs, args.knn_runs), "input": "two noisy sheets of 3 m x 3 m, 1 m apart, sigma 0.01", "not_timed": []}
    pos = two_sheets(args.points, 1).to(dev)

    row, (idx, count) = pieces(tp, F, pos, None, cfg, args.runs)
    # the whole-cloud scan of the parent commit, and that both searches name the same neighbours inside the radius
    kidx, kd2 = tp.knn(cfg["max_nn"], pos, pos)
    inside = kd2 < float(np.float32(cfg["radius"]) * np.float32(cfg["radius"]))
    row["knn256_ms"] = timed(lambda: tp.knn(cfg["max_nn"], pos, pos), args.knn_runs, warmup=1)
    row["grid_search_equals_knn_cut_at_the_radius"] = bool(torch.equal(torch.where(inside, kidx, torch.full_like(kidx, -1)),
                                                                       idx.long()))
    row["knn256_over_search"] = round(row["knn256_ms"] / row["search_ms"], 1)
    del kidx, kd2, inside
    print(json.dumps(row), flush=True)
    result["defaults"] = row

    cfg128 = dict(cfg, max_nn=128)
    row, _ = pieces(tp, F, pos, None, cfg128, args.runs)
    row["knn128_ms"] = timed(lambda: tp.knn(128, pos, pos), args.runs)
    print(json.dumps(row), flush=True)
    result["k128"] = row

    n8 = args.points // 5
    pos8 = torch.cat([two_sheets(n8, 10 + b) for b in range(8)]).to(dev)
    batch8 = torch.arange(8, device=dev).repeat_interleave(n8)
    row, _ = pieces(tp, F, pos8, batch8, cfg, args.runs)
    print(json.dumps(row), flush=True)
    result["batch"] = row

    host = two_sheets(n8, 10)
    f = F.FPFH(**cfg)
    t0 = time.perf_counter()
    out_host = f(Bag(pos=host))
    result["numpy_host"] = {"rows": n8, "config": cfg, "whole_call_ms": round(1e3 * (time.perf_counter() - t0), 1),
                            "device_whole_call_ms": timed(lambda: f(Bag(pos=pos8[:n8])), args.runs)}
    out_dev = f(Bag(pos=pos8[:n8])).cpu()
    result["numpy_host"]["rows_within_1e-3_of_the_device"] = round(float(((out_dev - out_host).abs().max(1)[0] <= 1e-3).double().mean()), 4)
    print(json.dumps(result["numpy_host"]), flush=True)
    result["not_timed"] += ["open3d (not installed)", "keypoint subsets (rows=)", "the float64 output", "a viewpoint",
                            "the numpy path at the other shapes", "knn(256) on the batch of 8"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f_out:
            f_out.write(line + "\n")


if __name__ == "__main__":
    main()
