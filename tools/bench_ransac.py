"""RANSAC registration: what the HIP path costs next to a torch composition kept on the device and next to the host.

  ransac_score   torchpoints.ransac_score (Horn poses + fp32 scoring + integer sums) at (N, H) = (5000, 80000) -- the
                 defaults of scripts/test_registration_scripts/evaluate.py --, (1000, 80000) and (5000, 10000), samples of 4
  ransac_pose    the whole solve (score, select, one refit, final stats), samples given
  kabsch         torchpoints.kabsch at N = 5000 against registration.estimate_transfo (torch.svd of the 3 x 3) on the device
  torch          the same hypotheses from torch ops on the device: batched torch.linalg.svd Kabsch over (H, 3, 3), scoring
                 by a broadcast matmul over chunks of --chunk hypotheses, argmax, Kabsch of the inliers by boolean mask.
                 The batched SVD is probed at H = 10000 first and left out above --svd-budget-s seconds per call
  numpy          registration._ransac_numpy (the CPU path of ransac_registration) at (5000, 10000): wall clock, one call

Inputs as tests/test_gpu_registration._fgr_case: 30 % outliers, noise 0.003; threshold 0.05.  HIP events, 3 warm-up calls,
the median of --runs (30) calls, inputs resident; the torch composition: median of --torch-runs (5).  Needs a GPU.

    python tools/bench_ransac.py [--out profiles/ransac_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparseconv import timed  # noqa: E402

THRESHOLD = 0.05


def case(n, seed):
    gen = torch.Generator().manual_seed(seed)
    T = torch.eye(4)
    T[:3, :3] = torch.linalg.matrix_exp(torch.tensor([[0.0, -0.3, 0.2], [0.3, 0.0, -0.4], [-0.2, 0.4, 0.0]]))
    T[:3, 3] = torch.tensor([0.2, -0.1, 0.3])
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    tgt = xyz @ T[:3, :3].T + T[:3, 3] + 0.003 * torch.randn(n, 3, generator=gen)
    bad = torch.randperm(n, generator=gen)[: (3 * n) // 10]
    tgt[bad] = torch.rand(len(bad), 3, generator=gen) * 3 - 1.5
    return xyz, tgt, T


def torch_poses(xyz, tgt, samples):
    """Kabsch with the determinant correction per hypothesis (utils/registration.py:24-43, batched)"""
    p, q = xyz[samples], tgt[samples]
    mp, mq = p.mean(1, keepdim=True), q.mean(1, keepdim=True)
    U, _, Vh = torch.linalg.svd((p - mp).transpose(1, 2) @ (q - mq))
    V, Ut = Vh.transpose(1, 2), U.transpose(1, 2)
    diag = torch.ones(len(samples), 3, device=xyz.device)
    diag[:, 2] = torch.det(V @ Ut)
    R = (V * diag[:, None, :]) @ Ut
    return R, mq.squeeze(1) - (R @ mp.transpose(1, 2)).squeeze(2)


def torch_counts(xyz, tgt, R, t, chunk):
    counts = torch.empty(len(R), dtype=torch.int64, device=xyz.device)
    for h0 in range(0, len(R), chunk):
        moved = xyz @ R[h0:h0 + chunk].transpose(1, 2) + t[h0:h0 + chunk, None, :] - tgt
        counts[h0:h0 + chunk] = (moved.pow(2).sum(2) < THRESHOLD * THRESHOLD).sum(1)
    return counts


def torch_ransac(reg, xyz, tgt, samples, chunk):
    R, t = torch_poses(xyz, tgt, samples)
    best = torch.argmax(torch_counts(xyz, tgt, R, t, chunk))
    inl = (xyz @ R[best].T + t[best] - tgt).pow(2).sum(1) < THRESHOLD * THRESHOLD
    return reg.estimate_transfo(xyz[inl], tgt[inl])  # (the boolean mask reads the inlier count back)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--torch-runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--svd-budget-s", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ransac needs a GPU: nothing is measured without one")
    from torch_points3d_amd import _lib
    from torch_points3d_amd import registration as reg
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    result = {"workload": "ransac", "threshold": THRESHOLD, "ransac_n": 4, "outliers": "30 %", "noise": 0.003,
              "timer": "hip events, 3 warm-up calls, median of %d (torch composition: median of %d)" % (args.runs, args.torch_runs),
              "shapes": [], "not_timed": []}

    xyz, tgt, _ = case(5000, 0)
    probe = torch.randint(0, 5000, (10000, 4), generator=torch.Generator().manual_seed(1)).to(dev)
    svd_ms = timed(lambda: torch_poses(xyz.to(dev), tgt.to(dev), probe), 3, warmup=1)
    result["torch_batched_kabsch_probe"] = {"H": 10000, "ms": svd_ms}
    print("batched torch Kabsch at H = 10000: %.3f ms" % svd_ms, flush=True)

    for N, H in ((5000, 80000), (1000, 80000), (5000, 10000)):
        xyz, tgt, T = case(N, N + H)
        samples = torch.randint(0, N, (H, 4), generator=torch.Generator().manual_seed(H))
        dx, dt, ds = xyz.to(dev), tgt.to(dev), samples.to(dev)
        poses, counts = tp.ransac_score(dx, dt, ds, THRESHOLD)
        T_hip, stats = tp.ransac_pose(dx, dt, THRESHOLD, samples=ds)
        row = {"N": N, "H": H, "splits_of_N": _lib.load().tp3d_ransac_splits(N, H),
               "ransac_score_ms": timed(lambda: tp.ransac_score(dx, dt, ds, THRESHOLD), args.runs),
               "ransac_pose_ms": timed(lambda: tp.ransac_pose(dx, dt, THRESHOLD, samples=ds), args.runs),
               "pair_tests_per_s": None, "best_count": int(stats["best_count"]), "inliers": int(stats["inliers"]),
               "translation_error": float((T_hip[:3, 3].cpu() - T[:3, 3]).norm())}
        row["pair_tests_per_s"] = round(N * H / (row["ransac_score_ms"] * 1e-3), 0)
        print(json.dumps(row), flush=True)
        if svd_ms * (H / 10000.0) * 1e-3 <= args.svd_budget_s:
            R, t = torch_poses(dx, dt, ds)
            c_ref = torch_counts(dx, dt, R, t, args.chunk)
            row["torch_score_ms"] = timed(lambda: torch_counts(dx, dt, *torch_poses(dx, dt, ds), args.chunk), args.torch_runs, warmup=1)
            row["torch_whole_ms"] = timed(lambda: torch_ransac(reg, dx, dt, ds, args.chunk), args.torch_runs, warmup=1)
            row["counts_differ_from_torch"] = int((c_ref != counts.long()).sum())
            row["counts_max_abs_diff"] = int((c_ref - counts.long()).abs().max())
            row["pose_max_abs_diff_from_torch"] = float((torch_ransac(reg, dx, dt, ds, args.chunk) - T_hip).abs().max())
        else:
            result["not_timed"].append("torch composition at (%d, %d): its batched SVD alone is %.1f s at H = 10000" % (N, H, svd_ms * 1e-3))
        if (N, H) == (5000, 10000):
            t0 = time.perf_counter()
            pose, best, c_np = reg._ransac_numpy(xyz.numpy(), tgt.numpy(), THRESHOLD, samples.numpy())
            row["numpy_host_whole_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            row["numpy_best_is_hip_best"] = bool(best == int(stats["best"]))
            row["pose_max_abs_diff_from_numpy"] = float((torch.from_numpy(pose).float() - T_hip[:3].cpu()).abs().max())
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)

    xyz, tgt, _ = case(5000, 7)
    dx, dt = xyz.to(dev), tgt.to(dev)
    w = torch.rand(5000, device=dev)
    result["kabsch"] = {"N": 5000, "kabsch_ms": timed(lambda: tp.kabsch(dx, dt), args.runs),
                        "kabsch_weighted_ms": timed(lambda: tp.kabsch(dx, dt, w), args.runs),
                        "estimate_transfo_on_device_ms": timed(lambda: reg.estimate_transfo(dx, dt), args.runs),
                        "pose_max_abs_diff": float((tp.kabsch(dx, dt) - reg.estimate_transfo(dx, dt)).abs().max())}
    result["not_timed"] += ["open3d's registration_ransac_based_on_correspondence (not installed)", "ransac_n other than 4",
                            "refine other than 1", "compute_metrics(use_ransac=True)", "the numpy path at the other two shapes"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
