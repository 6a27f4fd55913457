"""TSDF fusion on the device: what one 3DMatch fragment costs, and what applying all its frames in one pass over the
volume is worth.

  fragment   --frames (50) raw uint16 depth frames of 640 x 480 (a wavy wall 1.2 .. 1.8 m away, 5 % holes) with slightly
             moved cameras, fused into a cube of 2.56 m at 256^3 and 512^3 voxels
  (a) multi     one tsdf_integrate call with all frames: every volume element is read and written once
  (b) single    the same kernel called once per frame (F = 1): what the reference's one-launch-per-frame loop costs
  (c) surface   tsdf_surface(0.35, 0.0) of the fused volume (count + scan + emit, and the one host read)
  (d) unproject depth_unproject of the 50 frames
  (e) numpy     the host path (tsdf.integrate_numpy) on the same frames at 128^3: wall clock, one run

Reported next to (a): the bytes of the two volume streams (read + write of tsdf and weight: 16 bytes per voxel) per
second of (a).  HIP events, 3 warm-up calls, the median of --runs (30) calls, inputs resident.  Needs a GPU.

    python tools/bench_tsdf.py [--out profiles/tsdf_bench.json]
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

H, W = 480, 640
SIDE = 2.56


def scene(frames, seed=1):
    g = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    depths, poses = [], []
    for f in range(frames):
        z = 1.5 + 0.2 * np.sin(u / 90.0 + 0.2 * f) + 0.1 * np.cos(v / 70.0 - 0.1 * f)
        raw = np.round(z * 1000.0).astype(np.uint16)
        raw[g.random((H, W)) < 0.05] = 0
        a = 0.02 * f - 0.5
        p = np.eye(4)
        p[:3, :3] = [[np.cos(a * 0.2), 0, np.sin(a * 0.2)], [0, 1, 0], [-np.sin(a * 0.2), 0, np.cos(a * 0.2)]]
        p[:3, 3] = (0.1 * a, 0.02 * np.sin(f), 0.01 * f)
        depths.append(raw)
        poses.append(p)
    K = np.array([[585.0, 0.0, 320.0], [0.0, 585.0, 240.0], [0.0, 0.0, 1.0]])
    return np.stack(depths), np.stack(poses), K


def volumes(dim, device):
    return (torch.ones((dim,) * 3, dtype=torch.float32, device=device),
            torch.zeros((dim,) * 3, dtype=torch.float32, device=device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--host-dim", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs a GPU: nothing is measured without one")
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    raw, poses, K = scene(args.frames)
    d = torch.from_numpy(raw.view(np.int16).copy()).view(torch.uint16).to(dev)
    F = args.frames
    origin = np.array([-0.5 * SIDE, -0.5 * SIDE, 0.3], np.float32)
    result = {"workload": "tsdf", "timer": "hip events, 3 warm-up calls, median of %d" % args.runs,
              "input": "%d frames of %d x %d raw uint16 depth, a cube of %.2f m" % (F, W, H, SIDE), "shapes": []}
    for dim in args.dims:
        vs = SIDE / dim
        t, w = volumes(dim, dev)

        def multi():
            tp.tsdf_integrate(t, w, origin, vs, d, K, poses, 1.0, depth_thresh=6)

        def single():
            for f in range(F):
                tp.tsdf_integrate(t, w, origin, vs, d[f:f + 1], K, poses[f:f + 1], 1.0, depth_thresh=6)

        row = {"dim": dim, "voxels": dim ** 3, "voxel_size": vs, "frames": F,
               "launches_multi": -(-F // tp.tsdf_max_frames())}
        row["multi_ms"] = timed(multi, args.runs)
        row["single_ms"] = timed(single, args.runs)
        row["single_over_multi"] = round(row["single_ms"] / row["multi_ms"], 2)
        volume_bytes = 16 * dim ** 3
        row["two_volume_bytes"] = volume_bytes
        row["multi_volume_bytes_per_s"] = round(volume_bytes / (row["multi_ms"] * 1e-3), 0)
        row["single_volume_bytes_per_s"] = round(F * volume_bytes / (row["single_ms"] * 1e-3), 0)
        row["voxel_frame_updates_per_s"] = round(F * dim ** 3 / (row["multi_ms"] * 1e-3), 0)
        # one fragment from fresh volumes, both ways: the same bits
        t.fill_(1.0), w.zero_()
        multi()
        t1, w1 = t.clone(), w.clone()
        t.fill_(1.0), w.zero_()
        single()
        row["multi_equals_single"] = bool(torch.equal(t, t1) and torch.equal(w, w1))
        del t1, w1
        row["surface_rows"] = int(tp.tsdf_surface(t, w, origin, vs, 0.35, 0.0, with_index=False).status[0])
        row["surface_ms"] = timed(lambda: tp.tsdf_surface(t, w, origin, vs, 0.35, 0.0, with_index=False), args.runs)
        row["touched_fraction"] = round(float((w > 0).float().mean()), 4)
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        del t, w
        torch.cuda.empty_cache()

    res = tp.depth_unproject(d, K, poses)
    result["unproject"] = {"frames": F, "pixels": F * H * W, "rows": int(res.status[0]),
                           "ms": timed(lambda: tp.depth_unproject(d, K, poses), args.runs)}
    print(json.dumps(result["unproject"]), flush=True)

    hd = args.host_dim
    th, wh = volumes(hd, "cpu")
    dh = torch.from_numpy(raw.astype(np.int32))
    t0 = time.perf_counter()
    tp.tsdf_integrate(th, wh, origin, SIDE / hd, dh, K, poses, 1.0, depth_thresh=6)
    host_ms = 1e3 * (time.perf_counter() - t0)
    t, w = volumes(hd, dev)
    tp.tsdf_integrate(t, w, origin, SIDE / hd, d, K, poses, 1.0, depth_thresh=6)
    result["numpy_host"] = {"dim": hd, "frames": F, "wall_ms": round(host_ms, 1),
                            "device_equals_host": bool(torch.equal(t.cpu(), th) and torch.equal(w.cpu(), wh))}
    t.fill_(1.0), w.zero_()
    result["numpy_host"]["device_ms"] = timed(
        lambda: tp.tsdf_integrate(t, w, origin, SIDE / hd, d, K, poses, 1.0, depth_thresh=6), args.runs)
    print(json.dumps(result["numpy_host"]), flush=True)
    result["not_timed"] = ["float64 depth frames", "get_3D_bound", "the whole rgbd2fragment_fine call", "the mesh (not served)"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f_out:
            f_out.write(line + "\n")


if __name__ == "__main__":
    main()
