"""Forward pass of the message-passing PointNet++ (`pointnet2` of conf/models/segmentation/pointnet2.yaml, FEAT = 3) on a
ragged batch: 32 clouds of 2048 .. 16384 points, eval mode, no gradient.

    python tools/bench_pointnet2_mp.py [--clouds 32] [--min 2048] [--max 16384] [--iters 10] [--config pointnet2]

Prints one JSON line:
  * forward_ms: host clock around `iters` forward passes ending in a device synchronise (after 2 warm-up passes);
  * split_ms: device time per pass of the library's entry points, bracketed one by one with HIP events
    (_lib.KernelTimer, in a run of its own: the brackets drain the stream, so this pass is slower than forward_ms),
    grouped as fps / search (ball query, table -> edges, kNN of the decoder) / edge rows + MLP (edge rows, GEMMs,
    BatchNorm) / pools (segmented max) / interpolation; torch's own kernels (cat, index, library GEMMs) are not in it;
  * fps_us_per_step: tp3d_fps_ragged_f32 against tp3d_fps_f32 on EQUAL clouds of the same total size (device events
    around `iters` calls), and the ragged batch itself.  One step = one selected point of the largest cloud.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = (("fps", ("tp3d_fps_",)),
          ("search", ("tp3d_ball_query_", "tp3d_table_edge_", "tp3d_knn_partial", "tp3d_knn_dense")),
          ("pools", ("tp3d_segment_max_",)),
          ("interpolation", ("tp3d_knn_interpolate_",)),
          ("edge_rows_mlp", ("tp3d_pointconv_rows_", "tp3d_gemm_", "tp3d_bn_")))


def group_of(name):
    for g, prefixes in GROUPS:
        if name.startswith(prefixes):
            return g
    return "other"


def device_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--min", type=int, default=2048)
    ap.add_argument("--max", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--config", default="pointnet2")
    ap.add_argument("--feat", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet2_mp.py measures on the GPU; none found")
    from torch_points3d_amd import _lib, torchpoints as tp
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.pointnet2_mp import PointNet2MP
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    sizes = torch.randint(args.min, args.max + 1, (args.clouds,), generator=g)
    sizes[0], sizes[-1] = args.min, args.max
    total = int(sizes.sum())
    pos = (torch.rand(total, 3, generator=g) * 2 - 1).to(dev)
    x = torch.randn(total, args.feat, generator=g).to(dev)
    batch = torch.repeat_interleave(torch.arange(args.clouds), sizes).to(dev)
    torch.manual_seed(0)
    net = PointNet2MP(args.config, args.feat, 13).to(dev).eval()

    def forward():
        with torch.no_grad():
            return net(PDData(pos=pos, batch=batch, x=x))

    for _ in range(2):
        out = forward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = forward()
    torch.cuda.synchronize()
    forward_ms = (time.perf_counter() - t0) * 1e3 / args.iters

    timer = _lib.KernelTimer()
    prev = _lib.set_timer(timer)
    try:
        for _ in range(args.iters):
            forward()
        torch.cuda.synchronize()
    finally:
        _lib.set_timer(prev)
    split, calls = {}, {}
    for (name, _sizes), (n, ms) in timer.summary().items():
        k = group_of(name)
        split[k] = split.get(k, 0.0) + ms / args.iters
        calls[k] = calls.get(k, 0) + n // args.iters

    # ragged FPS against the dense kernel on equal clouds of the same total size (first level: ratio of the config)
    ratio = 0.25 if args.config == "pointnet2ms" else 0.2
    n_eq = total // args.clouds
    eq = pos[: n_eq * args.clouds].reshape(args.clouds, n_eq, 3).contiguous()
    eq_batch = torch.repeat_interleave(torch.arange(args.clouds, device=dev), n_eq)
    quota = int(tp.fps_quota([n_eq], ratio)[0])
    dense_ms = device_ms(lambda: tp.furthest_point_sample(eq, quota), args.iters)
    ragged_eq_ms = device_ms(lambda: tp.fps_ragged(eq.reshape(-1, 3), eq_batch, ratio=ratio), args.iters)
    ragged_ms = device_ms(lambda: tp.fps_ragged(pos, batch, ratio=ratio), args.iters)
    assert torch.equal(tp.fps_ragged(eq.reshape(-1, 3), eq_batch, ratio=ratio).view(args.clouds, quota),
                       tp.furthest_point_sample(eq, quota) + (torch.arange(args.clouds, device=dev) * n_eq).unsqueeze(1))
    steps_ragged = int(tp.fps_quota([int(sizes.max())], ratio)[0])
    print(json.dumps({
        "workload": "pointnet2_mp_forward", "config": args.config, "clouds": args.clouds, "points": total,
        "smallest": int(sizes.min()), "largest": int(sizes.max()), "out_rows": int(out.shape[0]),
        "forward_ms": round(forward_ms, 3),
        "split_ms": {k: round(v, 3) for k, v in sorted(split.items())},
        "split_calls": calls,
        "fps_us_per_step": {
            "dense_equal_clouds": round(dense_ms * 1e3 / quota, 3), "ragged_equal_clouds": round(ragged_eq_ms * 1e3 / quota, 3),
            "equal_cloud_points": n_eq, "equal_cloud_steps": quota,
            "ragged_batch": round(ragged_ms * 1e3 / steps_ragged, 3), "ragged_batch_steps": steps_ragged},
    }))


if __name__ == "__main__":
    main()
