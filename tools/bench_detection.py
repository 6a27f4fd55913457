"""Detection timings on one MI355X: the device path of torch_points3d_amd.votenet against the host path the reference
takes, restated in tests/votenet_ref.py / torch_points3d_amd/detection_cpu.py (wall clock, one run: it is a Python loop) --
  * `get_boxes(apply_nms=True)` at B = 8, P = 256, 18 classes, up to and including `to_list()`;
  * `box3d_iou` at (256, 64) and (4608, 64);
  * a full `DetectionEvaluator.finalise` over 312 synthetic scenes x 256 detections;
  * one `VoteNet("VoteNetPaper")` forward (eval) and training step at B = 8, N = 40000, and the loss's share of the step.
Device calls are bracketed by HIP events after a warm-up; the median of --iters (30) calls is reported with the spread.
The baseline is never the code under test.  Needs a GPU (no fallback).

    python tools/bench_detection.py [--iters 30] [--out profiles/detection_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t) * 1e3, 2)


def random_results(V, B, P, C, gen, dev):
    f = dict(center=torch.rand(B, P, 3, generator=gen) * 4, heading_scores=torch.randn(B, P, 1, generator=gen),
             heading_residuals=torch.randn(B, P, 1, generator=gen) * 0.3, size_scores=torch.randn(B, P, C, generator=gen),
             size_residuals=torch.randn(B, P, C, 3, generator=gen) * 0.05, objectness_scores=torch.randn(B, P, 2, generator=gen) * 2,
             sem_cls_scores=torch.randn(B, P, C, generator=gen))
    res = V.VoteNetResults(**{k: v.to(dev) for k, v in f.items()})
    res.has_class = True
    return res, {k: v.numpy() for k, v in f.items()}


def random_corners(V, n, gen, spread):
    return V.box_corners_from_param(torch.rand(n, 3, generator=gen) * 0.8 + 0.4, torch.rand(n, generator=gen) * 6.28 - 3.14,
                                    torch.rand(n, 3, generator=gen) * spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-net", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detection needs a GPU: nothing is measured without one")
    import votenet_ref as vr
    from torch_points3d_amd import detection_cpu
    from torch_points3d_amd import votenet as V
    from torch_points3d_amd.dense import Data
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    result = {"workload": "detection", "iters": args.iters, "timer": "HIP events around one call, median; host paths: wall clock, one run"}

    # ---- get_boxes
    B, P, C = 8, 256, 18
    mean_size = (torch.rand(C, 3, generator=gen) * 0.8 + 0.3)
    res, fields = random_results(V, B, P, C, gen, dev)

    class DS(object):
        mean_size_arr = mean_size.to(dev)

    got = res.get_boxes(DS(), apply_nms=True).to_list()
    want, host_ms = wall(lambda: vr.get_boxes(fields, mean_size.numpy(), None, 1, apply_nms=True))
    assert [len(s) for s in got] == [len(s) for s in want], "device and host paths keep different boxes"
    result["get_boxes"] = {"B": B, "P": P, "classes": C, "kept": sum(len(s) for s in got), "host_loop_ms": host_ms,
                           "device_to_boxset": timed(lambda: res.get_boxes(DS(), apply_nms=True), args.iters),
                           "device_to_list": timed(lambda: res.get_boxes(DS(), apply_nms=True).to_list(), args.iters)}
    result["get_boxes"]["speedup_to_list"] = round(host_ms / result["get_boxes"]["device_to_list"]["ms"], 1)

    # ---- box3d_iou
    result["box3d_iou"] = []
    for n, m in ((256, 64), (4608, 64)):
        a, b = random_corners(V, n, gen, 3.0), random_corners(V, m, gen, 3.0)
        dev_out = V.box3d_iou(a.to(dev), b.to(dev))
        host_out, host_ms = wall(lambda: detection_cpu.box3d_iou(a.numpy(), b.numpy()))
        row = {"n": n, "m": m, "host_ms": host_ms, "max_abs_diff": float(np.abs(dev_out.cpu().numpy() - host_out).max()),
               "device": timed(lambda: V.box3d_iou(a.to(dev), b.to(dev)), args.iters)}
        row["speedup"] = round(host_ms / row["device"]["ms"], 1)
        result["box3d_iou"].append(row)

    # ---- finalise over a validation pass
    S, D, G = 312, 256, 12
    gt_c = random_corners(V, S * G, gen, 4.0)
    pick = torch.randint(0, G, (S, D), generator=gen) + torch.arange(S).unsqueeze(1) * G
    det_c = gt_c[pick.reshape(-1)] + torch.randn(S * D, 1, 3, generator=gen) * 0.25
    gt_cls = torch.randint(0, C, (S * G,), generator=gen)
    det_cls = torch.where(torch.rand(S * D, generator=gen) < 0.7, gt_cls[pick.reshape(-1)], torch.randint(0, C, (S * D,), generator=gen))
    det_score = torch.rand(S * D, generator=gen)

    def sets(device):
        det = V.BoxSet(det_c.to(device), det_cls.to(device), torch.arange(S).repeat_interleave(D).to(device),
                       torch.ones(S * D, dtype=torch.bool, device=device), S, det_score.to(device))
        gt = V.BoxSet(gt_c.to(device), gt_cls.to(device), torch.arange(S).repeat_interleave(G).to(device),
                      torch.ones(S * G, dtype=torch.bool, device=device), S)
        return det, gt

    def finalise(device):
        ev = V.DetectionEvaluator()
        ev.add(*sets(device))
        return ev.finalise([0.25, 0.5])

    dev_ap = finalise(dev)[2]
    host_ap, host_ms = wall(lambda: finalise("cpu")[2])
    diff = max(abs(dev_ap[t][c] - host_ap[t][c]) for t in dev_ap for c in dev_ap[t])
    result["finalise"] = {"scenes": S, "detections_per_scene": D, "gt_per_scene": G, "classes": C, "host_numpy_ms": host_ms,
                          "max_abs_diff_ap": diff, "device": timed(lambda: finalise(dev), args.iters)}
    result["finalise"]["speedup"] = round(host_ms / result["finalise"]["device"]["ms"], 1)

    # ---- the network
    if not args.skip_net:
        B, N, K = 8, 40000, 64
        pos = (torch.rand(B, N, 3, generator=gen) * torch.tensor([8.0, 8.0, 3.0])).to(dev)
        labels = dict(center_label=(torch.rand(B, K, 3, generator=gen) * torch.tensor([8.0, 8.0, 3.0])).to(dev),
                      heading_class_label=torch.zeros(B, K, dtype=torch.int64, device=dev),
                      heading_residual_label=torch.zeros(B, K, device=dev),
                      size_class_label=torch.randint(0, C, (B, K), generator=gen).to(dev),
                      size_residual_label=(torch.randn(B, K, 3, generator=gen) * 0.05).to(dev),
                      sem_cls_label=torch.randint(0, C, (B, K), generator=gen).to(dev),
                      box_label_mask=(torch.rand(B, K, generator=gen) < 0.3).long().to(dev),
                      vote_label=(torch.randn(B, N, 9, generator=gen) * 0.3).to(dev),
                      vote_label_mask=(torch.rand(B, N, generator=gen) < 0.4).long().to(dev),
                      instance_box_corners=torch.zeros(B, K, 8, 3, device=dev))
        torch.manual_seed(0)
        net = V.VoteNet("VoteNetPaper", feat=0, num_classes=C, mean_size_arr=mean_size.numpy()).to(dev)
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)

        def fwd():
            net.eval()
            with torch.no_grad():
                return net(Data(pos=pos, x=None))

        def step():
            net.train()
            opt.zero_grad(set_to_none=True)
            net(Data(pos=pos, x=None), labels=dict(labels))
            net.losses["loss"].backward()
            opt.step()

        net.train()
        out = net(Data(pos=pos, x=None), labels=dict(labels))

        def loss_only():
            leaves = V.VoteNetResults(**{k: (v.detach().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point()
                                             else v) for k, v in out.__dict__.items()})
            V.get_loss(dict(labels), leaves, net.loss_params)["loss"].backward()

        result["net"] = {"model": "VoteNetPaper", "B": B, "N": N, "forward": timed(fwd, args.iters), "train_step": timed(step, args.iters),
                         "loss_forward_backward": timed(loss_only, args.iters)}
        result["net"]["loss_share_of_step"] = round(result["net"]["loss_forward_backward"]["ms"] / result["net"]["train_step"]["ms"], 3)
    result["not_timed"] = ["more than one GPU", "duplicate_boxes=True at full size", "the ScanNet loader"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
