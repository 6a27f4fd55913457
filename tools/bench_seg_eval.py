"""Segmentation-evaluation timings on one MI355X: the kernels of csrc/seg_metrics.hip against
  * the torch composition on the device (argmax + bincount, indexed add, kNN interpolation + argmax + bincount), and
  * the host path the reference takes: the device-to-host copy of the scores plus the numpy restatement of its counting
    (wall clock, median of 5 runs; it ends in host work, so there is nothing to synchronise).
Shapes: confusion at (10^6, 13), (10^6, 19), (65 536, 50); part counts at 32 x 2048 x 50; vote_add of 2 * 10^5 rows into
10^6 targets (13 classes); full-resolution finalise at 10^6 raw points with a quarter covered (its host path runs once
and uses the project's host kNN, the reference's torch_cluster not being installed).
Device calls are bracketed by HIP events after a warm-up; the median of --iters (30) calls is reported with the spread.
`bytes` is the traffic the algorithm needs (inputs read once, counters excluded), `gbps` that over the kernel's median.
The baseline is never the code under test.  Needs a GPU (no fallback).

    python tools/bench_seg_eval.py [--iters 30] [--out profiles/seg_eval_bench.json]
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


def row(kernel, torch_dev, host_ms, nbytes, **shape):
    out = dict(shape, kernel=kernel, torch_device=torch_dev, host_path_ms=host_ms, bytes=int(nbytes),
               gbps=round(nbytes / kernel["ms"] / 1e6, 1),
               speedup_vs_torch_device=round(torch_dev["ms"] / kernel["ms"], 2))
    if host_ms is not None:
        out["speedup_vs_host_path"] = round(host_ms / kernel["ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_eval needs a GPU: nothing is measured without one")
    from torch_points3d_amd import seg_metrics as SM
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.partial_dense import knn_interpolate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    result = {"workload": "seg_eval", "iters": args.iters,
              "timer": "HIP events around one call, median; host paths: wall clock, median of 5"}

    # ---- confusion
    result["confusion"] = []
    for N, C in ((1000000, 13), (1000000, 19), (65536, 50)):
        scores = torch.log_softmax(torch.randn(N, C, generator=gen), 1).to(dev)
        labels = torch.randint(-1, C, (N,), generator=gen).to(dev)
        cm = torch.zeros(C * C + 1, dtype=torch.int64, device=dev)

        def composed():
            keep = labels != -1
            return torch.bincount(C * labels[keep] + scores[keep].argmax(1), minlength=C * C)

        def host():
            s, l = scores.cpu().numpy(), labels.cpu().numpy()
            keep = l != -1
            return np.bincount(C * l[keep] + np.argmax(s[keep], 1), minlength=C * C)

        tp.confusion_count(cm, labels, scores=scores, ignore_label=-1)
        assert torch.equal(cm[:C * C], composed()) and np.array_equal(cm[:C * C].cpu().numpy(), host())
        result["confusion"].append(row(
            timed(lambda: tp.confusion_count(cm, labels, scores=scores, ignore_label=-1), args.iters),
            timed(composed, args.iters), wall(host), N * (4 * C + 8), N=N, C=C))

    # ---- ShapeNet part counts
    B, n, C = 32, 2048, 50
    segs = {"c%d" % i: list(range(a, b)) for i, (a, b) in enumerate(
        [(0, 4), (4, 6), (6, 8), (8, 12), (12, 16), (16, 19), (19, 22), (22, 24), (24, 28), (28, 30), (30, 36), (36, 38),
         (38, 41), (41, 44), (44, 47), (47, 50)])}
    ev = SM.ShapenetPartEvaluator(segs)
    cats = [list(segs.values())[i % 16] for i in range(B)]
    labels = torch.stack([torch.tensor(c)[torch.randint(0, len(c), (n,), generator=gen)] for c in cats]).to(dev)
    scores = torch.log_softmax(torch.randn(B, n, C, generator=gen), 2).to(dev)
    seg = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    lo, hi = torch.from_numpy(ev._part_lo).to(dev), torch.from_numpy(ev._part_hi).to(dev)
    flat_s, flat_l = scores.reshape(B * n, C), labels.reshape(B * n)

    def composed_parts():
        out = torch.zeros(B, 16, 2, dtype=torch.int64, device=dev)
        for b in range(B):
            c = cats[b]
            p = scores[b][:, c[0]:c[-1] + 1].argmax(1) + c[0]
            for part in c:
                out[b, part - c[0], 0] = ((labels[b] == part) & (p == part)).sum()
                out[b, part - c[0], 1] = ((labels[b] == part) | (p == part)).sum()
        return out

    counts, _ = tp.part_iou_counts(flat_s, flat_l, seg, lo, hi, 6)
    assert torch.equal(counts.long(), composed_parts())
    host_parts = wall(lambda: SM.part_iou_counts_numpy(flat_s.cpu(), flat_l.cpu(), seg.cpu(), ev._part_lo, ev._part_hi))
    result["part_counts"] = row(timed(lambda: tp.part_iou_counts(flat_s, flat_l, seg, lo, hi, 6), args.iters),
                                timed(composed_parts, args.iters), host_parts, B * n * (4 * 4 + 8), B=B, N=n, C=C,
                                note="bytes: the category's columns (4 on average) and the labels; the torch "
                                     "composition is the tracker's loop over clouds and parts on device tensors")

    # ---- vote_add
    T, rows, C = 1000000, 200000, 13
    ids = torch.randperm(T, generator=gen)[:rows].to(dev)
    out = torch.randn(rows, C, generator=gen).to(dev)
    st = SM._Votes(T, C, dev)
    votes_t, counts_t = torch.zeros(T, C, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)

    def composed_vote():
        votes_t[ids] += out
        counts_t[ids] += 1

    def host_vote():
        i, o = ids.cpu(), out.cpu()
        host_vote.votes[i] += o
        host_vote.counts[i] += 1

    host_vote.votes, host_vote.counts = torch.zeros(T, C), torch.zeros(T, dtype=torch.int32)
    st.add(ids, out)
    composed_vote()
    assert torch.equal(st.votes, votes_t) and torch.equal(st.counts, counts_t)
    result["vote_add"] = row(timed(lambda: st.add(ids, out), args.iters), timed(composed_vote, args.iters),
                             wall(host_vote), rows * (8 + 8 + 4 * C + 8 * C + 8), rows=rows, targets=T, C=C)

    # ---- full-resolution finalise
    T, C = 1000000, 13
    pos = (torch.rand(T, 3, generator=gen) * torch.tensor([40.0, 40.0, 5.0])).to(dev)
    y = torch.randint(0, C, (T,), generator=gen).to(dev)
    ids = torch.randperm(T, generator=gen)[:T // 4].to(dev)
    out = torch.log_softmax(torch.randn(T // 4, C, generator=gen), 1).to(dev)

    def finalise():
        ev = SM.S3DISEvaluator(C, pos, y, stage="test")
        ev._test_area = area
        ev.finalise(full_res=True, vote_miou=False)
        return ev

    def composed_finalise():
        has = area.counts > 0
        full = knn_interpolate(area.votes[has], pos[has], pos, k=1)
        return torch.bincount(C * y + full.argmax(1), minlength=C * C).cpu()

    def host_finalise():
        v, c, p, labels = area.votes.cpu(), area.counts.cpu(), pos.cpu(), y.cpu().numpy()
        has = c > 0
        full = SM.knn_interpolate_numpy(v[has], p[has], p, 1)
        return np.bincount(C * labels + full.argmax(1).numpy(), minlength=C * C)

    area = SM._Votes(T, C, dev)
    area.add(ids, out)
    got = finalise().full_confusion_matrix.get_confusion_matrix()
    same = bool(np.array_equal(got.reshape(-1), composed_finalise().numpy()))
    result["finalise_full_res"] = {
        "raw_points": T, "covered": T // 4, "C": C, "matrix_equals_torch_composition": same,
        "kernel_path": timed(lambda: finalise().full_confusion_matrix.get_confusion_matrix(), args.iters),
        "torch_device": timed(composed_finalise, args.iters),
        "host_path_ms": wall(host_finalise, runs=1),
        "note": "both device paths run the project's kNN (k = 1) and end in the read of the matrix; the kernel path forms "
                "no (raw_points, C) matrix.  Host path: copies to the host, the project's host kNN (points_cpu, one "
                "thread) in place of the reference's torch_cluster, interpolation, argmax, bincount; one run"}
    r = result["finalise_full_res"]
    r["matrix_equals_host_path"] = bool(np.array_equal(got.reshape(-1), host_finalise()))
    r["speedup_vs_torch_device"] = round(r["torch_device"]["ms"] / r["kernel_path"]["ms"], 2)
    r["speedup_vs_host_path"] = round(r["host_path_ms"] / r["kernel_path"]["ms"], 1)
    result["not_timed"] = ["more than one GPU", "the reference's own torch_cluster kNN", "ScanNet / panoptic trackers"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
