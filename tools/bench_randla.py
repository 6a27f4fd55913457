"""RandLA-Net timings: the one-kernel eval-mode edge pass (csrc/randla_lfa.hip, `lfa="fused"`) against the row kernels
between rows_mlp calls it replaces (`lfa="rows"`, the code the tree had before it), at the three levels of
`Randlanet_Conv` (conf/models/segmentation/randlanet.yaml, FEAT = 3) on one scene of 10^6 points: 250 000 / 62 500 /
15 625 queries with 16 neighbours each, the exact kNN tables of the levels.  Per level: one RandlaKernel forward
(edge pass + global_nn; both routes read the table once on the host for -1 slots) per route, the one-kernel edge pass
alone, the allocator peak above the inputs, and the distance between the two outputs.  Then
`RandLANetSeg("Randlanet_Conv")`: the eval-mode forward at 10^6 points with `lfa="auto"` against `lfa="rows"` on the
same weights and draws, and one training step (forward, nll loss, backward, SGD update) at 65 536 points, which takes
the rows route whatever `lfa` says.

`randla.lfa_route` may answer "fused" only for a width class (C <= 16 / 32 / 64) whose fused time here is not above its
rows time: `width_class_wins` in the result is what `randla.LFA_MEASURED_WIN` has to say.

Times are HIP events around `--inner` back-to-back calls, the two routes alternated, the median of `--runs` (>= 20)
timed runs after a warm-up, all in one process.  Needs a GPU (no fallback).

    python tools/bench_randla.py [--points 1000000] [--train-points 65536] [--runs 30] [--inner 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEAT, CLASSES = 3, 13


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, runs, inner, warmup=3):
    """median ms per call (and max - min over the runs) of every function, the timed runs interleaved"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            times[k].append(timed(fn, inner))
    return ({k: round(statistics.median(v), 5) for k, v in times.items()},
            {k: round(max(v) - min(v), 5) for k, v in times.items()})


def peak_mib(fn):
    """allocator peak of one call above what is allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return round(rise / float(1 << 20), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--train-points", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("at least 20 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_randla needs a GPU: nothing is measured without one")
    from torch_points3d_amd import randla
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.kpconv_blocks import PDData
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    cfg = randla.randla_config("Randlanet_Conv", FEAT)["down_conv"]
    result = {"workload": "randla_lfa", "points": args.points, "runs": args.runs, "calls_per_run": args.inner,
              "timer": "HIP events, median of the runs", "baseline": "lfa='rows' (the row kernels between rows_mlp calls)",
              "levels": []}

    pos = torch.rand(args.points, 3, generator=gen).to(dev)
    batch = torch.zeros(args.points, dtype=torch.long, device=dev)
    x = torch.randn(args.points, FEAT, generator=gen).to(dev)
    wins = {}
    for level in range(3):
        pp, at, gl = cfg["point_pos_nn"][level], cfg["attention_nn"][level], cfg["down_conv_nn"][level]
        M = pos.shape[0]
        idx = torch.sort(torch.randint(0, M, (int(M * cfg["ratio"][level]),), generator=gen))[0].to(dev)
        pos_q = pos[idx]
        nbr, _ = tp.knn(16, pos, pos_q, batch, batch[idx])
        assert int(nbr.min()) >= 0
        torch.manual_seed(level)
        kers = {}
        for lfa in ("rows", "fused"):
            kers[lfa] = randla.RandlaKernel(point_pos_nn=list(pp), attention_nn=list(at), global_nn=list(gl), lfa=lfa)
            kers[lfa].load_state_dict(kers["rows"].state_dict())
            kers[lfa].to(dev).eval()
        C = x.shape[1] + pp[2]
        cls = randla.lfa_width_class(C)
        saved = dict(randla.LFA_MEASURED_WIN)
        randla.LFA_MEASURED_WIN[cls] = True  # measure the kernel whatever the table says today
        try:
            def fwd(lfa, x=x, pos_q=pos_q, pos=pos, nbr=nbr, kers=kers):
                with torch.no_grad():
                    return kers[lfa](x, (pos_q, pos), nbr)

            out_r, out_f = fwd("rows"), fwd("fused")
            diff = float((out_r - out_f).abs().max())
            def edge_pass(x=x, pos_q=pos_q, pos=pos, nbr=nbr, ker=kers["fused"]):
                return randla.randla_lfa_eval(pos_q, pos, x, nbr, ker.point_pos_nn, ker.attention_nn)

            ms, spread = alternate({"rows": lambda: fwd("rows"), "fused": lambda: fwd("fused"),
                                    "fused_edge_pass_alone": edge_pass}, args.runs, args.inner)
            peaks = {lfa: peak_mib(lambda lfa=lfa: fwd(lfa)) for lfa in ("rows", "fused")}
        finally:
            randla.LFA_MEASURED_WIN.update(saved)
        wins[str(cls)] = bool(ms["fused"] <= ms["rows"])
        result["levels"].append({
            "level": level + 1, "support": M, "queries": int(idx.numel()), "edges": int(idx.numel()) * 16, "Cx": x.shape[1],
            "point_pos_nn": pp, "attention_nn": at, "global_nn": gl, "C": C, "width_class": cls, "forward_ms": ms,
            "spread_ms": spread, "fused_over_rows": round(ms["fused"] / ms["rows"], 3), "allocator_peak_mib": peaks,
            "output_mib": round(idx.numel() * gl[-1] * 4 / float(1 << 20), 3), "max_abs_diff_rows_fused": diff,
            "output_scale": float(out_r.abs().max())})
        x, pos, batch = out_r, pos_q, batch[idx]
        del out_f, nbr
    result["width_class_wins"] = wins
    result["route_table_in_tree"] = {str(k): v for k, v in randla.LFA_MEASURED_WIN.items()}

    # ---- the network: eval forward at the full size, the two routes on the same weights and the same draws
    pos0 = torch.rand(args.points, 3, generator=gen).to(dev)
    x0 = torch.randn(args.points, FEAT, generator=gen).to(dev)
    batch0 = torch.zeros(args.points, dtype=torch.long, device=dev)
    torch.manual_seed(0)
    nets = {}
    for lfa in ("rows", "auto"):
        nets[lfa] = randla.RandLANetSeg("Randlanet_Conv", FEAT, CLASSES, lfa=lfa)
        nets[lfa].load_state_dict(nets["rows"].state_dict())
        nets[lfa].to(dev).eval()

    def net_fwd(lfa):
        torch.manual_seed(1)  # the same draws on both sides
        with torch.no_grad():
            return nets[lfa](PDData(pos=pos0, batch=batch0, x=x0))

    o_r, o_a = net_fwd("rows"), net_fwd("auto")
    ndiff = float((o_r - o_a).abs().max())
    del o_r, o_a
    ms, spread = alternate({"rows": lambda: net_fwd("rows"), "auto": lambda: net_fwd("auto")}, args.runs, 1, warmup=2)
    peaks = {lfa: peak_mib(lambda lfa=lfa: net_fwd(lfa)) for lfa in ("rows", "auto")}
    result["net_eval"] = {"config": "Randlanet_Conv", "classes": CLASSES, "points": args.points, "forward_ms": ms,
                          "spread_ms": spread, "auto_over_rows": round(ms["auto"] / ms["rows"], 3),
                          "allocator_peak_mib": peaks, "max_abs_diff_rows_auto": ndiff,
                          "includes": "the draws, their sort, kNN of every level, interpolation, head"}

    # ---- one training step (always the rows route)
    n = args.train_points
    pos1, x1 = pos0[:n].contiguous(), x0[:n].contiguous()
    batch1 = batch0[:n].contiguous()
    labels = torch.randint(0, CLASSES, (n,), generator=gen).to(dev)
    net = nets["auto"].train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)

    def step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.nll_loss(net(PDData(pos=pos1, batch=batch1, x=x1)), labels).backward()
        opt.step()

    ms, spread = alternate({"train_step": step}, args.runs, 1, warmup=3)
    result["net_train"] = {"points": n, "train_step_ms": ms["train_step"], "spread_ms": spread["train_step"],
                           "route": "rows (training mode)"}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
