"""Message-passing RSConv timings: the fused aggregation torchpoints.rsconv_msgmax (forward, forward + backward) against
the composition it replaces, segment_max(w * x[col]) from the operators the tree had before it, at the shapes of
RSConv_2LD (conf/models/segmentation/rsconv.yaml) on a batch of 8 clouds of 4096 points: level 1 (32768 support points,
ratio 0.2, C = 3: x_j = pos_j) and level 2 (6560 support points, ratio 0.25, C = 64), at most 64 neighbours, with the
YAML's radii on unit-cube clouds (most runs below the cap) and with twice the radius (most runs at the cap).  Then the
three pieces of one Convolution forward (relation rows, local_nn through fused.rows_mlp, the fused max) and the full
`RSConvMP("RSConv_2LD")` forward and training step (forward, nll loss, backward, SGD update).

Times are HIP events around `--inner` back-to-back calls, the two sides alternated, the median of `--runs` (>= 20)
timed runs after a warm-up, all in one process; their outputs are compared first (they must be bit-equal).  Needs a GPU
(no fallback).

    python tools/bench_rsconv_mp.py [--clouds 8] [--points 4096] [--runs 30] [--inner 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, runs, inner, warmup=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("at least 20 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rsconv_mp needs a GPU: nothing is measured without one")
    from torch_points3d_amd import fused
    from torch_points3d_amd import torchpoints as tp
    from torch_points3d_amd.kpconv_blocks import PDData
    from torch_points3d_amd.partial_dense import MLP
    from torch_points3d_amd.rsconv_mp import RSConvMP, rsconv_mp_config
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    pos0 = torch.rand(args.clouds * args.points, 3, generator=gen).to(dev)
    batch0 = torch.repeat_interleave(torch.arange(args.clouds), args.points).to(dev)
    cfg = rsconv_mp_config("RSConv_2LD")["down_conv"]
    result = {"workload": "rsconv_mp", "clouds": args.clouds, "points_per_cloud": args.points, "runs": args.runs,
              "calls_per_run": args.inner, "timer": "HIP events, median of the runs", "msgmax": [], "layer": []}

    idx1 = tp.fps_ragged(pos0, batch0, ratio=cfg["ratios"][0])
    pos1, batch1 = pos0[idx1], batch0[idx1]
    levels = ((1, pos0, batch0, idx1, cfg["radius"][0], 3, cfg["local_nn"][0]),
              (2, pos1, batch1, tp.fps_ragged(pos1, batch1, ratio=cfg["ratios"][1]), cfg["radius"][1], 64, cfg["local_nn"][1]))
    for level, pos, batch, idx, radius, C, local_nn in levels:
        for scale in (1.0, 2.0):
            pos_q, batch_q = pos[idx], batch[idx]
            es, col = tp.radius_edges(radius * scale, 64, pos, pos_q, batch, batch_q)
            E, M, Nq = col.numel(), pos.shape[0], pos_q.shape[0]
            g = torch.Generator().manual_seed(level)
            w = torch.randn(E, C, generator=g).to(dev).requires_grad_(True)
            x = (pos.clone() if C == 3 else torch.randn(M, C, generator=g).to(dev)).requires_grad_(C != 3)
            cot = torch.randn(Nq, C, generator=g).to(dev)

            def fused_fwd():
                with torch.no_grad():
                    return tp.rsconv_msgmax(w, x, es, col)

            def comp_fwd():
                with torch.no_grad():
                    return tp.segment_max(w * x[col], es)

            def fused_train():
                w.grad = x.grad = None
                (tp.rsconv_msgmax(w, x, es, col) * cot).sum().backward()
                return w.grad, x.grad

            def comp_train():
                w.grad = x.grad = None
                (tp.segment_max(w * x[col], es) * cot).sum().backward()
                return w.grad, x.grad

            same_out = bool(torch.equal(fused_fwd(), comp_fwd()))
            (gw_f, gx_f), (gw_c, gx_c) = [(a.clone(), None if b is None else b.clone()) for a, b in (fused_train(), comp_train())]
            same_dw = bool(torch.equal(gw_f, gw_c))
            dx_diff = None if gx_f is None else float((gx_f - gx_c).abs().max())
            ms, spread = alternate({"fused_fwd": fused_fwd, "composition_fwd": comp_fwd, "fused_fwd_bwd": fused_train,
                                    "composition_fwd_bwd": comp_train}, args.runs, args.inner)
            result["msgmax"].append({
                "level": level, "C": C, "radius": radius * scale, "queries": Nq, "support": M, "edges": E,
                "runs_at_cap": round(float(((es[1:] - es[:-1]) == 64).float().mean()), 3), "ms": ms, "spread_ms": spread,
                "out_bit_equal": same_out, "d_w_bit_equal": same_dw, "dx_max_abs_diff": dx_diff,
                "fused_over_composition_fwd": round(ms["fused_fwd"] / ms["composition_fwd"], 3),
                "fused_over_composition_fwd_bwd": round(ms["fused_fwd_bwd"] / ms["composition_fwd_bwd"], 3)})
            if scale == 1.0:  # where one Convolution forward spends its time
                torch.manual_seed(level)
                mlp = MLP(local_nn).to(dev).train()
                rows = tp.rsconv_relation_rows(pos, pos_q, es, col)
                with torch.no_grad():
                    wts = fused.rows_mlp(mlp, rows)

                def f_rows():
                    return tp.rsconv_relation_rows(pos, pos_q, es, col)

                def f_mlp():
                    with torch.no_grad():
                        return fused.rows_mlp(mlp, rows)

                def f_max():
                    with torch.no_grad():
                        return tp.rsconv_msgmax(wts, x, es, col)

                ms, spread = alternate({"relation_rows": f_rows, "local_nn_rows_mlp": f_mlp, "msgmax": f_max}, args.runs,
                                       args.inner)
                result["layer"].append({"level": level, "local_nn": local_nn, "edges": E, "forward_ms": ms,
                                        "spread_ms": spread,
                                        "local_nn_share": round(ms["local_nn_rows_mlp"] / sum(ms.values()), 3)})

    torch.manual_seed(0)
    net = RSConvMP("RSConv_2LD", 13).to(dev)
    labels = torch.randint(0, 13, (pos0.shape[0],), generator=gen).to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)

    def net_fwd():
        with torch.no_grad():
            return net(PDData(pos=pos0, batch=batch0, x=None))

    def net_step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.nll_loss(net(PDData(pos=pos0, batch=batch0, x=None)), labels).backward()
        opt.step()

    net.eval()
    ms_f, sp_f = alternate({"forward": net_fwd}, args.runs, max(args.inner // 10, 1), warmup=3)
    net.train()
    ms_t, sp_t = alternate({"train_step": net_step}, args.runs, max(args.inner // 10, 1), warmup=3)
    result["net"] = {"config": "RSConv_2LD", "classes": 13, "points": pos0.shape[0], "forward_ms": ms_f["forward"],
                     "forward_spread_ms": sp_f["forward"], "train_step_ms": ms_t["train_step"],
                     "train_step_spread_ms": sp_t["train_step"], "includes": "FPS, radius search (one host read per level), kNN"}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
