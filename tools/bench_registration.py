"""Registration descriptors: what the HIP paths cost next to the reference's compositions kept on the device.

  feature_nn     torchpoints.feature_nn at (P, S, C) = (1024, 256, 32), (5192, 2048, 32), (5000, 5000, 32) against the
                 reference's literal broadcast `pdist(A, B).min(1)` (the (P, S, C) tensor; skipped above --broadcast-gib) and
                 against `torch.cdist(A, B).min(1)` (the |a|^2 + |b|^2 - 2ab expansion: a different arithmetic, timed as the
                 obvious alternative, not as an equal)
  hardest_neg    ContrastiveHardestNegativeLoss forward + backward on fragments of --rows rows with --pairs positive pairs,
                 at the YAML defaults (1024 positives, 256 mined rows) and the class defaults (5192, 2048), against the
                 reference's composition restated on the device (broadcast pdist, torch.isin, boolean-mask means; its
                 np.random.choice and .cpu().numpy() round trip are left out, so the baseline is flattered)
  fgr            torchpoints.fgr at N = 5000 (20 iterations) against the reference function on device tensors ((3N, 6)
                 matrix, torch.linalg.solve, one host read per iteration); both by wall clock around a synchronise
  train_step     one FragmentDescriptor.sparse forward + loss + backward on two fragments of about --voxels voxels

HIP events, 3 warm-up calls, the median of --runs (30) calls, except where stated.  Needs a GPU (no fallback).

    python tools/bench_registration.py [--out profiles/registration_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparseconv import timed  # noqa: E402


def unit(t):
    return t / t.norm(dim=1, keepdim=True)


def wall(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 4)


def reference_hardest_negative(F0, F1, pairs, sel0, sel1, pos_sel, pos_thresh, neg_thresh, num_pos):
    """metric_losses.py:69-113 with the selections given and every step on the device"""
    from torch_points3d_amd.registration import pdist
    hash_seed = max(len(F0), len(F1))
    sample = pairs[pos_sel] if len(pairs) > num_pos else pairs
    i0, i1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[i0], F1[i1]
    D01min, D01ind = pdist(posF0, F1[sel1]).min(1)
    D10min, D10ind = pdist(posF1, F0[sel0]).min(1)
    keys = pairs[:, 0] + pairs[:, 1] * hash_seed
    mask0 = ~torch.isin(i0 + sel1[D01ind] * hash_seed, keys)
    mask1 = ~torch.isin(sel0[D10ind] + i1 * hash_seed, keys)
    pos_loss = torch.relu((posF0 - posF1).pow(2).sum(1) - pos_thresh)
    neg0 = torch.relu(neg_thresh - D01min[mask0]).pow(2)
    neg1 = torch.relu(neg_thresh - D10min[mask1]).pow(2)
    return pos_loss.mean() + (neg0.mean() + neg1.mean()) / 2


def reference_fgr(xyz, xyz_target, mu_init=1.0, num_iter=20):
    """utils/registration.py:55-103 and geometry.get_trans on device tensors"""
    dev = xyz.device
    T_res = torch.eye(4, device=dev)
    mu = mu_init
    source = xyz.clone()
    weight = torch.ones(len(source), 1, device=dev)
    for i in range(num_iter):
        if i > 0 and i % 5 == 0:
            mu /= 2.0
        w = weight.view(-1)
        A = torch.zeros(3, len(source), 6, device=dev)
        A[0, :, 1], A[0, :, 2], A[0, :, 3] = w * source[:, 2], -w * source[:, 1], w
        A[1, :, 0], A[1, :, 2], A[1, :, 4] = -w * source[:, 2], w * source[:, 0], w
        A[2, :, 0], A[2, :, 1], A[2, :, 5] = w * source[:, 1], -w * source[:, 0], w
        A = A.reshape(-1, 6)
        b = torch.cat([w * (xyz_target[:, k] - source[:, k]) for k in range(3)], 0).view(-1, 1)
        x = torch.linalg.solve(A.T.mm(A), A.T @ b).view(-1)
        T = torch.eye(4, device=dev)
        T[:3, 3] = x[3:]
        axis = x[:3]
        theta = torch.norm(axis)
        if theta > 0:  # (the reference's host read)
            axis = axis / theta
        K = torch.zeros(3, 3, device=dev)
        K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
        T[:3, :3] = torch.eye(3, device=dev) + torch.sin(theta) * K + (1 - torch.cos(theta)) * K.mm(K)
        source = source.mm(T[:3, :3].T) + T[:3, 3]
        T_res = T @ T_res
        weight = (mu / (mu + torch.norm(xyz_target - source, dim=1) ** 2)).view(-1, 1)
    return T_res


def fragment(rng, voxels, n_feat, dev):
    """`voxels` distinct cells of a shell of radius about 40 cells"""
    d = rng.randn(4 * voxels, 3)
    cells = np.unique(np.round(d / np.linalg.norm(d, axis=1, keepdims=True) * (36 + 8 * rng.rand(len(d), 1))).astype(np.int64), axis=0)
    cells = cells[rng.permutation(len(cells))[:voxels]] + 64
    return types.SimpleNamespace(x=torch.from_numpy(rng.randn(len(cells), n_feat).astype(np.float32)).to(dev),
                                 coords=torch.from_numpy(cells).int().to(dev),
                                 batch=torch.zeros(len(cells), dtype=torch.long, device=dev),
                                 pos=torch.from_numpy(cells.astype(np.float32) * 0.02).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--pairs", type=int, default=8000)
    ap.add_argument("--voxels", type=int, default=20000)
    ap.add_argument("--broadcast-gib", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_registration needs a GPU: nothing is measured without one")
    from torch_points3d_amd import registration as reg
    from torch_points3d_amd import torchpoints as tp
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {"workload": "registration", "timer": "hip events, 3 warm-up calls, median of %d (fgr: wall clock + synchronise)" % args.runs,
              "feature_nn": [], "hardest_negative": [], "not_timed": []}

    for P, S, C in ((1024, 256, 32), (5192, 2048, 32), (5000, 5000, 32)):
        a, b = unit(torch.randn(P, C)).to(dev), unit(torch.randn(S, C)).to(dev)
        row = {"P": P, "S": S, "C": C, "feature_nn_ms": timed(lambda: tp.feature_nn(a, b), args.runs),
               "cdist_min_ms": timed(lambda: torch.cdist(a, b).min(1), args.runs)}
        gib = P * S * C * 4 / 2 ** 30
        if gib <= args.broadcast_gib:
            row["broadcast_pdist_min_ms"] = timed(lambda: reg.pdist(a, b).min(1), args.runs)
            ref = reg.pdist(a, b, "SquareL2").min(1)
            got = tp.feature_nn(a, b)
            row["same_argmin_as_broadcast"] = bool(torch.equal(got[1], ref[1]))
            row["dist2_max_abs_diff"] = float((got[0] - ref[0]).abs().max())
        else:
            result["not_timed"].append("broadcast pdist at (%d, %d, %d): %.1f GiB" % (P, S, C, gib))
        row["broadcast_tensor_gib"] = round(gib, 3)
        result["feature_nn"].append(row)

    F0, F1 = unit(torch.randn(args.rows, 32)).to(dev), unit(torch.randn(args.rows, 32)).to(dev)
    pairs = torch.stack([torch.randperm(args.rows)[: args.pairs], torch.randperm(args.rows)[: args.pairs]], 1).to(dev)
    F1[pairs[:, 1]] = unit(F0[pairs[:, 0]] + 0.06 * torch.randn(args.pairs, 32, device=dev))
    for num_pos, num_hn in ((1024, 256), (5192, 2048)):
        sel0 = torch.randperm(args.rows, device=dev)[:num_hn]
        sel1 = torch.randperm(args.rows, device=dev)[:num_hn]
        pos_sel = torch.randperm(args.pairs, device=dev)[:num_pos]
        loss_fn = reg.ContrastiveHardestNegativeLoss(0.1, 1.4, num_pos, num_hn)

        def hip_step():
            x, y = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
            loss = loss_fn(x, y, pairs, sel0=sel0, sel1=sel1, pos_sel=pos_sel)
            loss.backward()
            return loss.detach(), x.grad

        def ref_step():
            x, y = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
            loss = reference_hardest_negative(x, y, pairs, sel0, sel1, pos_sel, 0.1, 1.4, num_pos)
            loss.backward()
            return loss.detach(), x.grad

        (l_hip, g_hip), (l_ref, g_ref) = hip_step(), ref_step()
        result["hardest_negative"].append({
            "rows": args.rows, "pairs": args.pairs, "num_pos": num_pos, "num_hn_samples": num_hn,
            "fwd_bwd_ms": timed(hip_step, args.runs), "reference_composition_fwd_bwd_ms": timed(ref_step, args.runs),
            "loss": float(l_hip), "reference_loss": float(l_ref), "grad_max_abs_diff": float((g_hip - g_ref).abs().max())})

    n = 5000
    T = torch.eye(4)
    T[:3, :3] = torch.linalg.matrix_exp(torch.tensor([[0.0, -0.3, 0.2], [0.3, 0.0, -0.4], [-0.2, 0.4, 0.0]]))
    T[:3, 3] = torch.tensor([0.2, -0.1, 0.3])
    xyz = torch.rand(n, 3) * 2 - 1
    tgt = xyz @ T[:3, :3].T + T[:3, 3] + 0.003 * torch.randn(n, 3)
    tgt[: (3 * n) // 10] = torch.rand((3 * n) // 10, 3) * 3 - 1.5
    xyz, tgt = xyz.to(dev), tgt.to(dev)
    T_hip, T_ref = tp.fgr(xyz, tgt), reference_fgr(xyz, tgt)
    result["fgr"] = {"N": n, "iterations": 20, "outliers": (3 * n) // 10, "timer": "wall clock + synchronise, median of %d" % args.runs,
                     "fgr_ms": wall(lambda: tp.fgr(xyz, tgt), args.runs), "reference_on_device_ms": wall(lambda: reference_fgr(xyz, tgt), args.runs),
                     "pose_max_abs_diff": float((T_hip - T_ref).abs().max()),
                     "translation_error": float((T_hip[:3, 3].cpu() - T[:3, 3]).norm())}

    rng = np.random.RandomState(0)
    data, target = fragment(rng, args.voxels, 1, dev), fragment(rng, args.voxels, 1, dev)
    m = min(len(data.x), len(target.x), 5000)
    match = torch.stack([torch.randperm(len(data.x))[:m], torch.randperm(len(target.x))[:m]], 1).to(dev)
    net = reg.FragmentDescriptor.sparse(1, metric_loss=reg.ContrastiveHardestNegativeLoss(0.1, 1.4, 1024, 256)).to(dev).train()

    def train_step():
        net.zero_grad(set_to_none=True)
        net(data, target, match)
        net.loss.backward()

    result["train_step"] = {"model": "FragmentDescriptor.sparse(1): SparseConv3dUnet('unet_4', in_feat 32), head [96, 96] -> 32",
                            "voxels": [len(data.x), len(target.x)], "matches": m, "num_pos": 1024, "num_hn_samples": 256,
                            "fwd_loss_bwd_ms": timed(train_step, min(args.runs, 10))}
    result["not_timed"] += ["BatchHardContrastiveLoss", "FragmentDescriptor.kpconv", "get_matches with sym=True", "evaluate_pair"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
