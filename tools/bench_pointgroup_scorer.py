"""PointGroup's sparse scorers: the cluster tensor build (torchpoints.cluster_voxelize, csrc/cluster_voxel.hip) against its
composition from existing ops, and the three scorers of torch_points3d_amd.pointgroup.PointGroup.

Scene: tools/bench_region_grow.py's (4 clouds of filled boxes on a lattice of step 0.02 over a floor of stuff points),
clustered by torchpoints.region_grow_csr; backbone features of 96 channels (random: the scorers' cost does not depend on
their values); cluster_voxel_size 0.05.  Two cluster sets: PointGroup's own parameters (a few hundred large clusters), and
the same points with a random label per voxel and min_cluster_size 1 (tens of thousands of clusters of a few points: the
many-cloud case of SparseTensor(clouds=K)).

  build      fused = cluster_voxelize; composition = gather_rows -> device GridSampling3D(mode="mean") for the forward, and
             gather_rows -> voxel_cluster -> index_add_ / count (autograd) for forward + backward, GridSampling3D's mean
             having no gradient
  scoring    PointGroup._compute_score with scorer_type "unet", "encoder" (pointgroup.yaml's widths, in_feat 96) and "MLP":
             forward (no_grad, eval) and training step (forward + backward of the scores' sum, train mode)

HIP events, median of --runs (30) calls after 3 warm-up calls.  Needs a GPU (no fallback).

    python tools/bench_pointgroup_scorer.py [--out profiles/pointgroup_scorer_bench.json]
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_region_grow import H, STUFF, scene  # noqa: E402
from bench_sparseconv import timed  # noqa: E402

SIZE, WIDTH = 0.05, 96


class _Features(torch.nn.Module):
    """stands where the backbone is: the scorers only read its width"""
    output_nc = WIDTH


def measure(tp, pg, grid_sampling, clusters, x, pos, coords, runs):
    dev = x.device
    members, owner = clusters.members, clusters.member_cluster
    out = {"clusters": len(clusters), "member_slots": int(members.numel())}

    def fused_fwd():
        with torch.no_grad():
            return tp.cluster_voxelize(clusters, x, pos, SIZE)[0].F

    def fused_step():
        xg = x.detach().requires_grad_(True)
        tp.cluster_voxelize(clusters, xg, pos, SIZE)[0].F.sum().backward()

    def composed_fwd():
        with torch.no_grad():
            data = types.SimpleNamespace(x=tp.gather_rows(x, members), pos=pos[members], batch=owner)
            return grid_sampling.GridSampling3D(SIZE, quantize_coords=True, mode="mean")(data).x

    def composed_step():
        xg = x.detach().requires_grad_(True)
        rows = tp.gather_rows(xg, members)
        cluster, last, _, start = grid_sampling.voxel_cluster(pos[members], owner, SIZE)
        V = last.numel()
        count = (start[1:] - start[:-1]).float()
        (torch.zeros((V, rows.shape[1]), device=dev).index_add_(0, cluster, rows) / count[:, None]).sum().backward()

    out["voxels"] = int(fused_fwd().shape[0])
    out["build_ms"] = {"fused_forward": timed(fused_fwd, runs), "composition_forward": timed(composed_fwd, runs),
                       "fused_forward_backward": timed(fused_step, runs),
                       "composition_forward_backward": timed(composed_step, runs)}
    out["scoring_ms"] = {}
    for kind in ("unet", "encoder", "MLP"):
        torch.manual_seed(0)
        cfg = pg.pointgroup_config("PointGroup", 3)  # (its scorers take 96 channels)
        net = pg.PointGroup(3, 5, backbone=_Features(), scorer_type=kind, scorer_unet=cfg["scorer_unet"],
                            scorer_encoder=cfg["scorer_encoder"]).to(dev)
        net.input = types.SimpleNamespace(pos=pos, coords=coords)

        def forward():
            with torch.no_grad():
                return net._compute_score(clusters, x, None)

        def step():
            xg = x.detach().requires_grad_(True)
            net._compute_score(clusters, xg, None).sum().backward()

        net.eval()
        fwd = timed(forward, runs)
        net.train()
        out["scoring_ms"][kind] = {"forward": fwd, "training_step": timed(step, runs)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointgroup_scorer needs a GPU: nothing is measured without one")
    from torch_points3d_amd import grid_sampling, pointgroup as pg, torchpoints as tp
    dev = torch.device("cuda:0")
    pos, labels, batch = [t.to(dev) for t in scene(args.clouds, args.points)]
    coords = torch.round(pos / H).int()
    ignore = torch.tensor([-1, STUFF], device=dev)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(pos.shape[0], WIDTH, generator=g).to(dev)
    radius = 1.5 * H
    large = tp.region_grow_csr(pos, labels, batch, ignore_labels=ignore, radius=radius, nsample=300, min_cluster_size=10)
    kept = ~torch.isin(labels, ignore)
    noisy = torch.where(kept, torch.randint(1, 9, labels.shape, generator=torch.Generator().manual_seed(1)).to(dev), labels)
    tiny = tp.region_grow_csr(pos, noisy, batch, ignore_labels=ignore, radius=radius, nsample=300, min_cluster_size=1)
    result = {"workload": "pointgroup_scorer", "clouds": args.clouds, "points": int(pos.shape[0]), "channels": WIDTH,
              "cluster_voxel_size": SIZE, "lattice_step": H, "timer": "hip events, median of %d" % args.runs,
              "pointgroup_clusters": measure(tp, pg, grid_sampling, large, x, pos, coords, args.runs),
              "many_small_clusters": measure(tp, pg, grid_sampling, tiny, x, pos, coords, args.runs)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
