"""Generator of tests/golden/registration.npz: the REFERENCE's own registration code on the CPU.

  core/losses/metric_losses.py      loaded by file path (it imports torch and numpy only): ContrastiveHardestNegativeLoss,
                                    BatchHardContrastiveLoss, pdist
  utils/geometry.py                 loaded by file path as torch_points3d.utils.geometry (get_trans, rodrigues)
  utils/registration.py             loaded by file path with stand-ins in sys.modules for `open3d` (never called) and
                                    `torch_geometric.nn.knn` (a float64 brute force: for every row of y the k nearest rows of
                                    x, returned as (2, M) = [row of y, row of x], what torch_geometric documents)
  metrics/registration_metrics.py   loaded by file path with a stand-in for `sklearn.neighbors` (never called)
  metrics/registration_tracker.py   cannot be imported (torchnet, the trackers' base classes); lines 123-145, the sequence
                                    for one fragment pair, are restated here over the reference's own functions

The case: two fragments of 300 and 280 rows with unit-norm features of 32 channels, 150 positive pairs whose target rows
are a perturbed copy of the source rows (so the true nearest row is often the positive partner and the `isin` mask takes
both values on both sides), the selections the reference drew with np.random.choice under a fixed np.random.seed, both
losses' values and input gradients, get_matches (sym false and true), Kabsch and FGR on 200 correspondences of which 30 %
are outliers, the four metrics and the per-pair evaluation -- everything also in float64 (torch's default dtype switched:
the reference allocates its matrices in the default dtype).

Safety conditions (asserted here and again in tests/test_registration_cpu.py, re-seeded until they hold): every relu
argument of the losses is at least RELU_MARGIN from 0, every mined row's gap between the nearest and the second nearest
d^2 is at least GAP_MARGIN, and every distance the hit ratios threshold is at least 1e-4 from tau_1.

    python tests/golden/make_golden_registration.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import registration_ref as rr  # noqa: E402

RELU_MARGIN = 5e-5
GAP_MARGIN = 1e-4
CONFIG = dict(n0=300, n1=280, channels=32, pairs=150, num_pos=128, num_hn_samples=256, pos_thresh=0.1, neg_thresh=1.4,
              bh_pos_thresh=0.01, bh_neg_thresh=1.4, bh_min_dist=0.15, fgr_points=200, fgr_outliers=60, tau_1=0.1, tau_2=0.05,
              num_points=256, np_seed=1234)


class Unsafe(Exception):
    pass


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def knn(x, y, k, batch_x=None, batch_y=None):
    """torch_geometric.nn.knn for one cloud: (2, len(y) * k) = [row of y, row of x], brute force in float64"""
    d = torch.cdist(y.double(), x.double())
    col = torch.topk(d, k, dim=1, largest=False)[1]
    row = torch.arange(len(y)).view(-1, 1).expand(-1, k)
    return torch.stack([row.reshape(-1), col.reshape(-1)], 0)


def load_reference():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    base = os.path.join(mg.REF, "torch_points3d")
    mod("open3d")
    mod("torch_geometric")
    mod("torch_geometric.nn", knn=knn)
    mod("sklearn")
    mod("sklearn.neighbors", NearestNeighbors=None)
    mod("torch_points3d")
    mod("torch_points3d.utils")
    losses = _load("tp3d_ref_metric_losses", os.path.join(base, "core", "losses", "metric_losses.py"))
    _load("torch_points3d.utils.geometry", os.path.join(base, "utils", "geometry.py"))
    reg = _load("torch_points3d.utils.registration", os.path.join(base, "utils", "registration.py"))
    metrics = _load("tp3d_ref_registration_metrics", os.path.join(base, "metrics", "registration_metrics.py"))
    return losses, reg, metrics


def unit(t):
    return t / t.norm(dim=1, keepdim=True)


def lattice(n, g):
    """n distinct nodes of a 7 x 7 x 7 lattice of pitch 0.1: every pairwise distance is 0.1 sqrt(k), nowhere near 0.15"""
    nodes = torch.tensor([[a, b, c] for a in range(7) for b in range(7) for c in range(7)], dtype=torch.float32) * 0.1
    return nodes[torch.randperm(len(nodes), generator=g)[:n]].contiguous()


def evaluate_pair(reg, metrics, feat, feat_target, xyz, xyz_target, matches_gt, rand, rand_target):
    """registration_tracker.py:123-145 over the reference's functions"""
    T_gt = reg.estimate_transfo(xyz[matches_gt[:, 0]], xyz_target[matches_gt[:, 1]])
    matches_pred = reg.get_matches(feat[rand], feat_target[rand_target])
    src, tgt = xyz[rand][matches_pred[:, 0]], xyz_target[rand_target][matches_pred[:, 1]]
    T_pred = reg.fast_global_registration(src, tgt)
    hit_ratio = metrics.compute_hit_ratio(src, tgt, T_gt, CONFIG["tau_1"])
    trans_error, rot_error = metrics.compute_transfo_error(T_pred, T_gt)
    sr_err = metrics.compute_scaled_registration_error(xyz, T_gt, T_pred)
    dist = torch.norm(src.mm(T_gt[:3, :3].T) + T_gt[:3, 3] - tgt, dim=1)
    if float((dist - CONFIG["tau_1"]).abs().min()) < 1e-4:
        raise Unsafe("a matched distance within 1e-4 of tau_1")
    return {"hit_ratio": hit_ratio, "feat_match_ratio": (hit_ratio > CONFIG["tau_2"]).to(xyz.dtype), "trans_error": trans_error,
            "rot_error": rot_error, "sr_err": sr_err, "T_gt": T_gt, "T_pred": T_pred}


def inputs(seed):
    c = CONFIG
    g = torch.Generator().manual_seed(seed)
    F0 = unit(torch.randn(c["n0"], c["channels"], generator=g))
    F1 = unit(torch.randn(c["n1"], c["channels"], generator=g))
    m0 = torch.randperm(c["n0"], generator=g)[: c["pairs"]]
    m1 = torch.randperm(c["n1"], generator=g)[: c["pairs"]]
    F1[m1] = unit(F0[m0] + 0.35 * torch.randn(c["pairs"], c["channels"], generator=g) / c["channels"] ** 0.5)
    matches = torch.stack([m0, m1], 1)
    T_true = torch.eye(4, dtype=torch.float64)
    T_true[:3, :3] = rr.rotation([0.3, -0.5, 0.8], 0.6)
    T_true[:3, 3] = torch.tensor([0.25, -0.1, 0.4], dtype=torch.float64)
    T_true = T_true.float()
    xyz0 = lattice(c["n0"], g)
    xyz1 = torch.rand(c["n1"], 3, generator=g) * 1.5 - 0.4
    xyz1[m1] = xyz0[m0] @ T_true[:3, :3].T + T_true[:3, 3] + 0.004 * torch.randn(c["pairs"], 3, generator=g)
    n = c["fgr_points"]
    fgr_xyz = torch.rand(n, 3, generator=g) * 2 - 1
    fgr_clean = fgr_xyz @ T_true[:3, :3].T + T_true[:3, 3]
    fgr_target = fgr_clean + 0.005 * torch.randn(n, 3, generator=g)
    out = torch.randperm(n, generator=g)[: c["fgr_outliers"]]
    fgr_target[out] = torch.rand(len(out), 3, generator=g) * 3 - 1.5
    rand = torch.randperm(c["n0"], generator=g)[: c["num_points"]]
    rand_target = torch.randperm(c["n1"], generator=g)[: c["num_points"]]
    return dict(F0=F0, F1=F1, matches=matches, xyz0=xyz0, xyz1=xyz1, T_true=T_true, fgr_xyz=fgr_xyz, fgr_target=fgr_target,
                fgr_clean=fgr_clean, rand=rand, rand_target=rand_target)


def replay_selections(n0, n1, n_pairs):
    """the draws of ContrastiveHardestNegativeLoss.contrastive_hardest_negative_loss, in its order, from the same seed"""
    c = CONFIG
    np.random.seed(c["np_seed"])
    sel0 = np.random.choice(n0, min(n0, c["num_hn_samples"]), replace=False)
    sel1 = np.random.choice(n1, min(n1, c["num_hn_samples"]), replace=False)
    pos_sel = np.random.choice(n_pairs, c["num_pos"], replace=False) if n_pairs > c["num_pos"] else np.arange(n_pairs)
    return torch.from_numpy(sel0).long(), torch.from_numpy(sel1).long(), torch.from_numpy(pos_sel).long()


def run(losses, reg, metrics, inp, dtype):
    """everything the fixture holds for one dtype, from the reference's code"""
    c = CONFIG
    torch.set_default_dtype(dtype)
    try:
        cast = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
        rec = {}
        F0, F1 = cast["F0"].clone().requires_grad_(True), cast["F1"].clone().requires_grad_(True)
        hn = losses.ContrastiveHardestNegativeLoss(c["pos_thresh"], c["neg_thresh"], c["num_pos"], c["num_hn_samples"])
        np.random.seed(c["np_seed"])
        loss = hn(F0, F1, cast["matches"])
        loss.backward()
        rec["hn/loss"], rec["hn/dF0"], rec["hn/dF1"] = loss.detach(), F0.grad.clone(), F1.grad.clone()
        F0, F1 = cast["F0"].clone().requires_grad_(True), cast["F1"].clone().requires_grad_(True)
        bh = losses.BatchHardContrastiveLoss(c["bh_pos_thresh"], c["bh_neg_thresh"], c["bh_min_dist"])
        loss = bh(F0, F1, cast["matches"], cast["xyz0"], cast["xyz1"])
        loss.backward()
        rec["bh/loss"], rec["bh/dF0"], rec["bh/dF1"] = loss.detach(), F0.grad.clone(), F1.grad.clone()
        with torch.no_grad():
            rec["matches/plain"] = reg.get_matches(cast["F0"], cast["F1"])
            rec["matches/sym"] = reg.get_matches(cast["F0"], cast["F1"], sym=True)
            T_kabsch = reg.estimate_transfo(cast["fgr_xyz"], cast["fgr_target"])
            T_fgr = reg.fast_global_registration(cast["fgr_xyz"], cast["fgr_target"])
            rec["kabsch/T"], rec["fgr/T"] = T_kabsch, T_fgr
            T_true = cast["T_true"]
            rec["metrics/hit_ratio"] = metrics.compute_hit_ratio(cast["fgr_xyz"], cast["fgr_target"], T_true, c["tau_1"])
            dist = torch.norm(cast["fgr_xyz"].mm(T_true[:3, :3].T) + T_true[:3, 3] - cast["fgr_target"], dim=1)
            if float((dist - c["tau_1"]).abs().min()) < 1e-4:
                raise Unsafe("a correspondence within 1e-4 of tau_1")
            rte, rre = metrics.compute_transfo_error(T_true, T_fgr)
            rec["metrics/rte"], rec["metrics/rre"] = rte, rre
            rec["metrics/sr_err"] = metrics.compute_scaled_registration_error(cast["fgr_xyz"], T_true, T_fgr)
            rec["metrics/recall_fgr"] = np.array(metrics.compute_registration_recall(cast["fgr_xyz"], cast["fgr_clean"], T_fgr))
            rec["metrics/recall_kabsch"] = np.array(
                metrics.compute_registration_recall(cast["fgr_xyz"], cast["fgr_clean"], T_kabsch, thresh=0.02))
            pair = evaluate_pair(reg, metrics, cast["F0"], cast["F1"], cast["xyz0"], cast["xyz1"], cast["matches"], cast["rand"],
                                 cast["rand_target"])
            for k, v in pair.items():
                rec["pair/" + k] = v
        return rec
    finally:
        torch.set_default_dtype(torch.float32)


def check_safety(inp, sel0, sel1, pos_sel):
    """the conditions of the module docstring on the float64 restatement; returns the least margins"""
    c = CONFIG
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    hn = rr.hardest_negative_parts(d["F0"], d["F1"], d["matches"], sel0, sel1, pos_sel, c["pos_thresh"], c["neg_thresh"],
                                   c["num_pos"])
    bh = rr.batch_hard_parts(d["F0"], d["F1"], d["matches"], d["xyz0"], c["bh_pos_thresh"], c["bh_neg_thresh"], c["bh_min_dist"])
    relu_min = min(float(hn["relu_args"].abs().min()), float(bh["relu_args"].abs().min()))
    gap_min = min(float(hn["gap01"].min()), float(hn["gap10"].min()), float(bh["gap"].min()))
    both = all(0 < int(m.sum()) < m.numel() for m in (hn["mask0"], hn["mask1"]))
    if relu_min < RELU_MARGIN:
        raise Unsafe("a relu argument %.3g from 0" % relu_min)
    if gap_min < GAP_MARGIN:
        raise Unsafe("a mined row's gap is %.3g" % gap_min)
    if not both:
        raise Unsafe("the isin mask does not take both values on both sides")
    return relu_min, gap_min


def main():
    losses, reg, metrics = load_reference()
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    while True:
        try:
            inp = inputs(seed)
            sel0, sel1, pos_sel = replay_selections(CONFIG["n0"], CONFIG["n1"], CONFIG["pairs"])
            relu_min, gap_min = check_safety(inp, sel0, sel1, pos_sel)
            rec32 = run(losses, reg, metrics, inp, torch.float32)
            rec64 = run(losses, reg, metrics, inp, torch.float64)
            break
        except Unsafe as e:
            print("seed %d: %s" % (seed, e), flush=True)
            seed += 1
    rec = dict(inp)
    rec.update(sel0=sel0, sel1=sel1, pos_sel=pos_sel, seed=np.array([seed]), relu_min=np.array([relu_min]),
               gap_min=np.array([gap_min]))
    for k, v in CONFIG.items():
        rec["config/" + k] = np.array([v])
    rec.update(rec32)
    for k, v in rec64.items():
        rec["f64/" + k] = v.detach().numpy() if torch.is_tensor(v) else v
    path = os.path.join(HERE, "registration.npz")
    np.savez_compressed(path, **mg.to_np(rec))
    assert os.path.getsize(path) < 1 << 20
    print("wrote registration.npz (seed %d, %d arrays, %d bytes, least |relu argument| %.3g, least gap %.3g)"
          % (seed, len(rec), os.path.getsize(path), relu_min, gap_min))


if __name__ == "__main__":
    main()
