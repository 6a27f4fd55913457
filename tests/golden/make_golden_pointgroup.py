"""Generator of tests/golden/pointgroup_scorer_{unet,encoder}.npz, their `_grads` companions (the parameter gradients, in
files of their own to stay under the size limit of a committed file) and pointgroup_config.json: the
scoring path of the REFERENCE's PointGroup on the CPU, from the reference's own classes.

Driven as they are (loaded from the reference tree, with stand-ins for the third-party packages in sys.modules -- they live
here, never in the fixture):
  core/data_transform/grid_transform.py   GridSampling3D(0.05, quantize_coords=True, mode="mean") and group_data, over the
                                          voxel-function stand-ins of make_golden_ms_svconv.py (voxel_grid,
                                          consecutive_cluster of oracle/voxel_ref.py; scatter_mean in torch, differentiable)
  modules/SparseConv3d/modules.py         ResNetDown / ResNetUp over the dense stand-ins of make_golden_sparseconv.py
  core/base_conv/message_passing.py       GlobalBaseModule(aggr="max") with a torch global_max_pool
  core/common_modules                     MLP, Seq, FastBatchNorm1d

Restated here, because models/panoptic/pointgroup.py cannot be loaded (the Minkowski application, BaseModel,
torch_points_kernels.region_grow): the glue of PointGroup._compute_score, lines 123-159 (`compute_score` below, statement
for statement), the forwards of the Minkowski U-Net / encoder (applications/minkowski.py:129-190, the same as
applications/sparseconv3d.py:143-210) and the ScorerHead of pointgroup.py:46.

Case: 12 clusters of 20 to 60 points (the last two share points with the first two, as a cluster grown on the votes shares
points with one grown on the positions), points on a jittered lattice finer than the voxel so that voxels hold one to
several points, in_feat 8, one block per stage, train mode.  Stored per scorer: state_dict, inputs (shared), cluster
lists, the voxel rows, cluster scores, running statistics after the pass, the gradient wrt the backbone features and
every parameter for a stored cotangent, and the same pass in float64 (`f64/`).  Safety conditions (asserted here, the
weights re-seeded until they hold, and again in tests/test_pointgroup_scorer_cpu.py): README_pointgroup.md.

    python tests/golden/make_golden_pointgroup.py
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_ms_svconv as mgm  # noqa: E402
import make_golden_sparseconv as mgs  # noqa: E402

KINK_MARGIN = mgs.KINK_MARGIN  # 5e-5
HALF_MARGIN = 1e-3
MAX_MARGIN = 1e-6
COARSE_ROWS = 8
SIZE = 0.05
IN_FEAT = 8
SIZES = [20, 60, 33, 41, 27, 52, 38, 24, 45, 30, 36, 29]  # points per cluster; the last two take half from clusters 0 and 1
_leaky_inputs = []


def scorer_config(kind, f=IN_FEAT, n=1):
    cfg = dict(down_conv=dict(module_name="ResNetDown", dimension=3, down_conv_nn=[[f, 2 * f], [2 * f, 4 * f]], kernel_size=3,
                              stride=2, N=n))
    if kind == "unet":
        cfg["up_conv"] = dict(module_name="ResNetUp", dimension=3, up_conv_nn=[[4 * f, 2 * f], [4 * f, f]], kernel_size=3, stride=2,
                              N=n)
    else:
        cfg["innermost"] = dict(module_name="GlobalBaseModule", activation=dict(name="LeakyReLU", negative_slope=0.2), aggr="max",
                                nn=[4 * f, f])
    return cfg


class Data(object):
    """the slice of torch_geometric.data.Data / Batch that grid_transform.py and message_passing.py touch"""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __getattr__(self, k):  # an absent attribute reads as None (torch_geometric's behaviour)
        if k.startswith("__"):
            raise AttributeError(k)
        return None

    @property
    def keys(self):
        return [k for k, v in self.__dict__.items() if v is not None]

    @property
    def num_nodes(self):
        return self.pos.shape[0]

    def __iter__(self):
        for k in list(self.keys):
            yield k, getattr(self, k)

    def __contains__(self, k):
        return k in self.keys

    def __getitem__(self, k):
        return getattr(self, k)

    def __setitem__(self, k, v):
        setattr(self, k, v)

    def to(self, *a, **k):
        return self


def global_max_pool(x, batch):
    K = int(batch.max()) + 1
    out = torch.full((K, x.shape[1]), float("-inf"), dtype=x.dtype)
    return out.scatter_reduce(0, batch.unsqueeze(1).expand_as(x), x, "amax")


def scatter(src, index, dim=0, reduce="max"):
    assert reduce == "max" and dim == 0
    return global_max_pool(src, index)


def load_reference():
    modules = mgs.load_reference()
    tg_nn, tg_data = sys.modules["torch_geometric.nn"], sys.modules["torch_geometric.data"]
    tg_nn.voxel_grid, tg_nn.global_max_pool = mgm.voxel_grid, global_max_pool
    sys.modules["torch_geometric.nn.pool.consecutive"].consecutive_cluster = mgm.consecutive_cluster
    sys.modules["torch_scatter"].scatter_mean = mgm.scatter_mean
    tg_data.Data = tg_data.Batch = Data
    mg._stub("torch_cluster", grid_cluster=None)
    spec = importlib.util.spec_from_file_location(
        "ref_grid_transform_pg", os.path.join(mg.REF, "torch_points3d/core/data_transform/grid_transform.py"))
    gt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gt)
    import torch_points3d.core.base_conv.message_passing as mp
    mp.global_max_pool, mp.Batch = global_max_pool, Data  # (when an earlier import bound the empty stand-ins)
    from torch_points3d.core.common_modules import MLP, Seq
    return modules, gt, mp, MLP, Seq


def make_scorer(kind, modules, mp, Seq):
    cfg = scorer_config(kind)

    def opts(o, i):
        # (kernel_size, stride and N are scalars in the YAML: they hold for every stage)
        return {k: (v[i] if k.endswith("conv_nn") else v) for k, v in o.items() if k != "module_name"}

    class Unet(torch.nn.Module):  # applications/minkowski.py MinkowskiUnet.forward
        def __init__(self):
            super().__init__()
            d, u = cfg["down_conv"], cfg["up_conv"]
            self.down_modules = torch.nn.ModuleList(modules.ResNetDown(**opts(d, i)) for i in range(2))
            self.up_modules = torch.nn.ModuleList(modules.ResNetUp(**opts(u, i)) for i in range(2))

        def forward(self, data):
            x = mgs._Tensor(data.x, torch.cat([data.coords.int(), data.batch.int().unsqueeze(1)], 1))
            stack_down = []
            for i in range(len(self.down_modules) - 1):
                x = self.down_modules[i](x)
                stack_down.append(x)
            x = self.down_modules[-1](x)
            stack_down.append(None)
            for i in range(len(self.up_modules)):
                x = self.up_modules[i](x, stack_down.pop())
            return Data(x=x.F, batch=data.batch)

    class Encoder(torch.nn.Module):  # applications/minkowski.py MinkowskiEncoder.forward
        def __init__(self):
            super().__init__()
            d, inner = cfg["down_conv"], cfg["innermost"]
            self.down_modules = torch.nn.ModuleList(modules.ResNetDown(**opts(d, i)) for i in range(2))
            self.inner_modules = torch.nn.ModuleList([mp.GlobalBaseModule(nn=inner["nn"], aggr=inner["aggr"])])
            self.coarsest = []

        def forward(self, data):
            x = mgs._Tensor(data.x, torch.cat([data.coords.int(), data.batch.int().unsqueeze(1)], 1))
            for m in self.down_modules:
                x = m(x)
            self.coarsest.append(x.C)
            return self.inner_modules[0](Data(x=x.F, batch=x.C[:, 3].long()))

    class Scorer(torch.nn.Module):  # the attributes of pointgroup.py:41-46 that the scoring path uses
        def __init__(self):
            super().__init__()
            if kind == "unet":
                self.ScorerUnet = Unet()
            else:
                self.ScorerEncoder = Encoder()
            self.ScorerHead = Seq().append(torch.nn.Linear(IN_FEAT, 1)).append(torch.nn.Sigmoid())

    return Scorer


def compute_score(model, kind, voxelizer, all_clusters, backbone_features, data, keep):
    """PointGroup._compute_score (pointgroup.py:123-159), the branches of `kind`"""
    x, coords, batch, pos = [], [], [], []
    for i, cluster in enumerate(all_clusters):
        x.append(backbone_features[cluster])
        coords.append(data.coords[cluster])
        batch.append(i * torch.ones(cluster.shape[0]))
        pos.append(data.pos[cluster])
    batch_cluster = Data(x=torch.cat(x), coords=torch.cat(coords), batch=torch.cat(batch))
    batch_cluster.pos = torch.cat(pos)
    batch_cluster = voxelizer(batch_cluster)
    keep["voxel_coords"], keep["voxel_batch"], keep["voxel_x"] = batch_cluster.coords, batch_cluster.batch.long(), batch_cluster.x
    if kind == "encoder":
        score_backbone_out = model.ScorerEncoder(batch_cluster)
        cluster_feats = score_backbone_out.x
    else:
        score_backbone_out = model.ScorerUnet(batch_cluster)
        keep["rows"], keep["rows_batch"] = score_backbone_out.x, batch_cluster.batch.long()
        cluster_feats = scatter(score_backbone_out.x, batch_cluster.batch.long(), dim=0, reduce="max")
    return model.ScorerHead(cluster_feats).squeeze(-1)


def inputs():
    """points of 12 blobs on a jittered lattice of step 0.03 (voxels of 0.05 hold one to several of them), every pos / SIZE
    at least 2 * HALF_MARGIN from a half-integer"""
    g = torch.Generator().manual_seed(41)
    pos, clusters = [], []
    for c, n in enumerate(SIZES):
        own = n if c < 10 else n // 2
        origin = torch.tensor([0.45 * (c % 4), 0.5 * (c // 4), 0.2 * (c % 3)]) + 0.1
        cells = torch.randperm(6 * 6 * 4, generator=g)
        members, k = [], 0
        while len(members) < own:
            cell = int(cells[k])
            k += 1
            p = origin + 0.03 * torch.tensor([cell % 6, (cell // 6) % 6, cell // 36]) + 0.004 * torch.randn(3, generator=g)
            q = p.double() / SIZE
            if float((q - torch.floor(q) - 0.5).abs().min()) < 2 * HALF_MARGIN:
                continue
            members.append(len(pos))
            pos.append(p)
        if c >= 10:  # the other half: points of cluster c - 10
            members += clusters[c - 10][:n - own]
        clusters.append(members)
    pos = torch.stack(pos).float().contiguous()
    N = len(pos)
    assert [len(c) for c in clusters] == SIZES
    x = torch.randn(N, IN_FEAT, generator=g)
    clusters = [torch.tensor(sorted(c), dtype=torch.int64) for c in clusters]
    return dict(pos=pos, x=x, coords=torch.round(pos / 0.02).int(), cot=torch.randn(len(SIZES), generator=g),
                members=torch.cat(clusters), starts=torch.tensor([0] + list(np.cumsum(SIZES))))


def _hook_leaky(module):
    seen = set()
    for m in module.modules():
        if isinstance(m, torch.nn.LeakyReLU) and id(m) not in seen:
            seen.add(id(m))
            m.register_forward_pre_hook(lambda mod, a: _leaky_inputs.append(float(a[0].detach().abs().min())))


def run(kind, Scorer, gt, inp, dtype, state):
    torch.set_default_dtype(dtype)
    try:
        m = Scorer().train()
        m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()})
        _hook_leaky(m)
        del mgs._relu_inputs[:], _leaky_inputs[:]
        rows = []
        if kind == "encoder":  # the rows in front of the innermost maximum
            m.ScorerEncoder.inner_modules[0].nn.register_forward_hook(lambda mod, a, out: rows.append(out.detach()))
        x = inp["x"].to(dtype).clone().requires_grad_(True)
        data = Data(pos=inp["pos"].to(dtype), coords=inp["coords"])
        s = inp["starts"].tolist()
        clusters = [inp["members"][s[c]:s[c + 1]] for c in range(len(s) - 1)]
        keep = {}
        scores = compute_score(m, kind, gt.GridSampling3D(SIZE, quantize_coords=True, mode="mean"), clusters, x, data, keep)
        (scores * inp["cot"].to(dtype)).sum().backward()
        if kind == "encoder":
            keep["rows"], keep["rows_batch"] = rows[0], m.ScorerEncoder.coarsest[0][:, 3].long()
        rec = dict(scores=scores.detach(), grad_x=x.grad, voxel_coords=keep["voxel_coords"], voxel_batch=keep["voxel_batch"],
                   voxel_x=keep["voxel_x"].detach())
        # the least margin by which a per-cluster maximum wins (clusters of one row have no runner-up)
        win = float("inf")
        for c in range(len(clusters)):
            r = keep["rows"].detach()[keep["rows_batch"] == c]
            if len(r) > 1:
                top = torch.topk(r, 2, dim=0).values
                win = min(win, float((top[0] - top[1]).min()))
        kink = min(mgs._relu_inputs + _leaky_inputs)
        coarse = len(mgm.msr.sr.down_coords(torch.cat([keep["voxel_coords"], keep["voxel_batch"].int().unsqueeze(1)], 1), 4))
        return rec, m, dict(kink=kink, win=win, coarse=coarse)
    finally:
        torch.set_default_dtype(torch.float32)


def resolved_pointgroup_yaml(feat):
    """conf/models/panoptic/pointgroup.yaml with its constants and interpolations filled in (FEAT = `feat`)"""
    import yaml
    doc = yaml.safe_load(open(os.path.join(mg.REF, "conf", "models", "panoptic", "pointgroup.yaml")))

    def res(v, consts):
        if isinstance(v, list):
            return [res(u, consts) for u in v]
        if isinstance(v, dict):
            inner = dict(consts)
            for k, u in v.get("define_constants", {}).items():
                inner[k] = res(u, consts)
            return {k: res(u, inner) for k, u in v.items() if k != "define_constants"}
        if isinstance(v, str):
            if v.startswith("${models.") and v.endswith(".feat_size}"):
                return doc[v[len("${models."):-len(".feat_size}")]]["feat_size"]
            try:
                return eval(v, {"__builtins__": {}}, dict(consts, FEAT=feat))
            except Exception:
                return v
        return v

    return {name: res(entry, {}) for name, entry in doc.items()}


def main():
    modules, gt, mp, MLP, Seq = load_reference()
    inp = inputs()
    q = inp["pos"].double() / SIZE
    assert float((q - torch.floor(q) - 0.5).abs().min()) >= HALF_MARGIN
    shared = {k: v for k, v in inp.items()}
    names = {}
    for kind in ("unet", "encoder"):
        Scorer = make_scorer(kind, modules, mp, Seq)
        seed = 0
        while True:
            state = {k: v.clone() for k, v in mgm.init(Scorer(), 2000 + seed).state_dict().items()}
            r32, m32, s32 = run(kind, Scorer, gt, inp, torch.float32, state)
            r64, m64, s64 = run(kind, Scorer, gt, inp, torch.float64, state)
            ok = (min(s32["kink"], s64["kink"]) >= KINK_MARGIN and min(s32["win"], s64["win"]) >= MAX_MARGIN
                  and s64["coarse"] >= COARSE_ROWS)
            print("%s seed %d: activation input %.3g, maximum wins by %.3g, coarsest rows %d" % (kind, seed, s64["kink"], s64["win"],
                                                                                                 s64["coarse"]), flush=True)
            if ok:
                break
            seed += 1
        assert torch.equal(r32["voxel_coords"], r64["voxel_coords"]) and torch.equal(r32["voxel_batch"], r64["voxel_batch"])
        assert len(r32["voxel_coords"]) < len(inp["members"])  # some voxel holds several points
        rec = dict(shared)
        rec["seed"] = np.array([seed])
        rec["margins"] = np.array([min(s32["kink"], s64["kink"]), min(s32["win"], s64["win"]), s64["coarse"]])
        for k, v in state.items():
            rec["state/" + k] = v
        for k, v in r32.items():
            rec[k] = v
        for k in ("scores", "grad_x", "voxel_x"):
            rec["f64/" + k] = r64[k].numpy()
        for k, v in m32.state_dict().items():
            if "running_" in k:
                rec["after/" + k] = v.clone()
                rec["f64/after/" + k] = m64.state_dict()[k].numpy()
        grads = {}
        for (k, p), (_, p64) in zip(m32.named_parameters(), m64.named_parameters()):
            # the fp32 pass's gradients are kept as their distance to the float64 ones only, and the float64 ones rounded to
            # fp32 (half an ulp, 6e-8 relative, against a bar of 1e-4): the weights alone are 0.6 MB of the 1 MiB a file may have
            grads["pgrad_own/" + k] = np.array([float((p.grad.double() - p64.grad).abs().max())])
            grads["f64/pgrad/" + k] = p64.grad.numpy().astype(np.float32)
        names[kind] = [[k, list(v.shape)] for k, v in m32.state_dict().items()]
        for tail, part in (("", rec), ("_grads", grads)):
            path = os.path.join(HERE, "pointgroup_scorer_%s%s.npz" % (kind, tail))
            np.savez_compressed(path, **mg.to_np(part))
            assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
            print("wrote %s (%d arrays, %d bytes)" % (path, len(part), os.path.getsize(path)))
    with open(os.path.join(HERE, "pointgroup_config.json"), "w") as f:
        json.dump({"entries": resolved_pointgroup_yaml(4), "feat": 4, "state_dicts": names,
                   "fixture": dict(size=SIZE, in_feat=IN_FEAT, sizes=SIZES, unet=scorer_config("unet"), encoder=scorer_config("encoder"))},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote pointgroup_config.json")


if __name__ == "__main__":
    main()
