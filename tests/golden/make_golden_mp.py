"""Generator of tests/golden/pointnet2_mp.npz: the REFERENCE's message-passing PointNet++ on the CPU.

Runs the reference's own classes, loaded from the reference tree over the stand-in modules of make_golden.py:
  * `SAModule` (modules/pointnet2/message_passing.py:9-31) over `BaseMSConvolutionDown`, `GlobalBaseModule`, `FPModule`
    (core/base_conv/message_passing.py:61-94, 132-151, 157-176), `MLP` / `FastBatchNorm1d` (core/common_modules),
    `FPSSampler`, `MultiscaleRadiusNeighbourFinder` (core/spatial_ops), nested by the reference's
    `UnetSkipConnectionBlock` (models/base_architectures/unet.py:244-306, loaded by file path as
    make_golden.build_reference_nested_unet does) in the order `_init_from_compact_format` (:93-138) prescribes, with
    the three Linear layers of `Segmentation_MP` (models/segmentation/base.py:27-55) behind it.

torch_geometric / torch_cluster / torch_scatter are not installed; what those classes call is bound as follows:
  * `fps(pos, batch, ratio)`      -> per cloud, the oracle's dense FPS (oracle.tpk_ref.furthest_point_sample on the
    (1, n_b, 3) slice: start at the cloud's first row, ties to the lowest index) with the quota
    ceil(float32(n_b) * float32(ratio)) of tests/pointnet2_mp_ref.fps_quota.  torch_cluster draws a random start by
    default and its rounding cannot be read here: both are this project's stated conventions, not pinned behaviour.
  * `radius(x, y, r, batch_x, batch_y, max_num_neighbors)` -> oracle.tpk_ref.ball_query(mode="partial_dense"),
    compacted: (row = query, col = support row), a query's first max_num_neighbors hits in ascending support index.
  * `knn_interpolate`             -> oracle kNN + the published inverse-squared-distance blend (the stand-in of
    make_golden.make_kpconv_blocks_case).
  * `global_max_pool(x, batch)`   -> the max over the rows of each cloud.
  * `PointConv(local_nn, global_nn)` -> what PyG documents for it WITHOUT self-loop rewriting:
    out_i = global_nn(max_j local_nn(cat([x_j, pos_j - pos_i]))), pos = (source positions, target positions),
    edge_index = [source rows; target rows].
  * `BaseMSConvolutionDown.forward` (:80) calls `self.sampler(pos, batch)`, and `BaseSampler.__call__`'s second
    positional parameter is `x`: the batch vector reaches `fps` as None and the whole batch would be sampled as ONE
    cloud.  The fixture evaluates the call the way the call site evidently means it (the batch vector is the batch
    vector); nothing else of the sampler is touched.

The clouds have 97, 160 and 64 points; with ratios 0.25 / 0.25 the levels hold 25 / 40 / 16 and 7 / 10 / 4 points.
Conditions on the inputs, asserted below: at the first level some queries are cut at max_num_neighbors and others are
not, and no query of any level or scale is left without an edge.

Stored (data only): inputs, state_dict, sampled indices and CSR edges per level and scale, every stage's train-mode
output in float32 and the same pass in float64, the BatchNorm buffers after the step, the eval-mode outputs, a cotangent
with parameter and input gradients, the relative-L2 distance of the float32 gradients to the float64 ones, and one
two-scale SAModule (the `pointnet2ms` form).

    python tests/golden/make_golden_mp.py
"""
import copy
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
import pointnet2_mp_ref as ref  # noqa: E402
from oracle import tpk_ref  # noqa: E402

SIZES, FEAT, CLASSES, CAP, CFG, MS = ref.GOLD_SIZES, ref.GOLD_FEAT, ref.GOLD_CLASSES, ref.GOLD_CAP, ref.GOLD_CFG, ref.GOLD_MS

EDGE_LOG = []  # (edge_start, col) of every radius search, in call order


def fps(pos, batch=None, ratio=0.5, random_start=False):
    assert not random_start
    batch = torch.zeros(pos.shape[0], dtype=torch.long) if batch is None else batch
    counts = torch.bincount(batch).tolist()
    out, base = [], 0
    for n, q in zip(counts, ref.fps_quota(counts, ratio)):
        if n and q:
            out.append(tpk_ref.furthest_point_sample(pos[base:base + n].float().unsqueeze(0), q)[0] + base)
        base += n
    return torch.cat(out)


def radius(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    table, _ = tpk_ref.ball_query(r, max_num_neighbors, x.float(), y.float(), mode="partial_dense", batch_x=batch_x,
                                  batch_y=batch_y)
    edge_start, col = ref.table_edges(table)
    EDGE_LOG.append((edge_start, col))
    row = torch.repeat_interleave(torch.arange(y.shape[0]), edge_start[1:] - edge_start[:-1])
    return row, col


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, num_workers=1):
    idx, _ = tpk_ref.knn(k, pos_x.float(), pos_y.float(), batch_x, batch_y)
    Nq = pos_y.shape[0]
    y_idx = torch.arange(Nq).repeat_interleave(k)
    x_idx = idx.reshape(-1)
    keep = x_idx >= 0
    y_idx, x_idx = y_idx[keep], x_idx[keep]
    d2 = ((pos_x[x_idx] - pos_y[y_idx]) ** 2).sum(-1, keepdim=True)
    w = 1.0 / torch.clamp(d2, min=1e-16)
    num = torch.zeros(Nq, x.shape[1], dtype=x.dtype).index_add_(0, y_idx, x[x_idx] * w)
    return num / torch.zeros(Nq, 1, dtype=x.dtype).index_add_(0, y_idx, w)


def global_max_pool(x, batch):
    return torch.stack([x[batch == b].max(0)[0] for b in range(int(batch.max()) + 1)])


class PointConv(torch.nn.Module):
    def __init__(self, local_nn=None, global_nn=None, **kwargs):
        super().__init__()
        self.local_nn, self.global_nn = local_nn, global_nn

    def forward(self, x, pos, edge_index):
        pos_j, pos_i = pos
        src, dst = edge_index[0], edge_index[1]
        msg = pos_j[src] - pos_i[dst]
        if x is not None:
            msg = torch.cat([x[src], msg], 1)
        if self.local_nn is not None:
            msg = self.local_nn(msg)
        nq = pos_i.shape[0]
        edge_start = torch.zeros(nq + 1, dtype=torch.int64)
        edge_start[1:] = torch.cumsum(torch.bincount(dst, minlength=nq), 0)
        assert bool((dst[1:] >= dst[:-1]).all()) and int((edge_start[1:] == edge_start[:-1]).sum()) == 0
        out = ref.segment_max(msg, edge_start)[0]
        return out if self.global_nn is None else self.global_nn(out)


class _Data(mg._Bag):
    pass


def load_reference():
    mg.install_stubs()
    tgnn = sys.modules["torch_geometric.nn"]
    tgnn.fps, tgnn.radius, tgnn.knn_interpolate, tgnn.global_max_pool, tgnn.PointConv = (
        fps, radius, knn_interpolate, global_max_pool, PointConv)
    mg._stub("torch_points3d.datasets.base_dataset", BaseDataset=object)
    mg._stub("torch_points3d.models.base_model", BaseModel=torch.nn.Module, BaseInternalLossModule=torch.nn.Module)
    import torch_points3d.core.base_conv.message_passing as ref_mp
    import torch_points3d.core.spatial_ops.neighbour_finder as ref_nf
    import torch_points3d.core.spatial_ops.sampling as ref_sampling
    import torch_points3d.modules.pointnet2.message_passing as ref_sa
    ref_mp.Batch = _Data
    ref_mp.knn_interpolate, ref_mp.global_max_pool, ref_nf.radius, ref_sa.PointConv = (
        knn_interpolate, global_max_pool, radius, PointConv)
    # the call site passes the batch vector second (see the docstring)
    ref_sampling.BaseSampler.__call__ = lambda self, pos, batch=None, x=None: self.sample(pos, batch=batch, x=x)
    spec = importlib.util.spec_from_file_location(
        "_ref_unet", os.path.join(mg.REF, "torch_points3d/models/base_architectures/unet.py"))
    unet = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(unet)
    return ref_mp, ref_sa, unet


def build_net(ref_mp, ref_sa, unet):
    down, up = CFG["down_conv"], CFG["up_conv"]
    lib = types.SimpleNamespace(GlobalBaseModule=ref_mp.GlobalBaseModule)
    n = len(down["down_conv_nn"])

    def down_args(i):
        return dict(down_conv_cls=ref_sa.SAModule, ratio=down["ratios"][i], radius=down["radius"][i],
                    radius_num_point=down["radius_num_points"][i], down_conv_nn=down["down_conv_nn"][i], index=i)

    def up_args(j):
        return dict(up_conv_cls=ref_mp.FPModule, up_k=up["up_k"][j], up_conv_nn=up["up_conv_nn"][j], skip=True, index=j)

    block = unet.UnetSkipConnectionBlock(args_up=up_args(0), modules_lib=lib, innermost=True,
                                         args_innermost=dict(module_name="GlobalBaseModule", **CFG["innermost"]))
    for index in range(n - 1, 0, -1):
        block = unet.UnetSkipConnectionBlock(args_up=up_args(n - index), args_down=down_args(index), submodule=block)
    net = torch.nn.Module()
    net.model = unet.UnetSkipConnectionBlock(args_up=up_args(n), args_down=down_args(0), submodule=block, outermost=True)
    w = CFG["mlp_cls"]["nn"]
    net.lin1, net.lin2, net.lin3 = torch.nn.Linear(w[0], w[1]), torch.nn.Linear(w[2], w[3]), torch.nn.Linear(w[4], CLASSES)
    return net


def stages(net):
    b0 = net.model
    b1 = b0.submodule
    b2 = b1.submodule
    return b0.down, b1.down, b2.inner, b2.up, b1.up, b0.up


def head(net, x):
    x = torch.nn.functional.relu(net.lin1(x))
    return torch.nn.functional.log_softmax(net.lin3(net.lin2(x)), dim=-1)


def run(net, data):
    """the chained network, stage by stage (what UnetSkipConnectionBlock.forward nests); returns every stage's bag"""
    sa1, sa2, glob, fp0, fp1, fp2 = stages(net)
    d1 = sa1(data)
    d2 = sa2(d1)
    dg = glob(d2)
    u0 = fp0((dg, d2))
    u1 = fp1((u0, d1))
    u2 = fp2((u1, data))
    return dict(sa1=d1, sa2=d2, glob=dg, fp0=u0, fp1=u1, fp2=u2, out=_Data(x=head(net, u2.x)))


def rel_l2(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-300))


def main():
    ref_mp, ref_sa, unet = load_reference()
    g = torch.Generator().manual_seed(2024)
    pos = torch.cat([torch.rand(n, 3, generator=g) * 2 - 1 for n in SIZES])
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    x = torch.randn(pos.shape[0], FEAT, generator=g)
    torch.manual_seed(7)
    net = build_net(ref_mp, ref_sa, unet).train()
    rec = {"pos": pos, "batch": batch, "x": x, "cap": torch.tensor([CAP])}
    for k, v in net.state_dict().items():
        rec["sd/" + k] = v.detach().clone()
    net64 = copy.deepcopy(net).double()

    # ---- train-mode pass in float32, one backward
    del EDGE_LOG[:]
    xin = x.clone().requires_grad_(True)
    out = run(net, _Data(pos=pos, batch=batch, x=xin))
    assert len(EDGE_LOG) == 2
    for level, (edge_start, col) in enumerate(EDGE_LOG):
        deg = edge_start[1:] - edge_start[:-1]
        assert int(deg.min()) >= 1, "a query without an edge"
        print("  level %d: %d queries, %d edges, %d at the cap, %d below it" % (
            level + 1, deg.numel(), col.numel(), int((deg == CAP).sum()), int((deg < CAP).sum())))
        if level == 0:
            assert int((deg == CAP).sum()) >= 5 and int((deg < CAP).sum()) >= 5
        rec["edges/sa%d/edge_start" % (level + 1)], rec["edges/sa%d/col" % (level + 1)] = edge_start, col
    assert [int((out["sa2"].batch == b).sum()) for b in range(3)] == [7, 10, 4]
    cot = torch.randn(out["out"].x.shape, generator=g)
    (out["out"].x * cot).sum().backward()
    rec["cot"] = cot
    for k in ("sa1", "sa2"):
        rec[k + "/idx"], rec[k + "/pos"], rec[k + "/batch"] = out[k].idx, out[k].pos, out[k].batch
    for k, d in out.items():
        rec[k + "/x"] = d.x
    for k, v in net.state_dict().items():
        if "running_" in k or "num_batches" in k:
            rec["after/" + k] = v.detach().clone()

    # ---- the same pass in float64 (same samples and edges: positions go through the float32 searches on both sides)
    x64 = x.double().clone().requires_grad_(True)
    out64 = run(net64, _Data(pos=pos.double(), batch=batch, x=x64))
    assert torch.equal(out64["sa2"].idx, out["sa2"].idx)
    (out64["out"].x * cot.double()).sum().backward()
    for k, d in out64.items():
        rec["f64/" + k + "/x"] = d.x.detach().numpy()
    rec["grad/x"] = xin.grad
    rec["grel/x"] = torch.tensor([rel_l2(xin.grad, x64.grad)], dtype=torch.float64).numpy()
    worst = rec["grel/x"][0]
    p64 = dict(net64.named_parameters())
    for k, p in net.named_parameters():
        if p.grad is not None:
            rec["pgrad/" + k] = p.grad
            if not k.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
                r = rel_l2(p.grad, p64[k].grad)
                rec["grel/" + k] = np.array([r])
                worst = max(worst, r)
    print("  float32 gradients vs float64: relative L2 %.2e (input), worst parameter %.2e" % (rec["grel/x"][0], worst))

    # ---- eval mode, on the statistics the step left
    net.eval()
    with torch.no_grad():
        ev = run(net, _Data(pos=pos, batch=batch, x=x))
    for k, d in ev.items():
        rec["eval/" + k + "/x"] = d.x

    # ---- one two-scale SAModule (pointnet2ms form)
    torch.manual_seed(11)
    ms = ref_sa.SAModule(**MS).train()
    for k, v in ms.state_dict().items():
        rec["ms/sd/" + k] = v.detach().clone()
    ms64 = copy.deepcopy(ms).double()
    del EDGE_LOG[:]
    mx = x.clone().requires_grad_(True)
    mo = ms(_Data(pos=pos, batch=batch, x=mx))
    assert len(EDGE_LOG) == 2 and all(int((es[1:] - es[:-1]).min()) >= 1 for es, _ in EDGE_LOG)
    for s, (edge_start, col) in enumerate(EDGE_LOG):
        rec["ms/edges%d/edge_start" % s], rec["ms/edges%d/col" % s] = edge_start, col
    mcot = torch.randn(mo.x.shape, generator=g)
    (mo.x * mcot).sum().backward()
    mx64 = x.double().clone().requires_grad_(True)
    mo64 = ms64(_Data(pos=pos.double(), batch=batch, x=mx64))
    (mo64.x * mcot.double()).sum().backward()
    rec["ms/grel/x"] = np.array([rel_l2(mx.grad, mx64.grad)])
    rec.update({"ms/idx": mo.idx, "ms/x": mo.x, "ms/f64/x": mo64.x.detach().numpy(), "ms/cot": mcot, "ms/grad_x": mx.grad})
    for k, v in ms.state_dict().items():
        if "running_" in k:
            rec["ms/after/" + k] = v.detach().clone()
    ms.eval()
    with torch.no_grad():
        rec["ms/eval/x"] = ms(_Data(pos=pos, batch=batch, x=x)).x

    path = os.path.join(HERE, "pointnet2_mp.npz")
    np.savez_compressed(path, **mg.to_np(rec))
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    dist = lambda k: float((out[k].x.detach().double() - out64[k].x.detach()).abs().max())  # noqa: E731
    print("wrote %s (%.1f KiB, %d arrays); float32-vs-float64 distance of the reference pass: %s" % (
        path, size / 1024.0, len(rec), ", ".join("%s %.1e" % (k, dist(k)) for k in out)))


if __name__ == "__main__":
    main()
