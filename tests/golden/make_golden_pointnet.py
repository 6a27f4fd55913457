"""Generator of tests/golden/pointnet.npz and pointnet_config.json: the REFERENCE's PointNet modules on the CPU.

Runs the reference's own classes, loaded from the reference tree over the stand-in modules of make_golden.py:
  * `PointNetSeg`, `PointNetSTN3D`, `PointNetSTNkD`, `MiniPointNet` (modules/PointNet/modules.py) over
    `BaseLinearTransformSTNkD` (core/common_modules/spatial_transform.py) and `MLP` / `FastBatchNorm1d`
    (core/common_modules/base_modules.py);
  * `PointNet_Features` of conf/models/segmentation/pointnet.yaml, assembled as models/segmentation/pointnet.py:70-98
    does (a `MiniPointNet` with aggr = "mean" and return_local_out, `forward_embedding`, `MLP(seg_nn)`, log_softmax)
    without `BaseModel`, which needs a real OmegaConf.

torch_geometric is not installed; the two functions these classes call are bound as follows:
  * `global_max_pool(x, batch)`  -> the max over the rows of each cloud;
  * `global_mean_pool(x, batch)` -> the mean over the rows of each cloud.
`BaseInternalLossModule` (models/base_model.py) is bound to torch.nn.Module: only its method name matters here.

The reference builds its identity for `batch_size` clouds, so the networks are constructed with batch_size = 3.

Reduced widths (WIDTHS below); three clouds of 97, 160 and 64 rows; FEAT = 3 feature channels behind the position.  Both
`fc_layer`s, which the reference initialises to zero, are set to small random values, so neither transform is the
identity.  The scalar that is differentiated is (scores * cot).sum() + ORTHO_WEIGHT * orthogonal regularisation loss.

Stored (data only): inputs, state_dict, both `trans`, x after every step, the global feature, the scores, the orthogonal
loss, input and parameter gradients, the BatchNorm buffers after the training pass, the eval-mode scores after it, the
same pass in float64 under "f64/", the same for `PointNet_Features` under "feat/", and in pointnet_config.json the
widths and the state_dict key list of `PointNetSeg` at its published widths (names only).

    python tests/golden/make_golden_pointnet.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

SIZES = [97, 160, 64]
FEAT, CLASSES = 3, 5
ORTHO_WEIGHT = 1.0
CLOUD_SCALE, CLOUD_SHIFT = [0.5, 1.0, 2.0], [-0.5, 0.0, 0.75]
WIDTHS = dict(input_nc=FEAT + 3, input_stn_local_nn=[16, 32, 64], input_stn_global_nn=[64, 32, 16], local_nn_1=[16, 16],
              feat_stn_k=16, feat_stn_local_nn=[16, 32, 64], feat_stn_global_nn=[64, 32, 16],
              local_nn_2=[16, 32, 64], seg_nn=[80, 32, 16, CLASSES])
FEATURES = dict(pointnet=dict(local_nn=[3, 32, 64, 4], global_nn=[4, 2], aggr="mean", return_local_out=True),
                seg_nn=[4 + 2, 50, CLASSES])


def global_max_pool(x, batch):
    return torch.stack([x[batch == b].max(0)[0] for b in range(int(batch.max()) + 1)])


def global_mean_pool(x, batch):
    return torch.stack([x[batch == b].mean(0) for b in range(int(batch.max()) + 1)])


def load_reference():
    mg.install_stubs()
    tgnn = sys.modules["torch_geometric.nn"]
    tgnn.global_max_pool, tgnn.global_mean_pool = global_max_pool, global_mean_pool
    mg._stub("torch_points3d.datasets.base_dataset", BaseDataset=object)
    mg._stub("torch_points3d.models.base_model", BaseModel=torch.nn.Module, BaseInternalLossModule=torch.nn.Module)
    import torch_points3d.modules.PointNet.modules as ref
    return ref


def run_seg(net, x, batch):
    """PointNetSeg.forward (modules.py:95-114), step by step over the reference's own sub-modules"""
    rec = {}
    rec["x_input_stn"] = x1 = net.input_stn(x, batch)
    rec["trans_input"] = net.input_stn.trans
    rec["x_local_nn_1"] = x2 = net.local_nn_1(x1)
    rec["x_feat_stn"] = x3 = net.feat_stn(x2, batch)
    rec["trans_feat"] = net.feat_stn.trans
    rec["x_local_nn_2"] = x4 = net.local_nn_2(x3)
    rec["global_feature"] = g = net.func_global_max_pooling(x4, batch)
    rec["out"] = net.seg_nn(torch.cat([x3, g[batch]], dim=1))  # (the concatenation holds nothing new: not stored)
    rec["ortho_loss"] = net.feat_stn.get_orthogonal_regularization_loss()
    return rec


class Features(torch.nn.Module):
    """SegPointNetModel.__init__ / forward of models/segmentation/pointnet.py:70-98 without BaseModel"""

    def __init__(self, ref):
        super().__init__()
        p = FEATURES["pointnet"]
        self.pointnet_seg = ref.MiniPointNet(p["local_nn"], p["global_nn"], aggr=p["aggr"], return_local_out=p["return_local_out"])
        self.seg_nn = ref.MLP(FEATURES["seg_nn"])

    def forward(self, pos, batch):
        x = self.pointnet_seg.forward_embedding(pos, batch)
        return torch.nn.functional.log_softmax(self.seg_nn(x), dim=-1)


def bn_state(net):
    return {k: v for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k}


def one_pass(net, inputs, cot, run, out, prefix):
    """train-mode forward + backward, the buffers after it, the eval-mode scores after it; everything into `out`"""
    net.train()
    leaf = inputs[0].clone().requires_grad_(True)
    rec = run(net, leaf, *inputs[1:])
    loss = (rec["out"] * cot).sum()
    if "ortho_loss" in rec:
        loss = loss + ORTHO_WEIGHT * rec["ortho_loss"]
    loss.backward()
    for k, v in rec.items():
        out[prefix + k] = v.detach()
    out[prefix + "grad_x"] = leaf.grad
    for k, p in net.named_parameters():
        out[prefix + "grad/" + k] = p.grad
    for k, v in bn_state(net).items():
        out[prefix + "after/" + k] = v.clone()
    net.eval()
    with torch.no_grad():
        out[prefix + "eval/out"] = run(net, inputs[0], *inputs[1:])["out"]


def rel_l2(a, b, weight=None):
    """relative L2 distance.  A bias whose gradient is zero in exact arithmetic (a Linear bias, or the BatchNorm bias in
    front of a pool, whose per-channel constant the next training-mode BatchNorm removes; float64 norm below 1e-9 of its
    weight's) is measured against the gradient of its weight instead of its own rounding noise."""
    scale = float(b.double().norm())
    if weight is not None and scale < 1e-9 * float(weight.double().norm()):
        scale = float(weight.double().norm())
    return float((a.double() - b.double()).norm() / (scale + 1e-300))


def main():
    ref = load_reference()
    gen = torch.Generator().manual_seed(2026)
    N = sum(SIZES)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    x = torch.cat([torch.rand(N, 3, generator=gen) * 2 - 1, torch.randn(N, FEAT, generator=gen)], 1)
    # the clouds differ in extent and offset (as scans do), so that their pooled features differ and the three-row
    # training-mode BatchNorms of the regressors do not divide by a deviation far below their inputs
    x = x * torch.tensor(CLOUD_SCALE)[batch, None] + torch.tensor(CLOUD_SHIFT)[batch, None]
    cot = torch.randn(N, CLASSES, generator=gen)
    out = {"x": x, "batch": batch.to(torch.int16), "cot": cot}

    torch.manual_seed(7)
    net = ref.PointNetSeg(batch_size=len(SIZES), **WIDTHS)
    with torch.no_grad():
        for stn in (net.input_stn, net.feat_stn):  # zero in the reference: the transform would be the identity
            stn.fc_layer.weight.copy_(torch.randn(stn.fc_layer.weight.shape, generator=gen) * 0.05)
            stn.fc_layer.bias.copy_(torch.randn(stn.fc_layer.bias.shape, generator=gen) * 0.05)
    for k, v in net.state_dict().items():
        out["w/" + k] = v.clone()
    whole = copy.deepcopy(net).train()(x, batch)
    net64 = copy.deepcopy(net).double()
    one_pass(net, (x, batch), cot, run_seg, out, "")
    assert torch.equal(whole, out["out"]), "the step-by-step pass is not PointNetSeg.forward"
    one_pass(net64, (x.double(), batch), cot.double(), run_seg, out, "f64/")
    eye = torch.eye(WIDTHS["feat_stn_k"])
    assert float((out["trans_feat"] - eye).abs().max()) > 0.05 and float((out["trans_input"] - torch.eye(3)).abs().max()) > 0.05

    torch.manual_seed(11)
    feat = Features(ref)
    for k, v in feat.state_dict().items():
        out["feat/w/" + k] = v.clone()
    feat64 = copy.deepcopy(feat).double()
    pos = x[:, :3].contiguous()
    run_feat = lambda m, p, b: {"out": m(p, b)}  # noqa: E731
    one_pass(feat, (pos, batch), cot, run_feat, out, "feat/")
    one_pass(feat64, (pos.double(), batch), cot.double(), run_feat, out, "f64/feat/")

    # condition on the inputs: every float32 gradient sits within 1e-4 (relative L2) of its float64 evaluation, so no
    # LeakyReLU kink or arg-max switch separates the two passes
    worst = 0.0
    for k in sorted(out):
        if "grad" in k and not k.startswith("f64/"):
            d = rel_l2(out[k], out["f64/" + k], out.get("f64/" + k[:-4] + "weight") if k.endswith("bias") else None)
            worst = max(worst, d)
            assert d < 1e-4, "%s: the float32 gradient is %.2e (relative L2) from the float64 one: pick other inputs" % (k, d)
    print("largest relative L2 distance of a float32 gradient to its float64 evaluation: %.2e" % worst)

    published = ref.PointNetSeg()
    cfg = dict(sizes=SIZES, feat=FEAT, classes=CLASSES, ortho_weight=ORTHO_WEIGHT, widths=WIDTHS, features=FEATURES,
               published_state_dict_keys=list(published.state_dict().keys()))
    with open(os.path.join(HERE, "pointnet_config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
        f.write("\n")
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "pointnet.npz"), **arrays)
    print("wrote pointnet.npz (%d arrays, %.2f MB) and pointnet_config.json" % (
        len(arrays), os.path.getsize(os.path.join(HERE, "pointnet.npz")) / 1e6))


if __name__ == "__main__":
    main()
