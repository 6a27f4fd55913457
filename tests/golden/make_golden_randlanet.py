"""Generator of tests/golden/randlanet*.npz and randlanet_config.json: the REFERENCE's RandLA-Net segmentation
networks (conf/models/segmentation/randlanet.yaml `Randlanet_Conv`, `Randlanet_Res`) on the CPU.

Runs the reference's own classes, loaded from the reference tree:
  * `RandlaConv` / `RandLANetRes` (modules/RandLANet/modules.py:57-123) as the down modules, `GlobalBaseModule` and
    `FPModule` (core/base_conv/message_passing.py:132-151, 157-176), nested by `UnetSkipConnectionBlock`
    (models/base_architectures/unet.py:244-306) in the order `_init_from_compact_format` (:93-138) prescribes and with
    the arguments `_fetch_arguments_from_list` (:199-216) hands over, with the three Linear layers of `Segmentation_MP`
    (models/segmentation/base.py:27-55) behind it, nested the way make_golden_mp.py nests PointNet2_MP.
  * The widths are read from the reference's YAML; `FEAT` is resolved by evaluating its expressions.

What is not installed is bound by the other generators and IMPORTED from them, not copied:
  * the `MessagePassing` stand-in, the `knn` binding and the "callsite" tuple order are those of make_golden.py's
    `make_randla_case`.  They are local to that function, so it is run once (its own fixture goes to a scratch
    directory) and leaves them installed in the stand-in modules;
  * `knn_interpolate`, `global_max_pool`, the unet loader and the head (no dropout) are make_golden_mp.py's.

One cloud of 1024 points (RandomSampler's draw is unsorted, so `batch[idx]` of several clouds would be unsorted from the
second level on, which torch_cluster's knn does not accept -- see make_randla_case), FEAT = 3, 5 classes.  Level sizes
1024 / 256 / 64 / 16 (`Randlanet_Conv`) and 1024 / 1024 / 512 / 256 (`Randlanet_Res`): every kNN has at least 16 support
points, so no neighbour table has a -1 slot (asserted).

The initial weights are rounded to 8 mantissa bits before anything runs (they are arbitrary; the rounded values ARE
the weights of every pass), which lets the archive compress them.  Stored, data only, per config: inputs, state_dict,
the recorded `randint` draws, the train-mode output in float32 and float64, the BatchNorm buffers after the step, the
eval-mode output, one cotangent, the float64 input and parameter gradients (rounded to float32: 6e-8 relative) and the
relative L2 of the float32 gradients to them.  No committed file may exceed 1 MiB, so `Randlanet_Res` (236 368
parameters) is split: randlanet.npz (Conv), randlanet_res.npz, randlanet_res_grads.npz.

    python tests/golden/make_golden_randlanet.py
"""
import copy
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_mp as mgmp  # noqa: E402

N, FEAT, CLASSES, K = 1024, 3, 5, 16


def resolve(node, feat):
    """the YAML's numbers: strings such as "2 * FEAT" or "128 + 128" evaluated"""
    if isinstance(node, dict):
        return {k: resolve(v, feat) for k, v in node.items()}
    if isinstance(node, list):
        return [resolve(v, feat) for v in node]
    if isinstance(node, str) and any(ch.isdigit() for ch in node) or node == "FEAT":
        return int(eval(node, {"__builtins__": {}}, {"FEAT": feat}))  # noqa: S307 (arithmetic of a config file)
    return node


def reference_configs(feat):
    with open(os.path.join(mg.REF, "conf/models/segmentation/randlanet.yaml")) as f:
        raw = yaml.safe_load(f)
    return {name: resolve(raw[name], feat) for name in ("Randlanet_Conv", "Randlanet_Res")}


def load_reference():
    ref_mp, _, unet = mgmp.load_reference()
    # make_randla_case installs its MessagePassing stand-in and knn binding into the stand-in torch_geometric and sets
    # the "callsite" tuple order for its block-level part, which runs last; its own archive goes to a scratch directory
    here = mg.HERE
    with tempfile.TemporaryDirectory() as tmp:
        mg.HERE = tmp
        try:
            mg.make_randla_case()
        finally:
            mg.HERE = here
    standin = sys.modules["torch_geometric.nn"].MessagePassing
    assert standin.tuple_order == "callsite"
    spec = importlib.util.spec_from_file_location(
        "_ref_randla_net", os.path.join(mg.REF, "torch_points3d/modules/RandLANet/modules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert issubclass(mod.RandlaKernel, standin)
    ref_mp.knn_interpolate, ref_mp.global_max_pool = mgmp.knn_interpolate, mgmp.global_max_pool
    return ref_mp, mod, unet


def fetch(opt, index):
    """`_fetch_arguments_from_list`: entry `index` of every list-valued field (a trailing "s" dropped), scalars as is"""
    args = {}
    for name, v in opt.items():
        if isinstance(v, list) and len(v) > 0:
            if name[-1] == "s":
                name = name[:-1]
            v = copy.deepcopy(v[index])
        args[name] = v
    return args


def build_net(cfg, ref_mp, mod, unet):
    down, up = cfg["down_conv"], cfg["up_conv"]
    n = len(down["down_conv_nn"])
    lib = types.SimpleNamespace(GlobalBaseModule=ref_mp.GlobalBaseModule)

    def down_args(i):
        return dict(fetch(down, i), down_conv_cls=getattr(mod, down["module_name"]), index=i)

    def up_args(j, index=None):
        a = dict(fetch(up, j), up_conv_cls=ref_mp.FPModule)
        if index is not None:
            a["index"] = index
        return a

    block = unet.UnetSkipConnectionBlock(args_up=up_args(0), modules_lib=lib, innermost=True,
                                         args_innermost=copy.deepcopy(cfg["innermost"]))
    for index in range(n - 1, 0, -1):
        block = unet.UnetSkipConnectionBlock(args_up=up_args(n - index, index), args_down=down_args(index), submodule=block)
    net = torch.nn.Module()
    net.model = unet.UnetSkipConnectionBlock(args_up=up_args(n, 0), args_down=down_args(0), submodule=block, outermost=True)
    w = cfg["mlp_cls"]["nn"]
    net.lin1, net.lin2, net.lin3 = torch.nn.Linear(w[0], w[1]), torch.nn.Linear(w[2], w[3]), torch.nn.Linear(w[4], CLASSES)
    return net


def round_weights(net):
    """keep 8 mantissa bits of every parameter (see the module docstring)"""
    with torch.no_grad():
        for p in net.parameters():
            p.copy_((p.view(torch.int32) & -65536).view(torch.float32))


def rel_l2(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-300))


def make_case(name, cfg, ref_mp, mod, unet, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(N, 3, generator=g) * 2 - 1
    batch = torch.zeros(N, dtype=torch.long)
    x = torch.randn(N, FEAT, generator=g)
    torch.manual_seed(seed + 1)
    net = build_net(cfg, ref_mp, mod, unet).train()
    round_weights(net)
    rec = {"pos": pos, "batch": batch, "x": x}
    for k, v in net.state_dict().items():
        rec["sd/" + k] = v.detach().clone()
    net64 = copy.deepcopy(net).double()

    drawn, highs = [], []
    real_randint = torch.randint

    def recording_randint(low, high, size, **kw):
        out = real_randint(low, high, size, **kw)
        drawn.append(out.clone())
        highs.append(int(high))
        return out

    def run(model, xx, pp, record):
        torch.manual_seed(seed + 2)  # RandomSampler is the only consumer of the global generator in forward
        if record:
            torch.randint = recording_randint
        try:
            out = model.model(mg._Bag(pos=pp, batch=batch, x=xx))
        finally:
            torch.randint = real_randint
        return mgmp.head(model, out.x)

    xin = x.clone().requires_grad_(True)
    out = run(net, xin, pos, True)
    assert min(highs) >= K, "a level with fewer than %d support points: its neighbour table would have -1 slots" % K
    cot = torch.randn(out.shape, generator=g)
    (out * cot).sum().backward()
    x64 = x.double().clone().requires_grad_(True)
    out64 = run(net64, x64, pos.double(), False)
    (out64 * cot.double()).sum().backward()
    rec.update({"cot": cot, "out": out, "f64/out": out64.detach().numpy()})
    for i, t in enumerate(drawn):
        rec["draw%d" % i] = t
    rec["ndraws"] = torch.tensor([len(drawn)])
    for k, v in net.state_dict().items():
        if "running_" in k or "num_batches" in k:
            rec["after/" + k] = v.detach().clone()
    grads = {"grad64/x": x64.grad.float(), "grel/x": np.array([rel_l2(xin.grad, x64.grad)])}
    worst = grads["grel/x"][0]
    p64 = dict(net64.named_parameters())
    for k, p in net.named_parameters():
        if p.grad is not None:
            grads["pgrad64/" + k] = p64[k].grad.float()
            if not k.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
                r = rel_l2(p.grad, p64[k].grad)
                grads["grel/" + k] = np.array([r])
                if float(p64[k].grad.norm()) > 1e-12:
                    worst = max(worst, r)
    net.eval()
    with torch.no_grad():
        rec["eval/out"] = run(net, x, pos, False)
    own = float((out.detach().double() - out64.detach()).abs().max())
    print("%s: levels %s -> %d rows; %d parameters; float32 pass vs float64 %.2e; float32 gradients vs float64: input "
          "%.2e, worst parameter %.2e" % (name, highs, drawn[-1].numel(), sum(p.numel() for p in net.parameters()), own,
                                          grads["grel/x"][0], worst))
    return rec, grads


def save(fname, rec):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **mg.to_np(rec))
    size = os.path.getsize(path)
    assert size < (1 << 20), (fname, size)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, size / 1024.0, len(rec)))


def main():
    ref_mp, mod, unet = load_reference()
    with open(os.path.join(HERE, "randlanet_config.json"), "w") as f:
        json.dump({"FEAT=%d" % feat: reference_configs(feat) for feat in (3, 6)}, f, indent=1, sort_keys=True)
        f.write("\n")
    cfgs = reference_configs(FEAT)
    rec, grads = make_case("Randlanet_Conv", cfgs["Randlanet_Conv"], ref_mp, mod, unet, 2101)
    rec.update(grads)
    save("randlanet.npz", rec)
    rec, grads = make_case("Randlanet_Res", cfgs["Randlanet_Res"], ref_mp, mod, unet, 2201)
    save("randlanet_res.npz", rec)
    save("randlanet_res_grads.npz", grads)


if __name__ == "__main__":
    main()
