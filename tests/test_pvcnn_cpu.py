"""PVCNN without a GPU: properties of the restatement tests/pvcnn_ref.py the GPU tests lean on, the fixture
tests/golden/pvcnn.npz (the reference's own PVCNN) against that restatement, its safety conditions, the model's
state_dict keys, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import pvcnn_golden_util as gu
import pvcnn_ref as pref


def _points(n=600, seed=0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * 4.0 - 2.0  # both sides of 0, several points per voxel
    return torch.cat([xyz, torch.randint(0, 2, (n, 1), generator=g).float()], 1)


@pytest.mark.parametrize("s", [1, 2])
def test_devoxelize_reproduces_a_linear_field_where_all_corners_exist(s):
    pc = _points()
    q = pref.quantize(pc, s)
    C = pref.voxel_set(q)
    idx8 = pref.lookup8(q, s, C)
    w, _ = pref.trilinear_weights(pc, idx8, s, torch.float64)
    full = (idx8 >= 0).all(1)
    assert int(full.sum()) > 20 and int((~full).sum()) > 20
    a = torch.tensor([0.3, -1.2, 0.7], dtype=torch.float64)
    field = (C[:, :3].double() @ a + 0.5).unsqueeze(1)  # f(v) = a . v + b on the voxel corners
    got = pref.devoxelize(field, idx8, w)[full, 0]
    want = pc[full, :3].double() @ a + 0.5
    assert float((got - want).abs().max()) < 1e-6  # (the 1e-8 of the normalisation, times |f|)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_weights_sum_to_one_where_a_corner_exists(dtype):
    pc = _points()
    q = pref.quantize(pc, 1)
    C = pref.voxel_set(q)[::3].contiguous()  # a set that lacks most corners and some points' own voxels
    idx8 = pref.lookup8(q, 1, C)
    w, _ = pref.trilinear_weights(pc, idx8, 1, dtype)
    some = (idx8 >= 0).any(1)
    assert int(some.sum()) > 50 and int((~some).sum()) > 0
    assert bool((w >= 0).all()) and float(w[idx8 < 0].abs().max()) == 0.0
    # sum = S / (S + 1e-8) with S the weight that exists: 1 - O(1e-8 / S)
    total = w[some].double().sum(1)
    assert bool((total <= 1.0 + 1e-6).all()) and float((1.0 - total).median()) < 1e-6
    assert float(w[~some].abs().sum()) == 0.0
    wn, idxn = pref.trilinear_weights(pc, idx8, 1, dtype, nearest=True)
    assert float(wn[:, 1:].abs().sum()) == 0.0 and bool((idxn[:, 1:] == -1).all()) and torch.equal(wn[:, 0], w[:, 0])


def test_voxelize_is_the_mean_of_a_hand_computed_case():
    # floor, not truncation: -0.5 lies in voxel -1.  Voxels (batch, x, y, z) ascending: (0;-1,0,0) <- points 1, 3;
    # (0;0,0,0) <- points 0, 4; (1;0,0,0) <- point 2
    pc = torch.tensor([[0.5, 0.5, 0.5, 0], [-0.5, 0.5, 0.5, 0], [0.25, 0.75, 0.5, 1], [-0.25, 0.25, 0.75, 0], [0.75, 0.25, 0.25, 0]])
    Fx = torch.tensor([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0], [5.0, 50.0]])
    q = pref.quantize(pc, 1)
    C = pref.voxel_set(q)
    assert C.tolist() == [[-1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    idx = pref.lookup1(q, C)
    assert idx.tolist() == [1, 0, 2, 0, 1] and pref.counts(idx, 3).tolist() == [2, 2, 1]
    assert torch.equal(pref.voxelize(Fx, idx, 3), torch.tensor([[3.0, 30.0], [3.0, 30.0], [3.0, 30.0]]))
    extra = torch.cat([C, torch.tensor([[9, 9, 9, 0]], dtype=torch.int32)])  # a voxel without a point: a zero row
    assert pref.voxelize(Fx, pref.lookup1(q, extra), 4)[3].tolist() == [0.0, 0.0]
    assert pref.quantize(torch.tensor([[-33.0, -32.0, 31.5, 2.0]]), 16).tolist() == [[-48, -32, 16, 2]]


def test_model_state_dict_equals_the_fixture():
    from torch_points3d_amd import pvcnn as pv
    cfg = gu.config()
    net = pv.pvcnn(cfg["cr"], cfg["vres"], cfg["num_features"], cfg["num_classes"])
    want = gu.state_dict()
    have = net.state_dict()
    assert sorted(have.keys()) == sorted(want.keys())
    for k, v in have.items():
        assert tuple(v.shape) == tuple(want[k].shape), k
    assert net.dropout.p == 0.3 and net.dropout.inplace and net.vres == cfg["vres"]
    for name in ("stem", "stage1", "stage2", "stage3", "stage4", "up1", "up2", "up3", "up4", "classifier", "point_transforms"):
        assert hasattr(net, name)
    for m in net.modules():  # weight_initialization
        if isinstance(m, torch.nn.BatchNorm1d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    import torch_points3d_amd
    for name in ("PVCNN", "PointTensor", "initial_voxelize", "point_to_voxel", "voxel_to_point"):
        assert getattr(torch_points3d_amd, name) is getattr(pv, name)


def test_cpu_tensors_are_refused():
    from torch_points3d_amd import pvcnn as pv
    from torch_points3d_amd import sparseconv as sc
    pc = _points(20)
    z = pv.PointTensor(torch.zeros(20, 4), pc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pv.initial_voxelize(z, 1.0, 0.5)
    x = sc.SparseTensor(torch.zeros(3, 4), torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pv.point_to_voxel(x, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pv.voxel_to_point(x, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pv.pvcnn(0.125, 0.5, 4, 3)(z)


def test_fixture_safety_conditions():
    cfg, g = gu.config(), gu.load()
    v = g["pos"] / cfg["vres"]
    assert float((v - torch.round(v)).abs().min()) >= cfg["coord_margin"] == 1e-3
    assert float(g["relu_min"][0]) >= cfg["kink_margin"] == 5e-5
    assert 1300 <= len(g["pos"]) <= 1700 and sorted(g["batch"].unique().tolist()) == [0, 1]
    assert (cfg["cr"], cfg["vres"], cfg["num_features"], cfg["num_classes"]) == (0.125, 0.5, 5, 7)
    assert tuple(g["out"].shape) == (len(g["pos"]), 7) and g["f64/out"].dtype == np.float64


def test_restatement_reproduces_the_fixture_and_is_clear_of_kinks():
    """the restatement's network with the recorded weights: the fixture's logits and gradients (fp32 against fp32 of another
    summation order), and its own ReLU inputs stay outside the margin the generator asserted"""
    cfg, g = gu.config(), gu.load()
    net = pref.Net(cfg["cr"], cfg["vres"], cfg["num_features"], cfg["num_classes"])
    seen = []
    for m in net.modules():
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_pre_hook(lambda mod, inp: seen.append(float(inp[0].detach().abs().min())))
    x, out = gu.train_step(net, lambda m, f, pos, batch: m(f, torch.cat([pos, batch.unsqueeze(-1).float()], 1)),
                           dtype=torch.float64)
    assert len(seen) == 3 and min(seen) >= cfg["kink_margin"] - 1e-5  # (the fp32 pass met the margin; float64 moves it by ~1e-6)
    scale = max(1.0, float(np.abs(g["f64/out"]).max()))
    assert float((out.detach() - torch.from_numpy(g["f64/out"])).abs().max()) <= 1e-9 * scale
    gscale = max(1.0, float(np.abs(g["f64/grad_x"]).max()))
    assert float((x.grad - torch.from_numpy(g["f64/grad_x"])).abs().max()) <= 1e-9 * gscale
    for k, p in net.named_parameters():
        want = torch.from_numpy(g["f64/pgrad/" + k])
        assert float((gu.sample(p.grad) - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), k
