"""Sparse voxel convolution without a GPU: the coordinate rule of the restatement, the rejected inputs, the blocks'
state_dict keys and shapes, the networks' widths, the ABI table."""
import os
import re

import pytest
import torch

import sparseconv_ref as ref
from conftest import ROOT


def test_coordinate_rule_floors_keeps_clouds_apart_and_orders():
    C = torch.tensor([[-1, 0, 3, 0], [-2, 1, 2, 0], [1, 1, 1, 1], [-1, 0, 3, 1], [0, 0, 0, 0], [-3, 5, -4, 0]]).int()
    out = ref.down_coords(C, 2)
    # floor, not truncation: -1 -> -2, -3 -> -4; the two clouds' identical voxels stay separate; order (batch, x, y, z)
    assert out.tolist() == [[-4, 4, -4, 0], [-2, 0, 2, 0], [0, 0, 0, 0], [-2, 0, 2, 1], [0, 0, 0, 1]]
    again = ref.down_coords(out, 4)  # stride 2 -> 4
    assert again.tolist() == [[-4, 0, 0, 0], [-4, 4, -4, 0], [0, 0, 0, 0], [-4, 0, 0, 1], [0, 0, 0, 1]]
    assert [o for o in ref.offsets(3, 2)][:4] == [(-2, -2, -2), (-2, -2, 0), (-2, -2, 2), (-2, 0, -2)]  # x slowest, z fastest
    assert ref.offsets(2, 1) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]


def test_restatement_maps_are_adjoint_and_match_the_dense_convolution():
    g = torch.Generator().manual_seed(0)
    C = torch.unique(torch.cat([torch.randint(-5, 5, (120, 3), generator=g), torch.randint(0, 2, (120, 1), generator=g)], 1),
                     dim=0).int()
    coarse = ref.down_coords(C, 2)
    for k, stride, C_out in ((3, 1, C), (3, 2, coarse), (2, 2, coarse)):
        fwd, inv = ref.kernel_map(C, C_out, k, 1)
        i, kk = torch.nonzero(inv >= 0, as_tuple=True)
        assert torch.equal(fwd[inv[i, kk].long(), kk].long(), i)
        x = torch.randn(len(C), 3, generator=g, dtype=torch.float64)
        W = torch.randn(k ** 3, 3, 5, generator=g, dtype=torch.float64)
        y = ref.conv(x, C, C_out, W, k, stride, 1)
        want = torch.zeros(len(C_out), 5, dtype=torch.float64)
        for j in range(k ** 3):
            hit = fwd[:, j] >= 0
            want[hit] += x[fwd[hit, j].long()] @ W[j]
        torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
        # transposed: the adjoint pairing between the same two sets
        xt = torch.randn(len(C_out), 5, generator=g, dtype=torch.float64)
        Wt = torch.randn(k ** 3, 5, 3, generator=g, dtype=torch.float64)
        yt = ref.conv(xt, C_out, C, Wt, k, stride, 1, transposed=True)
        want = torch.zeros(len(C), 3, dtype=torch.float64)
        for j in range(k ** 3):
            hit = inv[:, j] >= 0
            want[hit] += xt[inv[hit, j].long()] @ Wt[j]
        torch.testing.assert_close(yt, want, rtol=1e-12, atol=1e-12)


def test_rejected_inputs_raise():
    from torch_points3d_amd import sparseconv as sc
    ok = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
    sc.SparseTensor(torch.zeros(3, 2), ok)
    with pytest.raises(ValueError, match="duplicate"):
        sc.SparseTensor(torch.zeros(4, 2), torch.cat([ok, ok[2:]]))
    for bad in ([1 << 18, 0, 0, 0], [0, -(1 << 18), 0, 0], [0, 0, 0, 1 << 9], [0, 0, 0, -1]):
        with pytest.raises(ValueError, match="out of range"):
            sc.SparseTensor(torch.zeros(4, 2), torch.cat([ok, torch.tensor([bad])]))
    sc.SparseTensor(torch.zeros(4, 2), torch.cat([ok, torch.tensor([[(1 << 18) - 1, -(1 << 18) + 1, 0, (1 << 9) - 1]])]))
    with pytest.raises(NotImplementedError, match="dilation"):
        sc.Conv3d(4, 4, dilation=2)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        sc.Conv3d(4, 4, kernel_size=5)
    with pytest.raises(NotImplementedError, match="stride"):
        sc.Conv3dTranspose(4, 4, stride=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.Conv3d(2, 4)(sc.SparseTensor(torch.zeros(3, 2), ok))
    with pytest.raises(ValueError, match="one entry per layer"):
        sc.SparseConv3dUnet("unet_2", input_nc=3)  # the file's kernel_size list is one short (the reference fails too)


def test_blocks_have_the_reference_keys_and_shapes():
    from torch_points3d_amd import sparseconv as sc
    blk = sc.ResBlock(16, 32, sc.Conv3d)
    sd = blk.state_dict()
    assert sd["block.0.kernel"].shape == (27, 16, 32) and sd["block.3.kernel"].shape == (27, 32, 32)
    assert sd["downsample.0.kernel"].shape == (16, 32)
    assert {"block.1.bn.weight", "block.1.bn.running_var", "block.4.bn.num_batches_tracked", "downsample.1.bn.bias"} <= set(sd)
    assert sc.ResBlock(32, 32, sc.Conv3dTranspose).downsample is None
    bott = sc.BottleneckBlock(32, 64, sc.Conv3d).state_dict()
    assert bott["block.0.kernel"].shape == (32, 16) and bott["block.3.kernel"].shape == (27, 16, 16)
    assert bott["block.6.kernel"].shape == (16, 64) and bott["downsample.0.kernel"].shape == (32, 64)
    down = sc.ResNetDown(down_conv_nn=[32, 64], kernel_size=3, stride=2, N=2)
    assert down.state_dict()["conv_in.0.kernel"].shape == (27, 32, 32)  # a strided stage keeps its width in conv_in
    assert down.state_dict()["blocks.1.block.3.kernel"].shape == (27, 64, 64)
    first = sc.ResNetDown(down_conv_nn=[3, 32], kernel_size=3, stride=1, N=0)
    assert first.blocks is None and first.state_dict()["conv_in.0.kernel"].shape == (27, 3, 32)
    up = sc.ResNetUp(up_conv_nn=[256, 128], kernel_size=3, stride=2, N=1)
    assert isinstance(up.conv_in[0], sc.Conv3dTranspose) and up.conv_in[0].transposed
    assert isinstance(up.blocks[0].block[0], sc.Conv3dTranspose) and up.blocks[0].block[0].stride == 1
    assert type(up.blocks[0].downsample[0]) is sc.Conv3d
    assert sc.ResNetDown(down_conv_nn=[8, 8], kernel_size=2, stride=2, N=0).state_dict()["conv_in.0.kernel"].shape == (8, 8, 8)
    # the restatement has the same keys and shapes
    for name in ("unet_4", "encoder_4", "encoder_2"):
        cls = sc.SparseConv3dUnet if name.startswith("unet") else sc.SparseConv3dEncoder
        mine = {k: tuple(v.shape) for k, v in cls(name, input_nc=3).state_dict().items()}
        theirs = {k: tuple(v.shape) for k, v in ref.Net(sc.sparseconv3d_config(name, 3)).state_dict().items()}
        assert mine == theirs, name


def test_network_widths_and_head():
    from torch_points3d_amd import sparseconv as sc
    cfg = sc.sparseconv3d_config("unet_4", 5)
    assert cfg["down_conv"]["down_conv_nn"] == [[5, 32], [32, 32], [32, 64], [64, 128], [128, 256]]
    assert cfg["up_conv"]["up_conv_nn"] == [[256, 128], [256, 128], [192, 96], [128, 96], [128, 96]]
    assert cfg["down_conv"]["N"] == [0, 1, 2, 2, 3] and cfg["up_conv"]["stride"] == [2, 2, 2, 2, 1]
    assert sc.sparseconv3d_config("encoder_4", 1)["innermost"]["nn"] == [256, 256]
    assert sc.sparseconv3d_config("encoder_2", 1)["innermost"]["nn"] == [64, 64]
    net = sc.SparseConv3dUnet("unet_4", input_nc=5, output_nc=13)
    assert net.output_nc == 13 and net.has_mlp_head and net.mlp[0][0].weight.shape == (13, 96) and net.mlp[0][0].bias is None
    assert "mlp.0.1.batch_norm.running_mean" in net.state_dict()
    assert sc.SparseConv3dUnet("unet_4", input_nc=5).output_nc == 96
    enc = sc.SparseConv3dEncoder("encoder_4", input_nc=1)
    assert enc.output_nc == 256 and enc.inner_modules[0].nn[0][0].bias is not None
    w = net.down_modules[2].blocks[0].block[0].kernel  # kaiming-normal, fan_out, relu
    fan_out = torch.nn.init._calculate_fan_in_and_fan_out(w)[1]
    assert float(w.detach().std()) == pytest.approx((2.0 / fan_out) ** 0.5, rel=0.1)
    assert all(float(m.bn.weight.min()) == 1.0 and float(m.bn.bias.abs().max()) == 0.0
               for m in net.modules() if isinstance(m, sc.BatchNorm))


def test_abi_table_has_the_sparse_entry_points():
    from torch_points3d_amd import _lib
    text = open(os.path.join(ROOT, "include", "tp3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tp3d_sparse_set_build_i32", "tp3d_sparse_kmap_i32", "tp3d_sparse_kmap_mirror_i32", "tp3d_sparse_conv_f32",
                 "tp3d_sparse_wgrad_f32"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, name
        assert len(_lib.SIGNATURES[name]) == decl.group(1).count(",") + 1, name
        assert hasattr(_lib.load(), name)
    h = _lib.load()
    assert h.tp3d_sparse_wgrad_chunks(1000, 27, 32, 32) == 1 and h.tp3d_sparse_wgrad_workspace_floats(1000, 27, 32, 32) == 0
    assert h.tp3d_sparse_wgrad_chunks(3000, 27, 32, 32) == 3
    assert h.tp3d_sparse_wgrad_chunks(10 ** 6, 27, 32, 32) <= 32


@pytest.mark.parametrize("tag", ["resblock", "resblock_t", "bottleneck", "down", "up", "chain"])
def test_restatement_reproduces_the_fixture(tag):
    """the fixture is the reference's own blocks over dense stand-ins; the restatement's blocks must give the same"""
    import numpy as np
    import sparseconv_golden_util as gu
    for dtype, pre, tol in ((torch.float32, "", 2e-5), (torch.float64, "f64/", 1e-11)):
        m, x, out, g = gu.run(tag, ref, ref.RefTensor, dtype=dtype)
        as_t = lambda v: torch.as_tensor(v)  # noqa: E731
        assert torch.equal(out.C, g["out_coords"])
        torch.testing.assert_close(out.F.detach(), as_t(g[pre + "out"]), rtol=tol, atol=tol)
        scale = max(1.0, float(as_t(g[pre + "grad_x"]).abs().max()))
        torch.testing.assert_close(x.grad, as_t(g[pre + "grad_x"]), rtol=tol * 10, atol=tol * scale)
        names = [k for k in g if k.startswith("pgrad/")]
        assert len(names) == len(list(m.parameters())) > 0
        for k, p in m.named_parameters():
            want = as_t(g[pre + "pgrad/" + k])
            torch.testing.assert_close(p.grad, want, rtol=tol * 10, atol=tol * max(1.0, float(want.abs().max())))
        if dtype == torch.float32:
            for k, v in m.state_dict().items():
                if "running_" in k:
                    torch.testing.assert_close(v, g["after/" + k], rtol=1e-5, atol=1e-6)
    assert isinstance(g["f64/out"], np.ndarray)


def test_project_blocks_load_the_fixture_state_and_widths_equal_the_json():
    import json
    import sparseconv_golden_util as gu
    from torch_points3d_amd import sparseconv as sc
    for tag in gu.CASES:
        g = gu.case(tag)
        m = gu.build(tag, sc)
        want = {k[len("state/"):]: tuple(v.shape) for k, v in g.items() if k.startswith("state/")}
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want, tag
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "sparseconv_config.json")))
    for name in ("unet_2", "unet_4", "encoder_2", "encoder_4"):
        mine = sc.sparseconv3d_config(name, "FEAT")
        for part in ("down_conv", "up_conv"):
            if part in cfg[name]:
                for key in ("N", "kernel_size", "stride", "block", part + "_nn"):
                    assert mine[part][key] == cfg[name][part][key], (name, part, key)
            else:
                assert part not in mine
        if "innermost" in cfg[name]:
            assert mine["innermost"]["nn"] == cfg[name]["innermost"]["nn"]
            assert mine["innermost"]["aggr"] == cfg[name]["innermost"]["aggr"] == "mean"
            assert mine["innermost"]["negative_slope"] == cfg[name]["innermost"]["activation"]["negative_slope"]


# ------------------------------------------------------------------------- the restatement over the whole accepted range
LIM = (1 << 18) - 1


def test_lookup_is_exact_over_the_accepted_range():
    """a fixed 2^20 radix wraps at batch 16 (16 * 2^60 = 2^64); rows are compared instead, so batches 0, 16 and 511 at one
    (x, y, z) stay three voxels, also next to +-(2^18 - 1) on every axis (66 bits of range: no int64 packing fits)"""
    near = torch.tensor([[1, 2, 3, 0], [1, 2, 3, 16], [1, 2, 3, 511], [1, 2, 4, 16]]).int()
    wide = torch.cat([near, torch.tensor([[LIM, LIM, LIM, 511], [-LIM, -LIM, -LIM, 0], [-LIM, LIM, -LIM, 16],
                                          [LIM - 1, LIM, LIM, 511], [-LIM, -LIM, -LIM + 1, 0]]).int()])
    for C in (near, wide):  # the bounding-box key, and (wide: 2^66 cells) the distinct-row rank
        assert ref.lookup(C, (0, 0, 0), C).tolist() == list(range(len(C)))
        assert ref.lookup(C[:3], (0, 0, 1), C).tolist() == [-1, 3, -1]
        assert ref.lookup(C[3:4], (0, 0, -1), C).tolist() == [1]
    assert ref.lookup(wide, (-1, 0, 0), wide).tolist() == [-1, -1, -1, -1, 7, -1, -1, -1, -1]
    assert ref.lookup(wide, (0, 0, 1), wide).tolist() == [-1, 3, -1, -1, -1, 8, -1, -1, -1]
    assert ref.lookup(wide, (1, 1, 1), wide).tolist() == [-1] * 9  # steps outside +-(2^18 - 1): absent, no wrap onto a row
    # a query set that is not the target set, in another order
    assert ref.lookup(torch.tensor([[-LIM, -LIM, -LIM, 16], [LIM, LIM, LIM - 1, 511], [1, 2, 2, 511]]).int(), (0, 0, 1),
                      wide).tolist() == [-1, 4, 2]
    fwd, inv = ref.kernel_map(wide, wide, 3, 1)
    assert (fwd >= 0).sum(1).tolist() == [1, 2, 1, 2, 2, 2, 1, 2, 2] and torch.equal(inv, fwd.flip(1))


ACCEPTED = [(k, stride, tr) for k in (1, 2, 3) for stride in (1, 2) for tr in (False, True)]


@pytest.mark.parametrize("ts", [1, 2])
@pytest.mark.parametrize("k,stride,transposed", ACCEPTED)
def test_table_convolution_equals_the_dense_one(k, stride, transposed, ts):
    """conv_by_table over kernel_map == the dense grid convolution in float64 to 1e-12 (observed: below 2e-14), for every
    (kernel_size, stride, transposed) the project accepts -- k = 2 at stride 1 in both directions included -- on a cloud
    with negative coordinates, at fine tensor strides 1 and 2"""
    g = torch.Generator().manual_seed(k * 100 + stride * 10 + ts)
    C = torch.unique(torch.cat([torch.randint(-7, 6, (160, 3), generator=g), torch.randint(0, 2, (160, 1), generator=g)], 1),
                     dim=0).int()
    fine = C if ts == 1 else ref.down_coords(C, ts)
    assert int(fine[:, :3].min()) < 0 and len(fine) > 60
    coarse = fine if stride == 1 else ref.down_coords(fine, ts * stride)
    fwd, inv = ref.kernel_map(fine, coarse, k, ts)
    assert int((fwd >= 0).sum()) == int((inv >= 0).sum()) > 0
    C_in, C_out, table = (coarse, fine, inv) if transposed else (fine, coarse, fwd)
    x = torch.randn(len(C_in), 3, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(k ** 3, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
    cot = torch.randn(len(C_out), 5, generator=g, dtype=torch.float64)
    dense = ref.conv(x, C_in, C_out, W, k, stride, ts, transposed)
    want = torch.autograd.grad((dense * cot).sum(), (x, W))
    got = ref.conv_by_table(x, table, W)
    assert got.dtype == torch.float64 and got.shape == (len(C_out), 5)
    torch.testing.assert_close(got, dense, rtol=1e-12, atol=1e-12)
    for a, b in zip(torch.autograd.grad((got * cot).sum(), (x, W)), want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    y32 = ref.conv_by_table(x.detach().float(), table, W.detach().float())
    assert y32.dtype == torch.float32
    torch.testing.assert_close(y32.double(), dense.detach(), rtol=1e-4, atol=1e-4)


def test_coordinate_rule_is_closed_under_flooring():
    """one rule: a voxel [c, c + stride) must hold a coordinate of (-2^18, 2^18).  -(2^18 - 1) floors to -2^18,
    which a stride-2 (and its floor, a stride-4) tensor therefore accepts and a stride-1 tensor does not."""
    from torch_points3d_amd import sparseconv as sc
    C = torch.tensor([[-LIM, LIM, 0, 0], [5, -LIM, LIM, 511]]).int()
    sc.check_coords_host(C, 1)
    C2 = ref.down_coords(C, 2)
    assert C2.tolist() == [[-LIM - 1, LIM - 1, 0, 0], [4, -LIM - 1, LIM - 1, 511]]
    sc.SparseTensor(torch.zeros(2, 1), C2, stride=2)
    C4 = ref.down_coords(C2, 4)
    assert int(C4.min()) == -LIM - 1
    sc.SparseTensor(torch.zeros(2, 1), C4, stride=4)
    with pytest.raises(ValueError, match="out of range"):
        sc.SparseTensor(torch.zeros(2, 1), C2, stride=1)
    for bad, stride in (([-LIM - 3, 0, 0, 0], 2), ([0, LIM + 1, 0, 0], 2), ([0, 0, -LIM - 5, 0], 4), ([0, 0, LIM + 1, 0], 4)):
        with pytest.raises(ValueError, match="out of range"):
            sc.SparseTensor(torch.zeros(1, 1), torch.tensor([bad]).int(), stride=stride)
