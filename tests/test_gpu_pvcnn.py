"""Point-voxel operations and PVCNN on the GPU against the restatement tests/pvcnn_ref.py evaluated in float64 on the device.
Bar (tests/test_gpu_ppnet.py::_close64): |hip - ref64| <= max(atol + rtol |ref64|, 2 |ref32 - ref64|max) with rtol 1e-5
(outputs) / 1e-4 (gradients) and atol = 1e-5 max(1, |ref|max); ref32 is the restatement's own fp32 evaluation.  Integer
tables are compared with torch.equal.  The network is held to the reference's own PVCNN (tests/golden/pvcnn.npz)."""
import pytest
import torch

import pvcnn_ref as pref
from test_gpu_ppnet import _close64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [1, 3, 4, 32, 40, 96]


def _cloud_points():
    """(N, 4) float [x, y, z, batch], two clouds on both sides of 0: shells of radius ~10, 300 points inside one stride-16
    voxel ([2, 14)^3 of cloud 0), two points in every voxel of the cube [-1, 2)^3 (all 8 corners of the inner ones exist),
    isolated points (one corner, one point per voxel) and points on exact integer coordinates; rows shuffled"""
    g = torch.Generator().manual_seed(11)

    def shell(n, radius):
        d = torch.randn(n, 3, generator=g)
        return d / d.norm(dim=1, keepdim=True) * (radius + torch.rand(n, 1, generator=g))

    blob = 2.0 + 12.0 * torch.rand(300, 3, generator=g)
    r = torch.arange(-1, 2).float()
    cells = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    cube = torch.cat([cells + 0.1 + 0.8 * torch.rand(27, 3, generator=g) for _ in range(2)])
    lonely = torch.tensor([[-20.5, -20.25, -20.75], [25.25, 24.5, -22.125], [-23.5, 26.75, 21.5], [22.5, -24.25, 5.5]])
    exact = torch.tensor([[3.0, -2.0, 5.0], [-7.0, -7.0, -7.0], [0.0, 0.0, 0.0]])
    c0 = torch.cat([shell(1500, 10.0), blob, cube, lonely, exact])
    c1 = torch.cat([shell(1100, 8.0), lonely[:1]])
    pc = torch.cat([torch.cat([c0, torch.zeros(len(c0), 1)], 1), torch.cat([c1, torch.ones(len(c1), 1)], 1)])
    return pc[torch.randperm(len(pc), generator=g)].contiguous()


_shared = {}


def _case(s):
    """the points, a target set of tensor stride s that lacks the voxels of some points and has one voxel no point falls
    into, and the restatement's tables; computed once per stride and never modified"""
    if s not in _shared:
        pc = _cloud_points().to(DEV)
        assert 2800 <= len(pc) <= 3200 and len(pc) % 64 != 0
        q = pref.quantize(pc, s)
        full = pref.voxel_set(q)
        keep = torch.ones(len(full), dtype=torch.bool, device=DEV)
        if s == 16:  # (few voxels: two of the isolated points lose theirs)
            keep[pref.lookup1(pref.quantize(pc.new_tensor([[25.25, 24.5, -22.125, 0.0], [-23.5, 26.75, 21.5, 0.0]]), s), full).long()] = False
        else:
            keep[3::17] = False  # some points lose their voxel, many more a corner
        empty = torch.tensor([[48 * s, -48 * s, 48 * s, 1]], dtype=torch.int32, device=DEV)
        Cs = torch.cat([full[keep], empty])
        Cs = Cs[torch.randperm(len(Cs), generator=torch.Generator().manual_seed(s)).to(DEV)].contiguous()
        idx = pref.lookup1(q, Cs)
        idx8 = pref.lookup8(q, s, Cs)
        cnt = pref.counts(idx, len(Cs))
        assert int((idx < 0).sum()) > 0 and int((cnt == 0).sum()) >= 1 and int((cnt == 1).sum()) >= 1
        present = (idx8 >= 0).sum(1)
        assert int(present.max()) == 8 and int(present.min()) <= 1
        _shared[s] = dict(pc=pc, Cs=Cs, idx=idx, idx8=idx8, cnt=cnt)
    return _shared[s]


def _tensors(s, C=1, seed=0):
    from torch_points3d_amd import pvcnn as pv
    from torch_points3d_amd import sparseconv as sc
    c = _case(s)
    g = torch.Generator().manual_seed(1000 * C + s + seed)
    Fp = torch.randn(len(c["pc"]), C, generator=g).to(DEV)
    Fv = torch.randn(len(c["Cs"]), C, generator=g).to(DEV)
    z = pv.PointTensor(Fp.clone().requires_grad_(True), c["pc"].clone())
    x = sc.SparseTensor(Fv.clone().requires_grad_(True), c["Cs"], s)
    return c, z, x, Fp, Fv, g


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("s", [1, 2, 16])
def test_tables_equal_the_restatement(s, nearest):
    from torch_points3d_amd import pvcnn as pv
    c, z, x, _, _, _ = _tensors(s)
    pv.point_to_voxel(x, z)
    pv.voxel_to_point(x, z, nearest=nearest)
    assert torch.equal(z.additional_features["idx_query"][s], c["idx"])
    assert torch.equal(z.additional_features["counts"][s], c["cnt"])
    w64, idx8 = pref.trilinear_weights(c["pc"], c["idx8"], s, torch.float64, nearest)
    w32, _ = pref.trilinear_weights(c["pc"], c["idx8"], s, torch.float32, nearest)
    assert torch.equal(z.idx_query[s], idx8)
    _close64(z.weights[s], w32, w64, 1e-5, 1e-5, floor=1.0, what="weights s%d nearest=%s" % (s, nearest))
    assert float(z.weights[s][idx8 < 0].abs().sum()) == 0.0  # absent corners carry no weight
    # the inverted tables list every present slot once, grouped by voxel row, ascending inside a row
    for key, table in ((("voxelize", s), c["idx"].view(-1, 1)), (("devoxelize", s), idx8)):
        start, order = z.inverted[key][:2]
        flat = table.reshape(-1).long()
        slots = torch.nonzero(flat >= 0).squeeze(1)
        dest, perm = torch.sort(flat[slots], stable=True)
        assert int(start[-1]) == len(slots) and int(start[0]) == 0
        assert torch.equal(order[:len(slots)].long(), slots[perm])
        assert torch.equal(start.long(), torch.searchsorted(dest, torch.arange(len(c["Cs"]) + 1, device=DEV)))


def _inverted_matches_the_restatement(table, Nv):
    from torch_points3d_amd import pvcnn as pv
    start, order = pv._invert(table, Nv)
    flat = table.reshape(-1).long()
    slots = torch.nonzero((flat >= 0) & (flat < Nv)).squeeze(1)
    dest, perm = torch.sort(flat[slots], stable=True)
    assert start.shape == (Nv + 1,) and order.shape == (flat.numel(),)
    assert int(start[-1]) == len(slots) and int(start[0]) == 0
    assert torch.equal(order[:len(slots)].long(), slots[perm])
    assert torch.equal(start.long(), torch.searchsorted(dest, torch.arange(Nv + 1, device=DEV)))
    return start


@pytest.mark.parametrize("Nv", [1, 5])
@pytest.mark.parametrize("N,K", [(1, 1), (1, 8), (256, 1), (257, 1), (32, 8), (33, 8)])
def test_invert_at_block_seams_with_absent_and_out_of_range_slots(N, K, Nv):
    """tp3d_pv_invert_i32 alone: one slot, one workgroup of 256 slots exactly and one slot past it, for both table widths;
    -1 and the out-of-range row Nv + 3 both count as absent."""
    g = torch.Generator().manual_seed(1000 * N + 10 * K + Nv)
    values = torch.tensor([-1] + list(range(Nv)) + [Nv + 3], dtype=torch.int32)
    table = values[torch.randint(0, len(values), (N, K), generator=g)].to(DEV)
    _inverted_matches_the_restatement(table, Nv)


def test_invert_of_a_table_without_a_present_slot():
    start = _inverted_matches_the_restatement(torch.full((33, 8), -1, dtype=torch.int32, device=DEV), 5)
    assert torch.equal(start, torch.zeros(6, dtype=torch.int32, device=DEV))


def test_initial_voxelize_builds_the_voxel_set():
    from torch_points3d_amd import pvcnn as pv
    c = _case(1)
    g = torch.Generator().manual_seed(4)
    Fp = torch.randn(len(c["pc"]), 5, generator=g).to(DEV)
    pos = torch.cat([c["pc"][:, :3] * 0.5, c["pc"][:, 3:]], 1)  # (x * 1.0) / 0.5 gives the test coordinates back exactly
    z = pv.PointTensor(Fp.clone().requires_grad_(True), pos)
    x0 = pv.initial_voxelize(z, 1.0, 0.5)
    assert torch.equal(z.C, c["pc"]) and x0.s == 1
    q = pref.quantize(c["pc"], 1)
    C0 = pref.voxel_set(q)
    idx = pref.lookup1(q, C0)
    assert torch.equal(x0.C, C0) and x0.cmaps[1].n == len(C0)
    assert torch.equal(z.additional_features["idx_query"][1], idx)
    assert torch.equal(z.additional_features["counts"][1], pref.counts(idx, len(C0)))
    cot = torch.randn(len(C0), 5, generator=g).to(DEV)
    (x0.F * cot).sum().backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        f = Fp.detach().to(dt).clone().requires_grad_(True)
        y = pref.voxelize(f, idx, len(C0))
        (y * cot.to(dt)).sum().backward()
        ref[dt] = (y.detach(), f.grad)
    _close64(x0.F, ref[torch.float32][0], ref[torch.float64][0], 1e-5, 1e-5, floor=1.0, what="initial_voxelize")
    _close64(z.F.grad, ref[torch.float32][1], ref[torch.float64][1], 1e-4, 1e-5, floor=1.0, what="initial_voxelize dF")


def _run_hip(s, C):
    from torch_points3d_amd import pvcnn as pv
    c, z, x, Fp, Fv, g = _tensors(s, C)
    cot_v = torch.randn(len(c["Cs"]), C, generator=g).to(DEV)
    cot_p = torch.randn(len(c["pc"]), C, generator=g).to(DEV)
    vox = pv.point_to_voxel(x, z)
    dev = pv.voxel_to_point(x, z)
    assert torch.equal(vox.C, x.C) and vox.s == s and vox.cmaps is x.cmaps and vox.kmaps is x.kmaps
    ((vox.F * cot_v).sum() + (dev.F * cot_p).sum()).backward()
    return c, (Fp, Fv, cot_v, cot_p), (vox.F.detach(), dev.F.detach(), z.F.grad, x.F.grad)


@pytest.mark.parametrize("s", [1, 16])
@pytest.mark.parametrize("C", WIDTHS)
def test_voxelize_and_devoxelize_against_float64(C, s):
    from torch_points3d_amd import pvcnn as pv
    c, (Fp, Fv, cot_v, cot_p), got = _run_hip(s, C)
    if s == 16:  # the piece-wise sum of long runs is taken, by the voxelisation and by the devoxelisation's backward
        assert int(c["cnt"].max()) > pv.LONG_RUN
        assert int(torch.bincount(c["idx8"][c["idx8"] >= 0].long()).max()) > pv.LONG_RUN
    ref = {}
    for dt in (torch.float32, torch.float64):
        fp, fv = (t.detach().to(dt).clone().requires_grad_(True) for t in (Fp, Fv))
        w, _ = pref.trilinear_weights(c["pc"], c["idx8"], s, dt)
        vox = pref.voxelize(fp, c["idx"], len(c["Cs"]))
        dev = pref.devoxelize(fv, c["idx8"], w)
        ((vox * cot_v.to(dt)).sum() + (dev * cot_p.to(dt)).sum()).backward()
        ref[dt] = (vox.detach(), dev.detach(), fp.grad, fv.grad)
    what = "C%d s%d " % (C, s)
    assert float(got[0][c["cnt"] == 0].abs().max()) == 0.0  # a voxel without a point
    for i, (name, rtol) in enumerate([("voxelize", 1e-5), ("devoxelize", 1e-5), ("d points", 1e-4), ("d voxels", 1e-4)]):
        _close64(got[i], ref[torch.float32][i], ref[torch.float64][i], rtol, 1e-5, floor=1.0, what=what + name)


@pytest.mark.parametrize("s", [1, 16])
def test_repeats_are_bit_equal(s):
    a = _run_hip(s, 32)[2]
    b = _run_hip(s, 32)[2]
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_second_call_at_a_stride_reuses_every_table():
    from torch_points3d_amd import pvcnn as pv
    c, z, x, _, _, _ = _tensors(16, 4)
    z1 = pv.voxel_to_point(x, z)
    pv.point_to_voxel(x, z)
    assert z1.idx_query is z.idx_query and z1.weights is z.weights and z1.inverted is z.inverted
    assert z1.additional_features is z.additional_features and z1.C is z.C
    held = (z.idx_query[16], z.weights[16], z.additional_features["idx_query"][16], z.additional_features["counts"][16],
            z.inverted[("voxelize", 16)], z.inverted[("devoxelize", 16)])
    z2 = pv.voxel_to_point(x, z1)  # through the derived tensor
    pv.point_to_voxel(x, z2)
    pv.voxel_to_point(x, z)
    now = (z2.idx_query[16], z2.weights[16], z2.additional_features["idx_query"][16], z2.additional_features["counts"][16],
           z2.inverted[("voxelize", 16)], z2.inverted[("devoxelize", 16)])
    assert all(a is b for a, b in zip(held, now))
    assert sorted(z.idx_query) == [16] and sorted(z.inverted) == [("devoxelize", 16), ("voxelize", 16)]


def test_network_against_the_reference_fixture():
    """the reference's own PVCNN (tests/golden/pvcnn.npz) with the recorded weights: logits, running statistics, input and
    parameter gradients of the train-mode step, then the eval-mode pass -- the bars of the SparseConv3d fixture tests"""
    import pvcnn_golden_util as gu
    from torch_points3d_amd import pvcnn as pv
    cfg, g = gu.config(), gu.load()
    net = pv.pvcnn(cfg["cr"], cfg["vres"], cfg["num_features"], cfg["num_classes"])
    net.dropout.p = 0.0
    x, out = gu.train_step(net, lambda m, f, pos, batch: m(gu.Data(f, pos, batch)), device=DEV)
    assert out.shape == g["out"].shape
    _close64(out, g["out"], g["f64/out"], 1e-5, 1e-5, floor=1.0, what="pvcnn out")
    _close64(x.grad, g["grad_x"], g["f64/grad_x"], 1e-4, 1e-5, floor=1.0, what="pvcnn dX")
    for k, p in net.named_parameters():
        _close64(gu.sample(p.grad), g["pgrad/" + k], g["f64/pgrad/" + k], 1e-4, 1e-5, floor=1.0, what="pvcnn " + k)
    for k, v in net.state_dict().items():
        if "running_" in k:
            torch.testing.assert_close(v.cpu(), g["after/" + k], rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        ev = net.eval()(gu.Data(g["x"].to(DEV), g["pos"].to(DEV), g["batch"].to(DEV)))
    _close64(ev, g["eval/out"], g["f64/eval/out"], 1e-5, 1e-5, floor=1.0, what="pvcnn eval out")
