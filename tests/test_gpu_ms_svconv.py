"""MS-SVConv on the GPU: kernel maps and convolutions of kernel_size 5 (the wide first-layer kernels and the generic route),
the multi-scale fusion, the voxelisation and the models, against float64 and the reference-generated fixture
(tests/golden/README_ms_svconv.md).

Bar (tests/test_gpu_ppnet.py::_close64, rtol 1e-5, atol 1e-5 max(1, |ref64|max)):
    |hip - ref64| <= max(1e-5 max(1, |ref64|max) + 1e-5 |ref64|, 2 |ref32 - ref64|max)
ref32 is the fp32 torch evaluation of the same formula (tests/ms_svconv_ref.py)."""
import pytest
import torch

import ms_svconv_ref as ref
from test_gpu_ppnet import _close64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K5 = 125


def _bar(got, ref32, ref64, what):
    _close64(got, ref32, ref64, 1e-5, 1e-5, floor=1.0, what=what)


# ----------------------------------------------------------------------------------------------------------- kernel map
def _brute_table(Cq, Cs, k, ts, sign):
    """host dictionary lookup: row of Cs at Cq + sign * offset"""
    rows = {tuple(c): i for i, c in enumerate(Cs.tolist())}
    offs = ref.offsets(k, ts)
    return torch.tensor([[rows.get((x + sign * o[0], y + sign * o[1], z + sign * o[2], b), -1) for o in offs]
                         for x, y, z, b in Cq.tolist()], dtype=torch.int32)


def _small_voxels():
    g = torch.Generator().manual_seed(11)
    r = torch.arange(-4, 5)
    grid = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    a = grid[torch.randperm(len(grid), generator=g)[:60]]
    b = grid[torch.randperm(len(grid), generator=g)[:50]]
    C = torch.cat([torch.cat([a, torch.zeros(60, 1, dtype=torch.long)], 1), torch.cat([b, torch.ones(50, 1, dtype=torch.long)], 1)])
    assert len(C) == 110 and int(C[:, :3].min()) < 0
    return C.int()


@pytest.mark.parametrize("ts", [1, 2])
def test_kernel_map_k5_equals_brute_force(ts):
    from torch_points3d_amd import sparseconv as sc
    C = _small_voxels()
    C[:, :3] *= ts
    st = sc.SparseTensor(torch.zeros(len(C), 1, device=DEV), C.to(DEV), stride=ts)
    km = st._kmap(5, ts, 1)
    assert km.forward.shape == (110, K5)
    fwd = _brute_table(C, C, 5, ts, 1)
    assert torch.equal(km.forward.cpu(), fwd)
    assert torch.equal(km.inverse.cpu(), _brute_table(C, C, 5, ts, -1))  # the mirrored table = the search from the other side
    assert torch.equal(km.inverse.cpu(), fwd.flip(1))
    assert bool((km.forward[:, 62] == torch.arange(110, device=DEV)).all())  # the centre offset is the row itself


# -------------------------------------------------------------------------------------------------- wide convolution, k = 5
def _with_batch(xyz, b):
    return torch.cat([xyz, torch.full((len(xyz), 1), b, dtype=torch.long)], 1)


def _block():
    r = torch.arange(0, 7)
    return _with_batch(torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) - 3, 0)  # solid 7^3


def _isolated():
    r = torch.arange(0, 24, 6)
    g = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)[:40]
    return _with_batch(g + torch.tensor([8, -12, -12]), 0)  # six apart: the centre offset only


def _sheet():
    g = torch.Generator().manual_seed(4)
    r = torch.arange(-10, 10)
    xy = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2)
    z = torch.round(2.5 * torch.sin(xy[:, 0].float() / 3.0) + 1.5 * torch.cos(xy[:, 1].float() / 2.0)
                    + 0.8 * torch.randn(len(xy), generator=g)).long()
    return _with_batch(torch.cat([xy, z.unsqueeze(1)], 1), 1)


def _shuffled(C, seed):
    return C[torch.randperm(len(C), generator=torch.Generator().manual_seed(seed))].int().contiguous()


@pytest.fixture(scope="module")
def cloud():
    C = _shuffled(torch.cat([_block(), _isolated(), _sheet()]), 6)
    assert len(torch.unique(C, dim=0)) == len(C) == 343 + 40 + 400
    return C.to(DEV)


class _Calls(object):
    """names of the C-ABI entry points called inside the block"""

    def __enter__(self):
        from torch_points3d_amd import _lib
        self.names = []
        self.prev = _lib.set_post_call_hook(lambda name, args: self.names.append(name))
        return self.names

    def __exit__(self, *exc):
        from torch_points3d_amd import _lib
        _lib.set_post_call_hook(self.prev)
        return False


def _layer(cin, cout, seed=0):
    from torch_points3d_amd import sparseconv as sc
    torch.manual_seed(seed)
    m = sc.WideConv3d(cin, cout, kernel_size=5)
    with torch.no_grad():
        m.kernel.normal_(0, 0.2)
    return m.to(DEV)


def _run_k5(C, cin, cout, route, monkeypatch, what, ts=1, need_dx=False, seed=0):
    """one WideConv3d(kernel_size 5) on coordinates C: forward, dW (and dX) against the dense float64 definition and the
    float64 table sum; returns (y, dW, dX, names of the entry points called)"""
    from torch_points3d_amd import sparseconv as sc
    monkeypatch.setattr(sc, "WIDE_ROUTE", route)
    g = torch.Generator().manual_seed(cin * 1000 + cout + seed)
    x = torch.randn(len(C), cin, generator=g).to(DEV)
    cot = torch.randn(len(C), cout, generator=g).to(DEV)
    m = _layer(cin, cout)
    xh = x.clone().requires_grad_(need_dx)
    with _Calls() as names:
        out = m(sc.SparseTensor(xh, C, stride=ts))
        (out.F * cot).sum().backward()
    assert torch.equal(out.C, C) and out.s == ts
    table = ref.kernel_map(C, C, 5, ts)[0]
    res = {}
    for dtype in (torch.float64, torch.float32):
        W = m.kernel.detach().to(dtype).requires_grad_(True)
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        with torch.backends.cudnn.flags(enabled=False):
            y = ref.conv(xr, C, C, W, 5, 1, ts)
        (y * cot.to(dtype)).sum().backward()
        res[dtype] = (y.detach(), W.grad, xr.grad)
        if dtype == torch.float64:  # the dense definition and the table sum are one function
            Wt = m.kernel.detach().double().requires_grad_(True)
            yt = ref.conv_by_table(x.double(), table, Wt)
            (yt * cot.double()).sum().backward()
            assert float((yt - y).detach().abs().max()) <= 1e-12 * max(1.0, float(y.detach().abs().max()))
            assert float((Wt.grad - W.grad).abs().max()) <= 1e-12 * max(1.0, float(W.grad.abs().max()))
    _bar(out.F, res[torch.float32][0], res[torch.float64][0], what + " y")
    _bar(m.kernel.grad, res[torch.float32][1], res[torch.float64][1], what + " dW")
    if need_dx:
        _bar(xh.grad, res[torch.float32][2], res[torch.float64][2], what + " dX")
    return out.F.detach().clone(), m.kernel.grad.clone(), (xh.grad.clone() if need_dx else None), names


WIDE_WIDTHS = [(1, 32), (3, 32), (4, 32), (1, 5), (2, 96)]


@pytest.mark.parametrize("route", ["wide", "generic"])
@pytest.mark.parametrize("cin,cout", WIDE_WIDTHS)
def test_first_layer_k5_against_float64(cloud, cin, cout, route, monkeypatch):
    from torch_points3d_amd import _lib
    h = _lib.load()
    n = len(cloud)
    chunks = h.tp3d_sparse_wgrad_wide_chunks(n, K5, cin, cout)
    assert chunks >= 3 and chunks == (n + 127) // 128 and n % 128 != 0, (n, chunks)  # 128-row chunks, a partial last one
    assert h.tp3d_sparse_wgrad_wide_workspace_floats(n, K5, cin, cout) == chunks * K5 * cin * cout
    _, _, _, names = _run_k5(cloud, cin, cout, route, monkeypatch, "k5 %dx%d %s" % (cin, cout, route))
    wide = route != "generic"
    assert ("tp3d_sparse_conv_wide_f32" in names) == wide and ("tp3d_sparse_wgrad_wide_f32" in names) == wide
    assert ("tp3d_sparse_conv_f32" in names) != wide and ("tp3d_sparse_wgrad_f32" in names) != wide


def test_solid_block_and_isolated_voxels(cloud, monkeypatch):
    """the 27 interior voxels of the 7^3 block have all 125 offsets; voxels six apart have the centre only: y = x W[62]"""
    from torch_points3d_amd import sparseconv as sc
    block = _shuffled(_block(), 1).to(DEV)
    st = sc.SparseTensor(torch.zeros(len(block), 1, device=DEV), block)
    present = (st._kmap(5, 1, 1).forward >= 0).sum(1)
    assert int((present == K5).sum()) == 27 and int(present.min()) == 27
    for cin, cout in ((1, 32), (4, 32)):
        _run_k5(block, cin, cout, "wide", monkeypatch, "block %dx%d" % (cin, cout))
    lone = _shuffled(_isolated(), 2).to(DEV)
    for route in ("wide", "generic"):
        _, dw, _, _ = _run_k5(lone, 3, 32, route, monkeypatch, "isolated " + route)
        assert float(dw[:62].abs().max()) == 0.0 and float(dw[63:].abs().max()) == 0.0 and float(dw[62].abs().max()) > 0.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100, 129])
def test_row_count_seams(cloud, n, monkeypatch):
    """1 row, the 64 rows of a wave pass +- 1, 100 rows (less than one weight-gradient chunk), 129 (one row into the second)"""
    from torch_points3d_amd import _lib
    sheet = _shuffled(_sheet(), 3)[:n].contiguous().to(DEV)
    chunks = _lib.load().tp3d_sparse_wgrad_wide_chunks(n, K5, 4, 32)
    assert chunks == (2 if n == 129 else 1)
    for cin, cout in ((1, 32), (4, 32)):
        _run_k5(sheet, cin, cout, "wide", monkeypatch, "N=%d %dx%d" % (n, cin, cout))


@pytest.mark.parametrize("cin,cout", [(8, 32), (33, 16)])
def test_generic_route_at_k125_with_input_gradient(cloud, cin, cout, monkeypatch):
    """more than four input channels (a pre_mlp_nn in front): the MFMA kernel, the generic weight gradient and dX through the
    mirrored table, whatever WIDE_ROUTE says"""
    _, _, _, names = _run_k5(cloud, cin, cout, "wide", monkeypatch, "generic k125 %dx%d" % (cin, cout), need_dx=True)
    assert "tp3d_sparse_conv_wide_f32" not in names and "tp3d_sparse_wgrad_wide_f32" not in names


def test_narrow_layer_input_gradient_takes_the_generic_kernel(cloud, monkeypatch):
    _, _, dx, names = _run_k5(cloud, 3, 32, "wide", monkeypatch, "k5 3x32 dX", need_dx=True)
    assert dx is not None and names.count("tp3d_sparse_conv_f32") == 1 and names.count("tp3d_sparse_conv_wide_f32") == 1


@pytest.mark.parametrize("cin,cout", [(4, 96), (4, 80)])
def test_declined_shapes_fall_back(cloud, cin, cout, monkeypatch):
    """(4, 96): neither W nor one wave's accumulators fit the LDS; (4, 80): the accumulators of one wave do, W with the hit
    lists of four waves does not"""
    from torch_points3d_amd import _lib
    h = _lib.load()
    assert h.tp3d_sparse_conv_wide_serves(K5, cin, cout) == 0
    served = h.tp3d_sparse_wgrad_wide_chunks(len(cloud), K5, cin, cout) > 0
    assert served == (cout == 80)
    _, _, _, names = _run_k5(cloud, cin, cout, "wide", monkeypatch, "declined %dx%d" % (cin, cout))
    assert "tp3d_sparse_conv_wide_f32" not in names and "tp3d_sparse_conv_f32" in names
    assert ("tp3d_sparse_wgrad_wide_f32" in names) == served


def test_two_calls_are_bit_equal(cloud, monkeypatch):
    for route in ("wide", "generic"):
        a = _run_k5(cloud, 4, 32, route, monkeypatch, "repeat " + route)
        b = _run_k5(cloud, 4, 32, route, monkeypatch, "repeat " + route)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wide_conv_behind_a_stride_2_convolution(cloud, monkeypatch):
    """tensor stride 2: offsets {-4 .. 4} in steps of 2"""
    from torch_points3d_amd import sparseconv as sc
    import sparseconv_ref as sr
    monkeypatch.setattr(sc, "WIDE_ROUTE", "wide")
    torch.manual_seed(3)
    down = sc.Conv3d(3, 4, kernel_size=2, stride=2).to(DEV)
    wide = _layer(4, 32)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(len(cloud), 3, generator=g).to(DEV)
    mid = down(sc.SparseTensor(x, cloud))
    out = wide(mid)
    assert out.s == 2 and torch.equal(out.C, mid.C)
    C2 = sr.down_coords(cloud, 2).to(DEV)
    assert torch.equal(mid.C, C2)
    cot = torch.randn(len(C2), 32, generator=g).to(DEV)
    (out.F * cot).sum().backward()
    res = {}
    for dtype in (torch.float64, torch.float32):
        W1 = down.kernel.detach().to(dtype).requires_grad_(True)
        W2 = wide.kernel.detach().to(dtype).requires_grad_(True)
        with torch.backends.cudnn.flags(enabled=False):
            y = ref.conv(ref.conv(x.to(dtype), cloud, C2, W1, 2, 2, 1), C2, C2, W2, 5, 1, 2)
        (y * cot.to(dtype)).sum().backward()
        res[dtype] = (y.detach(), W1.grad, W2.grad)
    _bar(out.F, res[torch.float32][0], res[torch.float64][0], "ts2 y")
    _bar(down.kernel.grad, res[torch.float32][1], res[torch.float64][1], "ts2 dW down")
    _bar(wide.kernel.grad, res[torch.float32][2], res[torch.float64][2], "ts2 dW wide")


# --------------------------------------------------------------------------------------------------------- scale_fuse
def _fuse_inputs(S, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(N, C, generator=g) * (0.5 + s) for s in range(S)]
    cot = torch.randn(N, S * C, generator=g)
    cots = [torch.randn(N, C, generator=g) for _ in range(S)]
    return xs, cot, cots


def _fuse_ref(xs, mode, cot, cots, dtype):
    xr = [x.detach().clone().to(dtype).requires_grad_(True) for x in xs]
    out, hs = ref.scale_fuse(xr, mode)
    loss = (out * cot.to(dtype)[:, :out.shape[1]]).sum()
    if cots is not None:
        loss = loss + sum((h * c.to(dtype)).sum() for h, c in zip(hs, cots))
    loss.backward()
    return out.detach(), [h.detach() for h in hs], [x.grad for x in xr]


@pytest.mark.parametrize("mode", ["cat", "max", "mean"])
@pytest.mark.parametrize("C", [1, 3, 32, 33])
@pytest.mark.parametrize("S", [1, 3, 4])
def test_scale_fuse_against_float64(S, C, mode):
    from torch_points3d_amd import torchpoints as tp
    for N in (1, 63, 64, 65, 1000):
        xs, cot, cots = _fuse_inputs(S, C, N, S * 100 + C)
        xs, cot, cots = [x.to(DEV) for x in xs], cot.to(DEV), [c.to(DEV) for c in cots]
        for with_scales in (False, True):
            xh = [x.clone().requires_grad_(True) for x in xs]
            if with_scales:
                out, hs = tp.scale_fuse(xh, mode, return_scales=True)
                loss = (out * cot[:, :out.shape[1]]).sum() + sum((h * c).sum() for h, c in zip(hs, cots))
            else:
                out = tp.scale_fuse(xh, mode)
                loss = (out * cot[:, :out.shape[1]]).sum()
            loss.backward()
            r64 = _fuse_ref(xs, mode, cot, cots if with_scales else None, torch.float64)
            r32 = _fuse_ref(xs, mode, cot, cots if with_scales else None, torch.float32)
            what = "fuse S%d C%d N%d %s%s" % (S, C, N, mode, " +scales" if with_scales else "")
            assert out.shape == (N, S * C if mode == "cat" else C)
            _bar(out, r32[0], r64[0], what + " out")
            for s in range(S):
                _bar(xh[s].grad, r32[2][s], r64[2][s], what + " dx%d" % s)
                if with_scales:
                    _bar(hs[s], r32[1][s], r64[1][s], what + " xhat%d" % s)
                    if mode == "cat":  # column views of the output
                        assert hs[s].data_ptr() == out[:, s * C:].data_ptr() and torch.equal(hs[s], out[:, s * C:(s + 1) * C])


@pytest.mark.parametrize("mode", ["cat", "max", "mean"])
def test_scale_fuse_zero_row_and_repeat(mode):
    """an all-zero row: 0 forward, g / eps backward, bit-equal to torch's fp32 result on that row; repeats bit-equal"""
    from torch_points3d_amd import torchpoints as tp
    S, C, N, row = 3, 32, 65, 17
    xs, cot, _ = _fuse_inputs(S, C, N, 5)
    for x in xs:
        x[row] = 0.0
    xs, cot = [x.to(DEV) for x in xs], cot.to(DEV)
    runs = []
    for _ in range(2):
        xh = [x.clone().requires_grad_(True) for x in xs]
        out = tp.scale_fuse(xh, mode)
        (out * cot[:, :out.shape[1]]).sum().backward()
        runs.append([out.detach()] + [x.grad for x in xh])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # torch's fp32 evaluation on the CPU (where max(0) sends a tie to the lowest index)
    out32, _, dx32 = _fuse_ref([x.cpu() for x in xs], mode, cot.cpu(), None, torch.float32)
    assert float(runs[0][0][row].abs().max()) == 0.0 and float(out32[row].abs().max()) == 0.0
    for s in range(S):
        got = runs[0][1 + s][row].cpu()
        assert torch.equal(got, dx32[s][row])
        ch = cot.cpu()  # (the division by S on the host: IEEE, as in the kernel)
        g = ch[row, s * C:(s + 1) * C] if mode == "cat" else (ch[row, :C] / S if mode == "mean" else ch[row, :C] * (s == 0))
        assert torch.equal(got, g / 1e-20)


def test_scale_fuse_max_tie_goes_to_the_lowest_scale():
    """scales 0 and 1 are the same tensor: wherever they beat scale 2 they tie, and scale 1 gets no gradient at all"""
    from torch_points3d_amd import torchpoints as tp
    g = torch.Generator().manual_seed(8)
    a = torch.randn(64, 8, generator=g)
    xs = [a.clone(), a.clone(), a * 0.5 + 0.1]
    cot = torch.randn(64, 8, generator=g)
    xh = [x.to(DEV).requires_grad_(True) for x in xs]
    out, hs = tp.scale_fuse(xh, "max", return_scales=True)
    (out * cot.to(DEV)).sum().backward()
    assert torch.equal(hs[0], hs[1])
    won2 = hs[2] > hs[0]
    assert 0 < int(won2.sum()) < won2.numel()
    assert float(xh[1].grad.abs().max()) == 0.0 and float(xh[0].grad.abs().max()) > 0.0
    # torch's own rule on the CPU: max(0) of equal values returns index 0, so its gradient is the same function
    assert int(torch.stack([a, a], 0).max(0)[1].max()) == 0
    r64 = _fuse_ref(xs, "max", cot, None, torch.float64)
    r32 = _fuse_ref(xs, "max", cot, None, torch.float32)
    for s in range(3):
        _bar(xh[s].grad, r32[2][s], r64[2][s], "tie dx%d" % s)


# ------------------------------------------------------------- voxelisation and models: the reference-generated fixture
import ms_svconv_golden_util as gu  # noqa: E402


class _Data(object):
    def __init__(self, pos, batch, x):
        self.pos, self.batch, self.x = pos, batch, x


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("c", [0, 1])
def test_voxelize_equals_the_reference_tables(c, scale):
    """cluster, unique_pos_indices and coords of the reference's _prepare_data (tests/golden/ms_svconv.npz), both clouds and
    both grid sizes; the three aggregations against float64"""
    from torch_points3d_amd import ms_svconv as ms
    g = gu.load()
    gs = gu.fixture_numbers()[0][scale]
    pos, batch = g["pos%d" % c].to(DEV), g["batch%d" % c].to(DEV)
    t = "tables/cloud%d/scale%d/" % (c, scale)
    gen = torch.Generator().manual_seed(31 + c)
    x = torch.randn(len(pos), 5, generator=gen).to(DEV)
    for aggr in (None, "mean", "max"):
        xh = x.clone().requires_grad_(True)
        v = ms.voxelize(pos, batch, gs, xh, aggr)
        assert torch.equal(v.cluster.cpu(), g[t + "cluster"]) and torch.equal(v.unique_pos_indices.cpu(), g[t + "unique_pos_indices"])
        assert torch.equal(v.coords.cpu(), g[t + "coords"]) and torch.equal(v.batch.cpu(), g[t + "batch"])
        assert len(v.coords) < len(pos)  # a voxel with several points
        cot = torch.randn(v.x.shape, generator=gen).to(DEV)
        (v.x * cot).sum().backward()
        res = {}
        for dtype in (torch.float64, torch.float32):
            xr = x.detach().clone().to(dtype).requires_grad_(True)
            xv = ref.voxelize(pos, batch, gs, xr, aggr)[3]
            (xv * cot.to(dtype)).sum().backward()
            res[dtype] = (xv.detach(), xr.grad)
        _bar(v.x, res[torch.float32][0], res[torch.float64][0], "voxelize %s x" % aggr)
        _bar(xh.grad, res[torch.float32][1], res[torch.float64][1], "voxelize %s dx" % aggr)


@pytest.mark.parametrize("tag", gu.CASES)
def test_fixture_passes(tag):
    """UnetMSparseConv3d, MS_SparseConv3d, MS_SparseConv3d_Shared (intermediate loss, drawn selections replayed),
    MS_SparseConv3d_Shared_Pool (max, mean), MS_SparseConvModel with the reference's weights: outputs, per-scale outputs,
    the loss and its intermediate terms, every parameter gradient OF THAT LOSS, and the running statistics, against the
    reference's fp32 pass and its float64 pass (`f64/`)"""
    g = gu.load()
    got, net = gu.run_hip(tag, g, DEV)
    t = tag + "/"
    for k, v in got.items():
        want64 = g[t + "f64/" + k]
        _bar(v.reshape(want64.shape), g[t + k], want64, "%s %s" % (tag, k))
    assert ("loss" in got or "loss_seg" in got) == (tag != "unet")
    checked = 0
    for name, p in net.named_parameters():
        want64 = g[t + "f64/pgrad/" + name]
        own = float(g[t + "pgrad_own/" + name])  # |the reference's fp32 gradient - its float64 gradient|max
        assert p.grad is not None, name
        _bar(p.grad.reshape(want64.shape), want64 + own, want64, "%s grad %s" % (tag, name))
        checked += 1
    assert checked == sum(1 for k in g if k.startswith(t + "f64/pgrad/"))
    for k, v in net.state_dict().items():
        if "running_" in k:
            _bar(v, g[t + "after/" + k], g[t + "f64/after/" + k], "%s %s" % (tag, k))


def test_full_width_training_step_is_finite_and_repeatable():
    """MS_SVCONV_B2cm_X2_3head on 2 x 2 000 points: finite outputs and gradients, every parameter with a gradient that is not
    all zero, and a second identical step from the same state bit-equal"""
    from torch_points3d_amd import ms_svconv as ms
    g = torch.Generator().manual_seed(70)

    def cloud(n, shift):
        uv = torch.rand(n, 2, generator=g) * 1.5
        p = torch.stack([uv[:, 0], uv[:, 1], 0.2 * torch.sin(4 * uv[:, 0]) * torch.cos(3 * uv[:, 1]) + shift], 1)
        return _Data((p + 0.004 * torch.randn(n, 3, generator=g)).to(DEV), torch.zeros(n, dtype=torch.long, device=DEV),
                     torch.ones(n, 1, device=DEV))

    d0, d1 = cloud(2000, 0.0), cloud(2000, 0.01)
    match = torch.stack([torch.randperm(2000, generator=g)[:500], torch.randperm(2000, generator=g)[:500]], 1).to(DEV)
    sel = dict(sel0=torch.randperm(2000, generator=g)[:256].to(DEV), sel1=torch.randperm(2000, generator=g)[:256].to(DEV))
    torch.manual_seed(71)
    net = ms.build("MS_SVCONV_B2cm_X2_3head").to(DEV).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    runs = []
    for _ in range(2):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        out = net(d0, d1, match, loss_kwargs=sel)
        net.loss.backward()
        assert out.shape == (2000, 32) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(net.loss))
        grads = {}
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            assert float(p.grad.abs().max()) > 0.0, name
            grads[name] = p.grad.clone()
        runs.append((out.detach().clone(), net.loss.detach().clone(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for name in runs[0][2]:
        assert torch.equal(runs[0][2][name], runs[1][2][name]), name
