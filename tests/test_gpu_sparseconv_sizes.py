"""Sparse voxel convolution past the shapes of tests/test_gpu_sparseconv.py: even kernels at stride 1 and transposed, widths
that are no multiple of 4 or step one past a staging size, misaligned features, tensor strides above 1 at the kernel
level, the weight gradient with more than 1024 rows per chunk, a set build that loops over its capped grid, the edges of
the accepted coordinate range, the rejections next to them, and the bias.

Bar: tests/test_gpu_ppnet.py::_close64 unchanged -- |hip - ref64| <= max(atol + rtol |ref64|, 2 |ref32 - ref64|max), rtol
1e-5 (outputs) / 1e-4 (gradients), atol = 1e-5 max(1, |ref|max) -- against the restatement tests/sparseconv_ref.py in
float64, its own fp32 run as the noise floor: the dense grid convolution where the cloud fits a grid, `conv_by_table` over
`kernel_map` (equal to the dense one to 1e-12, tests/test_sparseconv_cpu.py) where it does not.  Tables and coordinate
sets: torch.equal.  Every test asserts the precondition that puts it on the path it is about."""
import pytest
import torch

import sparseconv_ref as ref
from test_gpu_ppnet import _close64
from test_gpu_sparseconv import DEV, _cloud_coords, _module

pytestmark = pytest.mark.gpu
LIM = (1 << 18) - 1


@pytest.fixture(scope="module")
def coords():
    return _cloud_coords().to(DEV)


def _tensor(x, C, ts, k, stride, transposed):
    """the tensor a (k, stride, transposed) convolution receives when its fine set is C at tensor stride ts; a transposed
    stride-2 one sits on the coarse set with what the encoder's forward convolution left in the cache"""
    from torch_points3d_amd import sparseconv as sc
    if transposed and stride == 2:
        st = sc.SparseTensor(torch.zeros(len(C), 1, device=DEV), C, stride=ts)
        st._kmap(k, ts, 2)
        return sc.SparseTensor(x, st.cmaps[2 * ts].coords, 2 * ts, st.cmaps, st.kmaps)
    return sc.SparseTensor(x, C, stride=ts)


def _to_dev(t):
    return t.to(DEV)


def _one_float_in(t):
    """a contiguous view of t's shape that starts one float into a larger buffer"""
    buf = torch.zeros(t.numel() + 4, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _check(C, ts, k, stride, transposed, cin, cout, what, place=_to_dev, by_table=False):
    """one convolution whose fine set is C at tensor stride ts: output set and stride, both tables against
    ref.kernel_map, y / dX / dW against the restatement (dense, or by_table for clouds no grid holds)"""
    coarse = C if stride == 1 else ref.down_coords(C, ts * stride).to(DEV)
    C_in, C_out = (coarse, C) if transposed else (C, coarse)
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = place(torch.randn(len(C_in), cin, generator=g))
    cot = place(torch.randn(len(C_out), cout, generator=g))
    m = _module(k, stride, transposed, cin, cout)
    xh = x.requires_grad_(True)
    st = _tensor(xh, C, ts, k, stride, transposed)
    out = m(st)
    out.F.backward(cot)
    assert torch.equal(out.C, C_out) and out.s == (ts if (stride == 1 or transposed) else ts * stride)
    fwd, inv = ref.kernel_map(C, coarse, k, ts)
    km = st.kmaps.get((k, ts, stride))
    if km is None:  # only the rows GEMM of kernel_size 1 builds no map
        assert k == 1 and stride == 1 and cin % 4 == 0 and cout % 4 == 0
    else:
        assert torch.equal(km.forward, fwd) and torch.equal(km.inverse, inv)
    table = inv if transposed else fwd
    r = {}
    for dtype in (torch.float64, torch.float32):
        Wr = m.kernel.detach().to(dtype).requires_grad_(True)
        xr = x.detach().to(dtype).requires_grad_(True)
        with torch.backends.cudnn.flags(enabled=False):
            y = ref.conv_by_table(xr, table, Wr) if by_table else ref.conv(xr, C_in, C_out, Wr, k, stride, ts, transposed)
            y.backward(cot.to(dtype))
        r[dtype] = (y.detach(), xr.grad, Wr.grad)
    r32, r64 = r[torch.float32], r[torch.float64]
    _close64(out.F, r32[0], r64[0], 1e-5, 1e-5, floor=1.0, what=what + " y")
    _close64(xh.grad, r32[1], r64[1], 1e-4, 1e-5, floor=1.0, what=what + " dX")
    _close64(m.kernel.grad, r32[2], r64[2], 1e-4, 1e-5, floor=1.0, what=what + " dW")
    return out.F.detach(), xh.grad, m.kernel.grad, st


def _name(k, stride, transposed, cin, cout, ts=1):
    return "k%d s%d%s ts%d %dx%d" % (k, stride, " T" if transposed else "", ts, cin, cout)


# ------------------------------------------------------------------------------------------------------ missing shapes
@pytest.mark.parametrize("cin,cout", [(3, 32), (32, 32), (40, 24)])
@pytest.mark.parametrize("k,stride,transposed", [(2, 2, True), (2, 1, False), (2, 1, True), (1, 1, True)])
def test_even_and_transposed_shapes(coords, k, stride, transposed, cin, cout):
    """ResNetUp's default (k = 2, stride 2, transposed), and k = 2 at stride 1: the one same-set map whose inverse table is
    a second search with sign -1, not the mirrored forward table"""
    st = _check(coords, 1, k, stride, transposed, cin, cout, _name(k, stride, transposed, cin, cout))[3]
    if k == 2:
        km = st.kmaps[(2, 1, stride)]
        assert km.K == 8 and int((km.forward >= 0).sum()) == int((km.inverse >= 0).sum())
        if stride == 1:
            assert not torch.equal(km.inverse, km.forward.flip(1))  # (no mirror symmetry for offsets {0, 1})


# ---------------------------------------------------------------------------------------------------------- odd widths
ODD = [(6, 32), (7, 13), (5, 5), (33, 65), (65, 33), (32, 6)]


@pytest.mark.parametrize("cin,cout", ODD)
@pytest.mark.parametrize("k,stride,transposed", [(3, 1, False), (3, 2, False), (3, 2, True)])
def test_odd_widths_take_the_scalar_gather(coords, k, stride, transposed, cin, cout):
    """Cin > 4 and Cin % 4 != 0 is the scalar gather of the MFMA kernel (forward for an odd cin, dX for an odd cout); 33
    steps past the 32-channel LDS stage, 65 past the 64-column tile and the 64-channel weight-gradient tile, 5 / 6 / 13
    stay below one 16-column MFMA block"""
    assert (cin > 4 and cin % 4) or (cout > 4 and cout % 4)
    _check(coords[:700].contiguous(), 1, k, stride, transposed, cin, cout, _name(k, stride, transposed, cin, cout))


@pytest.mark.parametrize("cin,cout", [(6, 13), (33, 32)])
def test_kernel_size_one_at_odd_widths_is_a_one_offset_gather(coords, cin, cout):
    st = _check(coords[:700].contiguous(), 1, 1, 1, False, cin, cout, _name(1, 1, False, cin, cout))[3]
    assert st.kmaps[(1, 1, 1)].K == 1  # (the rows GEMM builds no map)


# ------------------------------------------------------------------------------------------------- misaligned features
@pytest.mark.parametrize("k,stride,transposed", [(3, 1, False), (3, 2, False), (3, 2, True)])
def test_features_one_float_off_alignment(coords, k, stride, transposed):
    """x (N, 32) and the cotangent (., 24) are contiguous views 4 bytes past a 16-byte boundary (_one_float_in asserts
    it): float4 rows are impossible, the kernel must take the scalar gather.  Both gathers feed the same MFMA in the same
    order, so the run on aligned copies gives the same bits."""
    off = _check(coords, 1, k, stride, transposed, 32, 24, "misaligned " + _name(k, stride, transposed, 32, 24), _one_float_in)
    on = _check(coords, 1, k, stride, transposed, 32, 24, "aligned " + _name(k, stride, transposed, 32, 24))
    for a, b, what in zip(off[:3], on[:3], ("y", "dX", "dW")):
        assert torch.equal(a, b), what


# ----------------------------------------------------------------------------------------------- coarse tensor strides
@pytest.mark.parametrize("cin,cout", [(32, 32), (6, 32)])
@pytest.mark.parametrize("k,stride,transposed", [(3, 1, False), (3, 2, False), (2, 2, False), (3, 2, True), (2, 2, True)])
def test_tensor_stride_two_at_the_kernel_level(coords, k, stride, transposed, cin, cout):
    """SparseTensor(x, C2, stride=2): offsets are {-2, 0, 2} / {0, 2}, a stride-2 convolution floors to multiples of 4
    (negative coordinates: floor, not truncation) and a transposed one returns from tensor stride 4 to 2"""
    C2 = ref.down_coords(coords, 2).to(DEV)
    assert int(C2[:, :3].min()) < 0 and int((C2[:, :3] % 4 != 0).sum()) > 0
    out_c = _check(C2, 2, k, stride, transposed, cin, cout, _name(k, stride, transposed, cin, cout, 2))[3]
    if stride == 2:
        assert torch.equal(out_c.cmaps[4].coords, ref.down_coords(C2, 4).to(DEV))


# ----------------------------------------------------------------------------------- weight gradient past 32 chunks
def _solid(lo, hi, seed):
    """every voxel of [lo, hi)^3 in two clouds, rows shuffled"""
    r = torch.arange(lo, hi)
    g = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    C = torch.cat([torch.cat([g, torch.full((len(g), 1), b, dtype=torch.long)], 1) for b in (0, 1)]).int()
    return C[torch.randperm(len(C), generator=torch.Generator().manual_seed(seed))].contiguous()


@pytest.fixture(scope="module")
def block26():
    C = _solid(-13, 13, 7)
    assert len(C) == 35152
    return C.to(DEV)


@pytest.mark.parametrize("n", [32768, 32769, 35152])
def test_weight_gradient_chunks_longer_than_1024_rows(block26, n):
    """N > 32 * 1024: 32 chunks of ceil(N / 32) rows rounded up to 32 (1024, 1056, 1120 here), the last one partial"""
    from torch_points3d_amd import _lib
    h = _lib.load()
    assert h.tp3d_sparse_wgrad_chunks(n, 27, 8, 16) == 32
    assert h.tp3d_sparse_wgrad_workspace_floats(n, 27, 8, 16) == 32 * 27 * 8 * 16
    C = block26[:n].contiguous()
    dw = _check(C, 1, 3, 1, False, 8, 16, "wgrad N=%d" % n)[2]
    assert int((dw.abs().amax((1, 2)) > 0).sum()) == 27  # (a solid block: every offset contributes)
    if n == 35152:
        _check(C, 1, 3, 2, False, 8, 16, "wgrad N=%d s2" % n)


# ------------------------------------------------------------------------------------------ set build past the grid cap
def test_set_build_loops_over_its_capped_grid():
    """the bounding-box pass runs at most 1024 blocks of 256 rows; N = 2 * 52^3 = 281216 makes its grid-stride loop take a
    second turn.  Low corner -27: negative and odd.  Tables only, one feature column."""
    from torch_points3d_amd import sparseconv as sc
    C = _solid(-27, 25, 11).to(DEV)
    assert len(C) == 281216 > 1024 * 256 and int(C[:, :3].min()) == -27
    st = sc.SparseTensor(torch.zeros(len(C), 1, device=DEV), C)
    C2 = ref.down_coords(C, 2).to(DEV)
    assert len(C2) == 2 * 27 ** 3  # -28 .. 24
    for k, stride in ((3, 1), (3, 2), (2, 2)):
        km = st._kmap(k, 1, stride)
        C_out = C if stride == 1 else C2
        assert torch.equal(st.cmaps[stride].coords, C_out)
        fwd, inv = ref.kernel_map(C, C_out, k, 1)
        assert torch.equal(km.forward, fwd), (k, stride)
        assert torch.equal(km.inverse, inv), (k, stride)
    assert int((st.kmaps[(3, 1, 1)].forward >= 0).sum(1).max()) == 27


# --------------------------------------------------------------------------------------------------------- range edges
def _edge_cloud():
    """3^3 clumps in the corners of x, y in {-(2^18 - 1), 2^18 - 1}, z in [-512, 511], one at the origin; batches 0, 16, 511
    (the first and sixth clump share their (x, y, z)); 189 voxels, rows shuffled.  Returns (C, rows of the clump centres)."""
    centres = [(-LIM + 1, -LIM + 1, -511, 0), (LIM - 1, -LIM + 1, 510, 0), (-LIM + 1, LIM - 1, 510, 16), (LIM - 1, LIM - 1, -511, 16),
               (0, 0, 0, 16), (-LIM + 1, -LIM + 1, -511, 511), (LIM - 1, LIM - 1, 510, 511)]
    cube = torch.stack(torch.meshgrid(*([torch.arange(-1, 2)] * 3), indexing="ij"), -1).reshape(-1, 3)
    C = torch.cat([torch.cat([cube + torch.tensor(c[:3]), torch.full((27, 1), c[3])], 1) for c in centres]).int()
    perm = torch.randperm(len(C), generator=torch.Generator().manual_seed(13))
    C = C[perm].contiguous()
    want = torch.tensor(centres).int()
    centre_rows = [int(torch.nonzero((C == w).all(1))[0, 0]) for w in want]
    return C, centre_rows


def test_range_edges_stride_one():
    """voxels at +-(2^18 - 1): a span of 2^19 * 2^19 * 2^10 * 2^9 = 2^57 cells, keys far past 32 bits, batch 511; offsets
    of the outermost voxels step outside the set's bounding box.  No grid holds this cloud: the reference is
    conv_by_table over the restatement's row-exact kernel_map."""
    C, centre_rows = _edge_cloud()
    assert len(C) == 189 and int(C[:, :2].max()) == LIM and int(C[:, :2].min()) == -LIM
    assert int(C[:, 2].min()) == -512 and int(C[:, 2].max()) == 511 and sorted(set(C[:, 3].tolist())) == [0, 16, 511]
    st = _check(C.to(DEV), 1, 3, 1, False, 6, 16, "range edges k3 s1 6x16", by_table=True)[3]
    fwd = st.kmaps[(3, 1, 1)].forward.cpu()
    assert (fwd[centre_rows] >= 0).sum(1).tolist() == [27] * 7
    lo, hi = C[:, :3].min(0).values, C[:, :3].max(0).values
    offs = torch.tensor(ref.offsets(3, 1))
    q = C[:, None, :3] + offs[None]  # (N, 27, 3)
    outside = ((q < lo) | (q > hi)).any(2)
    assert int(outside.sum()) > 0 and bool((fwd[outside] == -1).all())
    print("range edges: %d of %d entries present, %d step outside the box" % (int((fwd >= 0).sum()), fwd.numel(), int(outside.sum())))


def test_range_edges_down_twice_and_back():
    """stride 2 (k = 3), stride 2 again (k = 2) and both transposed steps back on the edge cloud.  -(2^18 - 1) floors to
    -2^18 in the stride-2 set: the second down-convolution builds its set from that coordinate, which the range rule
    accepts at a tensor stride above 1 (before the rule was stated per stride this raised "out of range")."""
    from torch_points3d_amd import sparseconv as sc
    C = _edge_cloud()[0].to(DEV)
    C2 = ref.down_coords(C, 2).to(DEV)
    C4 = ref.down_coords(C2, 4).to(DEV)
    assert int(C2[:, :2].min()) == -LIM - 1 and int(C4[:, :2].min()) == -LIM - 1 and int(C4[:, 3].max()) == 511
    widths = [(3, 2, False, 6, 16), (2, 2, False, 16, 8), (2, 2, True, 8, 16), (3, 2, True, 16, 6)]
    mods = [_module(k, s, t, ci, co, seed=i) for i, (k, s, t, ci, co) in enumerate(widths)]
    g = torch.Generator().manual_seed(17)
    x = torch.randn(len(C), 6, generator=g).to(DEV)
    cot = torch.randn(len(C), 6, generator=g).to(DEV)
    xh = x.clone().requires_grad_(True)
    st = sc.SparseTensor(xh, C)
    outs = [st]
    for m in mods:
        outs.append(m(outs[-1]))
    outs[-1].F.backward(cot)
    for o, (want, s) in zip(outs[1:], ((C2, 2), (C4, 4), (C2, 2), (C, 1))):
        assert torch.equal(o.C, want) and o.s == s
    f1, i1 = ref.kernel_map(C, C2, 3, 1)
    f2, i2 = ref.kernel_map(C2, C4, 2, 2)
    for key, (f, i) in (((3, 1, 2), (f1, i1)), ((2, 2, 2), (f2, i2))):
        assert torch.equal(st.kmaps[key].forward, f) and torch.equal(st.kmaps[key].inverse, i), key
    assert sorted(st.kmaps) == [(2, 2, 2), (3, 1, 2)] and sorted(st.cmaps) == [1, 2, 4]
    r = {}
    for dtype in (torch.float64, torch.float32):
        Ws = [m.kernel.detach().to(dtype).requires_grad_(True) for m in mods]
        xr = x.to(dtype).requires_grad_(True)
        y = xr
        for table, W in zip((f1, f2, i2, i1), Ws):
            y = ref.conv_by_table(y, table, W)
        y.backward(cot.to(dtype))
        r[dtype] = [y.detach(), xr.grad] + [W.grad for W in Ws]
    got = [outs[-1].F, xh.grad] + [m.kernel.grad for m in mods]
    names = ["y", "dX", "dW1", "dW2", "dW3", "dW4"]
    for a, b32, b64, name in zip(got, r[torch.float32], r[torch.float64], names):
        _close64(a, b32, b64, 1e-5 if name == "y" else 1e-4, 1e-5, floor=1.0, what="range edges chain " + name)


# ---------------------------------------------------------------------------------------------------------- rejections
def test_rejections_at_the_range_edges():
    from torch_points3d_amd import sparseconv as sc
    m = _module(3, 1, False, 4, 8)

    def run(rows, stride=1):
        C = torch.tensor(rows).int().to(DEV)
        return m(sc.SparseTensor(torch.zeros(len(C), 4, device=DEV), C, stride=stride))

    # (2^19 - 1)^3 * 512 cells: past the 64-bit key
    with pytest.raises(ValueError, match="span"):
        run([[-LIM, -LIM, -LIM, 0], [LIM, LIM, LIM, 511]])
    with pytest.raises(ValueError, match="out of range"):
        run([[0, 0, 0, 0], [1, 2, 3, 512]])
    # the range rule on the device is the host's (tests/test_sparseconv_cpu.py): -2^18 only at a tensor stride above 1
    with pytest.raises(ValueError, match="out of range"):
        run([[0, 0, 0, 0], [-LIM - 1, 2, 4, 1]])
    assert run([[0, 0, 0, 0], [-LIM - 1, 2, 4, 1]], stride=2).F.shape == (2, 8)
    with pytest.raises(ValueError, match="out of range"):
        run([[0, 0, 0, 0], [-LIM - 3, 2, 4, 1]], stride=2)
    assert run([[-LIM, -LIM, 0, 0], [LIM, LIM, 0, 511]]).F.shape == (2, 8)  # the widest accepted (x, y) box with every batch


# ---------------------------------------------------------------------------------------------------------------- bias
@pytest.mark.parametrize("transposed", [False, True])
def test_bias_is_added_and_its_gradient_is_the_column_sum(coords, transposed):
    from torch_points3d_amd import sparseconv as sc
    C = coords[:700].contiguous()
    k, stride = (3, 2) if transposed else (3, 1)
    cls = sc.Conv3dTranspose if transposed else sc.Conv3d
    torch.manual_seed(4)
    mb = cls(6, 13, kernel_size=k, stride=stride, bias=True).to(DEV)
    m0 = cls(6, 13, kernel_size=k, stride=stride).to(DEV)
    with torch.no_grad():
        mb.kernel.normal_(0, 0.2)
        mb.bias.normal_(0, 1.0)
        m0.kernel.copy_(mb.kernel)
    assert m0.bias is None and mb.bias.shape == (13,) and "bias" in mb.state_dict()
    n_in = len(ref.down_coords(C, 2)) if transposed else len(C)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n_in, 6, generator=g).to(DEV)
    cot = torch.randn(len(C), 13, generator=g).to(DEV)
    res = []
    for m in (mb, m0):
        xh = x.clone().requires_grad_(True)
        out = m(_tensor(xh, C, 1, k, stride, transposed))
        out.F.backward(cot)
        res.append((out.F.detach(), xh.grad, m.kernel.grad))
    assert torch.equal(res[0][0], res[1][0] + mb.bias.detach())
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    _close64(mb.bias.grad, cot.sum(0), cot.double().sum(0), 1e-5, 1e-5, floor=1.0, what="bias gradient" + (" T" if transposed else ""))
