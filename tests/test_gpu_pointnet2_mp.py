"""Message-passing PointNet++ on the HIP kernels (csrc/fps.hip tp3d_fps_ragged_f32, csrc/pointconv.hip,
torch_points3d_amd/pointnet2_mp.py) against the CPU oracle, the plain-torch statement tests/pointnet2_mp_ref.py, and the
fixture the REFERENCE's own SAModule / GlobalBaseModule / FPModule produced (tests/golden/pointnet2_mp.npz, written by
tests/golden/make_golden_mp.py; see its docstring for what stands in for torch_geometric).

Bars.  Index outputs (samples, edges, argmax) and the copy kernels: torch.equal.  Floating point, as
tests/test_gpu_randla_golden.py writes them: every stage teacher-forced on the fixture's inputs rtol = 1e-5,
atol = bound(out, out64) (1e-5, or twice the reference pass's own distance to its float64 evaluation); the chained
network by its distance to the float64 pass, <= 4x max and <= 2x RMS of the reference pass's own; BatchNorm buffers
rtol 1e-4 / atol 1e-5; eval mode 1e-5 * max(1, scale).  Gradients in relative L2: the larger of 1e-4 and 4x the distance
of the reference's float32 gradients to its float64 gradients, measured when the fixture was made and stored in it
(`grel/*`): 2.4e-6 for the input, 3.4e-6 for the worst parameter, so the 1e-4 floor is the bar everywhere (the max pools
make the gradient piecewise).  None of these figures comes from the code under test."""
import pytest
import torch

from conftest import load_golden
import pointnet2_mp_ref as ref
from randla_golden_util import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_REG = 32768  # TP3D_FPS_MAX_REG_POINTS


@pytest.fixture(scope="module")
def gold():
    return load_golden("pointnet2_mp")


def _oracle_fps(oracle, pos, sizes, quotas):
    out, base = [], 0
    for n, q in zip(sizes, quotas):
        if n and q:
            out.append(oracle.furthest_point_sample(pos[base:base + n].unsqueeze(0), q)[0] + base)
        base += n
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64)


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


# ---------------------------------------------------------------------------------------------------- ragged FPS
RAGGED_SIZES = [65, 1, 4099, 2, 0, 63, 1025, 64, 257]  # id 4 has no point.  ONE template serves the whole batch, picked from
# the largest cloud: <512,16> here; the others are tests/test_gpu_pointnet2_mp_sizes.py's


@pytest.fixture(scope="module")
def ragged_cloud():
    g = torch.Generator().manual_seed(11)
    return torch.rand(sum(RAGGED_SIZES), 3, generator=g) * 2 - 1


@pytest.mark.parametrize("ratio", [0.25, 1.0])
def test_fps_ragged_matches_oracle_cloud_by_cloud(hip, oracle, ragged_cloud, ratio):
    batch = _batch_of(RAGGED_SIZES)
    want = _oracle_fps(oracle, ragged_cloud, RAGGED_SIZES, ref.fps_quota(RAGGED_SIZES, ratio))
    got = hip.fps_ragged(ragged_cloud.to(DEV), batch.to(DEV), ratio=ratio)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)


def test_fps_ragged_small_batches(hip, oracle):
    """largest cloud <= 128 (one wave), the reference's 5-point pin, duplicate points (ties -> lowest index)"""
    pin = torch.tensor([[0, 0, 0], [0.5, 0.5, 0], [0.4, 0.2, 0], [2, 2, 2], [-1, -2, -0.01]]).float()
    got = hip.fps_ragged(pin.to(DEV), torch.zeros(5, dtype=torch.long, device=DEV), ratio=3 / 5.0)
    assert got.cpu().tolist() == [0, 3, 4]
    assert hip.fps_ragged(pin.to(DEV), None, ratio=3 / 5.0).cpu().tolist() == [0, 3, 4]
    # a 4x4x4 lattice stored twice, between two random clouds: every distance is tied many times over
    ax = torch.arange(4.0)
    lattice = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    g = torch.Generator().manual_seed(3)
    sizes = [33, 128, 7]
    pos = torch.cat([torch.rand(33, 3, generator=g), lattice, lattice, torch.rand(7, 3, generator=g)])
    for ratio in (0.5, 1.0):
        want = _oracle_fps(oracle, pos, sizes, ref.fps_quota(sizes, ratio))
        got = hip.fps_ragged(pos.to(DEV), _batch_of(sizes).to(DEV), ratio=ratio)
        assert torch.equal(got.cpu(), want)
    # explicit per-cloud counts, a zero among them; more than a cloud holds is an error
    got = hip.fps_ragged(pos.to(DEV), _batch_of(sizes).to(DEV), counts=[5, 0, 7])
    assert torch.equal(got.cpu(), _oracle_fps(oracle, pos, sizes, [5, 0, 7]))
    with pytest.raises(ValueError):
        hip.fps_ragged(pos.to(DEV), _batch_of(sizes).to(DEV), counts=[5, 0, 8])


def test_fps_ragged_equal_clouds_match_the_dense_kernel(hip):
    g = torch.Generator().manual_seed(5)
    B, N = 3, 300
    pos = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(DEV)
    dense = hip.furthest_point_sample(pos, 75)
    ragged = hip.fps_ragged(pos.reshape(-1, 3), _batch_of([N] * B).to(DEV), ratio=0.25)
    offs = (torch.arange(B, device=DEV) * N).unsqueeze(1)
    assert torch.equal(ragged.view(B, 75), dense + offs)


def test_fps_ragged_scratch_path(hip, oracle):
    """a cloud above TP3D_FPS_MAX_REG_POINTS: the running minimum lives in memory, for every cloud of the batch"""
    g = torch.Generator().manual_seed(9)
    sizes = [100, MAX_REG + 5, 3]
    pos = torch.rand(sum(sizes), 3, generator=g)
    quotas = [10, 40, 3]
    got = hip.fps_ragged(pos.to(DEV), _batch_of(sizes).to(DEV), counts=quotas)
    assert torch.equal(got.cpu(), _oracle_fps(oracle, pos, sizes, quotas))


# ---------------------------------------------------------------------------------------------------- edges, rows
@pytest.fixture(scope="module")
def ragged_edges(oracle):
    """two clouds; the queries are NOT a subset of the support: some have no hit, some are cut at the cap"""
    g = torch.Generator().manual_seed(21)
    sizes, qsizes, cap, radius = [50, 131], [40, 67], 4, 0.45
    pos_s = torch.rand(sum(sizes), 3, generator=g) * 2 - 1
    pos_q = torch.rand(sum(qsizes), 3, generator=g) * 3 - 1.5
    bs, bq = _batch_of(sizes), _batch_of(qsizes)
    table, _ = oracle.ball_query(radius, cap, pos_s, pos_q, mode="partial_dense", batch_x=bs, batch_y=bq)
    edge_start, col = ref.table_edges(table)
    deg = edge_start[1:] - edge_start[:-1]
    assert int((deg == 0).sum()) >= 3 and int((deg == cap).sum()) >= 3 and int(((deg > 0) & (deg < cap)).sum()) >= 3
    return dict(pos_s=pos_s, pos_q=pos_q, bs=bs, bq=bq, cap=cap, radius=radius, edge_start=edge_start, col=col)


def test_radius_edges_match_the_compacted_oracle_table(hip, oracle, gold, ragged_edges):
    c = ragged_edges
    es, col = hip.radius_edges(c["radius"], c["cap"], c["pos_s"].to(DEV), c["pos_q"].to(DEV), c["bs"].to(DEV), c["bq"].to(DEV))
    assert torch.equal(es.cpu(), c["edge_start"]) and torch.equal(col.cpu(), c["col"])
    # a table wider than a wave (two steps of 64 slots), on the same geometry
    es, col = hip.radius_edges(1.5, 100, c["pos_s"].to(DEV), c["pos_q"].to(DEV), c["bs"].to(DEV), c["bq"].to(DEV))
    wes, wcol = ref.table_edges(oracle.ball_query(1.5, 100, c["pos_s"], c["pos_q"], mode="partial_dense", batch_x=c["bs"],
                                                   batch_y=c["bq"])[0])
    assert int((wes[1:] - wes[:-1]).max()) > 64
    assert torch.equal(es.cpu(), wes) and torch.equal(col.cpu(), wcol)
    # the fixture's two levels, through the finder the modules use
    from torch_points3d_amd.pointnet2_mp import MultiscaleRadiusNeighbourFinder
    cfg = ref.GOLD_CFG["down_conv"]
    levels = ((gold["pos"], gold["batch"], gold["sa1/pos"], gold["sa1/batch"]),
              (gold["sa1/pos"], gold["sa1/batch"], gold["sa2/pos"], gold["sa2/batch"]))
    for i, (ps, bs, pq, bq) in enumerate(levels):
        finder = MultiscaleRadiusNeighbourFinder(cfg["radius"][i], cfg["radius_num_points"][i])
        row, col = edges = finder(ps.to(DEV), pq.to(DEV), batch_x=bs.to(DEV), batch_y=bq.to(DEV))
        want_es, want_col = gold["edges/sa%d/edge_start" % (i + 1)], gold["edges/sa%d/col" % (i + 1)]
        assert torch.equal(edges.edge_start.cpu(), want_es) and torch.equal(col.cpu(), want_col)
        assert torch.equal(row.cpu(), torch.repeat_interleave(torch.arange(pq.shape[0]), want_es[1:] - want_es[:-1]))


@pytest.mark.parametrize("C", [0, 1, 4, 35])
def test_pointconv_rows_exact(hip, ragged_edges, C):
    c = ragged_edges
    g = torch.Generator().manual_seed(C)
    x = torch.randn(c["pos_s"].shape[0], C, generator=g) if C else None
    for ld in sorted({C + 3, (C + 3 + 3) & ~3}):
        want = ref.edge_rows(x, c["pos_s"], c["pos_q"], c["edge_start"], c["col"], ld=ld)
        got = hip.pointconv_rows(None if x is None else x.to(DEV), c["pos_s"].to(DEV), c["pos_q"].to(DEV),
                                 c["edge_start"].to(DEV), c["col"].to(DEV), ld=ld)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), ld
    if C:  # gradient wrt x: every edge hands its row's first C columns back to its support row, in edge order
        xg = x.to(DEV).requires_grad_(True)
        rows = hip.pointconv_rows(xg, c["pos_s"].to(DEV), c["pos_q"].to(DEV), c["edge_start"].to(DEV), c["col"].to(DEV))
        cot = torch.randn(rows.shape, generator=g)
        (rows * cot.to(DEV)).sum().backward()
        want = torch.zeros_like(x).index_add_(0, c["col"], cot[:, :C])
        torch.testing.assert_close(xg.grad.cpu(), want, rtol=1e-6, atol=1e-6)


SEG_LENGTHS = [2, 0, 63, 1, 300, 64, 0, 65]


@pytest.mark.parametrize("C", [1, 32, 67])
def test_segment_max_forward_and_backward_exact(hip, C):
    g = torch.Generator().manual_seed(100 + C)
    seg = torch.zeros(len(SEG_LENGTHS) + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.tensor(SEG_LENGTHS), 0)
    E = int(seg[-1])
    for ld in sorted({C, (C + 3) & ~3, C + 5}):
        # eighths: every segment of more than a few rows holds its maximum several times (the first one wins)
        rows = torch.randint(-8, 9, (E, ld), generator=g).float() / 8
        rows[int(seg[4]) + 7] = rows[int(seg[4]) + 3] = 2.0  # an explicit tie inside the 300-row segment
        want, warg = ref.segment_max(rows, seg, C)
        assert int(warg[4, 0]) == int(seg[4]) + 3
        rg = rows.to(DEV).requires_grad_(True)
        out, arg = hip.segment_max(rg, seg.to(DEV), C=C, return_argmax=True)
        assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), warg)
        cot = torch.randn(want.shape, generator=g)
        (out * cot.to(DEV)).sum().backward()
        rc = rows.clone().requires_grad_(True)
        (ref.segment_max(rc, seg, C)[0] * cot).sum().backward()
        assert torch.equal(rg.grad.cpu(), rc.grad), ld
    # continuous values (no ties), as one long segment and as per-row segments
    rows = torch.randn(E, C, generator=g)
    for s in (torch.tensor([0, E]), torch.arange(E + 1)):
        want, warg = ref.segment_max(rows, s)
        out, arg = hip.segment_max(rows.to(DEV), s.to(DEV), return_argmax=True)
        assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), warg)


# ---------------------------------------------------------------------------------------------------- the fixture
def _bag(gold, tag, x=None):
    from torch_points3d_amd.kpconv_blocks import PDData
    if tag == "in":
        pos, batch, xx = gold["pos"], gold["batch"], gold["x"]
    elif tag == "glob":
        pos, batch, xx = torch.zeros(len(ref.GOLD_SIZES), 3), torch.arange(len(ref.GOLD_SIZES)), gold["glob/x"]
    else:
        pos, batch, xx = gold[tag + "/pos"], gold[tag + "/batch"], gold[tag + "/x"]
    return PDData(pos=pos.to(DEV), batch=batch.to(DEV), x=(xx if x is None else x).to(DEV))


def _net(gold):
    from torch_points3d_amd.pointnet2_mp import PointNet2MP
    net = PointNet2MP(ref.GOLD_CFG, ref.GOLD_FEAT, ref.GOLD_CLASSES)
    net.load_state_dict({k[3:]: v for k, v in gold.items() if k.startswith("sd/")}, strict=True)  # the reference's keys
    return net.to(DEV).train()


def _dist64(t, ref64):
    d = t.detach().double().cpu() - torch.as_tensor(ref64)
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def _close(got, gold, key):
    want = gold[key + "/x"]
    torch.testing.assert_close(got.detach().cpu(), want, rtol=1e-5, atol=bound(want, gold["f64/" + key + "/x"]),
                               msg=lambda m: "stage %s: %s" % (key, m))


def test_stages_teacher_forced_on_the_fixture(hip, gold):
    net = _net(gold)
    b0 = net.model
    b1 = b0.submodule
    b2 = b1.submodule
    d1 = b0.down(_bag(gold, "in"))
    assert torch.equal(d1.idx.cpu(), gold["sa1/idx"]) and torch.equal(d1.pos.cpu(), gold["sa1/pos"])
    assert torch.equal(d1.batch.cpu(), gold["sa1/batch"])
    _close(d1.x, gold, "sa1")
    d2 = b1.down(_bag(gold, "sa1"))
    assert torch.equal(d2.idx.cpu(), gold["sa2/idx"]) and torch.equal(d2.batch.cpu(), gold["sa2/batch"])
    _close(d2.x, gold, "sa2")
    dg = b2.inner(_bag(gold, "sa2"))
    assert torch.equal(dg.batch.cpu(), torch.arange(3)) and not bool(dg.pos.any()) and tuple(dg.pos.shape) == (3, 3)
    _close(dg.x, gold, "glob")
    _close(b2.up((_bag(gold, "glob"), _bag(gold, "sa2"))).x, gold, "fp0")
    _close(b1.up((_bag(gold, "sa2", gold["fp0/x"]), _bag(gold, "sa1"))).x, gold, "fp1")
    _close(b0.up((_bag(gold, "sa1", gold["fp1/x"]), _bag(gold, "in"))).x, gold, "fp2")


def test_chained_network_gradients_buffers_and_eval(hip, gold):
    net = _net(gold)
    data = _bag(gold, "in")
    x = data.x.clone().requires_grad_(True)
    data.x = x
    out = net(data)
    own_max, own_rms = _dist64(gold["out/x"], gold["f64/out/x"])
    got_max, got_rms = _dist64(out, gold["f64/out/x"])
    print("chained output vs float64: max %.3e (reference pass %.3e), rms %.3e (reference pass %.3e)" % (
        got_max, own_max, got_rms, own_rms))
    assert got_max <= 4 * own_max and got_rms <= 2 * own_rms, (got_max, own_max, got_rms, own_rms)
    (out * gold["cot"].to(DEV)).sum().backward()
    checked = 0
    for name, p in list(net.named_parameters()) + [("x", x)]:
        want = gold["grad/x"] if p is x else gold.get("pgrad/" + name)
        assert want is not None, name
        if p is not x and name.endswith(".0.bias"):  # Linear bias under train-mode BatchNorm: analytically zero
            wn = float(gold["pgrad/" + name[:-4] + "weight"].norm())
            assert p.grad is None or float(p.grad.norm()) < 1e-4 * wn + 1e-6, name
            continue
        tol = max(1e-4, 4.0 * float(gold["grel/" + name][0]))
        rel = float((p.grad.cpu() - want).norm() / (want.norm() + 1e-30))
        print("gradient %s: relative L2 %.3e (bar %.1e)" % (name, rel, tol))
        assert rel <= tol, (name, rel, tol)
        checked += 1
    assert checked > 40
    sd = net.state_dict()
    after = {k[len("after/"):]: v for k, v in gold.items() if k.startswith("after/")}
    assert len(after) > 30
    for name, v in after.items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v), name
        else:
            torch.testing.assert_close(sd[name].cpu(), v, rtol=1e-4, atol=1e-5, msg=name)
    net.eval()
    with torch.no_grad():
        ev = net(_bag(gold, "in"))
    want = gold["eval/out/x"]
    torch.testing.assert_close(ev.cpu(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))


def test_two_scale_sa_module_matches_reference(hip, gold):
    from torch_points3d_amd.pointnet2_mp import SAModule
    sa = SAModule(**ref.GOLD_MS)
    sa.load_state_dict({k[len("ms/sd/"):]: v for k, v in gold.items() if k.startswith("ms/sd/")}, strict=True)
    sa = sa.to(DEV).train()
    data = _bag(gold, "in")
    for s in range(2):
        edges = sa.neighbour_finder(data.pos, data.pos[gold["ms/idx"].to(DEV)], batch_x=data.batch,
                                    batch_y=data.batch[gold["ms/idx"].to(DEV)], scale_idx=s)
        assert torch.equal(edges.edge_start.cpu(), gold["ms/edges%d/edge_start" % s])
        assert torch.equal(edges[1].cpu(), gold["ms/edges%d/col" % s])
    x = data.x.clone().requires_grad_(True)
    data.x = x
    out = sa(data)
    assert torch.equal(out.idx.cpu(), gold["ms/idx"]) and out.x.shape[1] == 64
    torch.testing.assert_close(out.x.detach().cpu(), gold["ms/x"], rtol=1e-5, atol=bound(gold["ms/x"], gold["ms/f64/x"]))
    (out.x * gold["ms/cot"].to(DEV)).sum().backward()
    want = gold["ms/grad_x"]
    rel = float((x.grad.cpu() - want).norm() / want.norm())
    assert rel <= max(1e-4, 4.0 * float(gold["ms/grel/x"][0])), rel
    sd = sa.state_dict()
    for k, v in gold.items():
        if k.startswith("ms/after/"):
            torch.testing.assert_close(sd[k[len("ms/after/"):]].cpu(), v, rtol=1e-4, atol=1e-5, msg=k)
    sa.eval()
    with torch.no_grad():
        ev = sa(_bag(gold, "in"))
    want = gold["ms/eval/x"]
    torch.testing.assert_close(ev.x.cpu(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))
