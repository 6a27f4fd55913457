"""Host side of the message-passing PointNet++ (torch_points3d_amd/pointnet2_mp.py, torchpoints.fps_quota) and the
consistency of its fixture tests/golden/pointnet2_mp.npz (tests/golden/make_golden_mp.py).  No GPU."""
import pytest
import torch

from conftest import load_golden
import pointnet2_mp_ref as ref


@pytest.fixture(scope="module")
def gold():
    return load_golden("pointnet2_mp")


def test_fps_quota_reference_pin():
    """reference test/test_fps.py:35-42: 5 points, 3 of 5 kept"""
    from torch_points3d_amd import fps_quota
    assert fps_quota([5], 3 / 5.0).tolist() == [3]


@pytest.mark.parametrize("ratio,counts,want", [
    (0.25, [97, 160, 64, 25, 40, 16], [25, 40, 16, 7, 10, 4]),
    (0.2, [5, 10, 97, 2048, 16384], [1, 2, 20, 410, 3277]),
    (1.0, [1, 2, 63, 4099], [1, 2, 63, 4099]),
    (0.25, [1, 0, 3], [1, 0, 1]),  # a single point is kept, an empty cloud gives nothing
    (1e-9, [1, 0], [1, 0]),
])
def test_fps_quota(ratio, counts, want):
    from torch_points3d_amd import fps_quota
    got = fps_quota(counts, ratio)
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert got.tolist() == want
    assert got.tolist() == ref.fps_quota(counts, ratio)
    assert fps_quota(torch.tensor(counts), ratio).tolist() == want


def test_fps_quota_never_exceeds_the_cloud():
    from torch_points3d_amd import fps_quota
    counts = list(range(0, 300))
    for ratio in (0.2, 0.25, 0.5, 0.999, 1.0, 1.5):
        got = fps_quota(counts, ratio).tolist()
        assert all(0 <= q <= n for q, n in zip(got, counts))
        assert got == ref.fps_quota(counts, ratio)


def test_sampler_and_finder_constructor_errors():
    from torch_points3d_amd.pointnet2_mp import FPSSampler, MultiscaleRadiusNeighbourFinder, RadiusNeighbourFinder
    with pytest.raises(ValueError, match="not several"):
        FPSSampler(ratio=0.5, num_to_sample=10)
    with pytest.raises(ValueError, match="not several"):
        FPSSampler(num_to_sample=10, subsampling_param=2)
    with pytest.raises(Exception, match="should be defined"):
        FPSSampler()
    with pytest.raises(ValueError, match="dimension 2"):
        FPSSampler(ratio=0.5).sample(torch.rand(2, 8, 3), None)
    assert FPSSampler(num_to_sample=10)._get_ratio_to_sample(40) == 0.25
    with pytest.raises(ValueError, match="same length"):
        MultiscaleRadiusNeighbourFinder([0.1, 0.2], [8, 16, 32])
    ms = MultiscaleRadiusNeighbourFinder([0.1, 0.2], 8)
    assert ms.num_scales == 2 and ms._max_num_neighbors == [8, 8]
    ms = MultiscaleRadiusNeighbourFinder(0.3, [8, 16, 32])
    assert ms.num_scales == 3 and ms._radius == [0.3, 0.3, 0.3]
    assert MultiscaleRadiusNeighbourFinder(0.3, 8).num_scales == 1
    with pytest.raises(ValueError, match="out of bounds"):
        ms.find_neighbours(torch.rand(4, 3), torch.rand(4, 3), scale_idx=3)
    assert RadiusNeighbourFinder(0.1, conv_type="PARTIAL_DENSE")._conv_type == "partial_dense"


def test_cpu_tensors_are_refused():
    from torch_points3d_amd import fps_ragged
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fps_ragged(torch.rand(8, 3), torch.zeros(8, dtype=torch.long), ratio=0.5)
    with pytest.raises(ValueError):
        fps_ragged(torch.rand(8, 3), None)  # neither ratio nor counts
    with pytest.raises(ValueError):
        fps_ragged(torch.rand(8, 3), None, ratio=0.5, counts=[4])


def _sd_keys(gold, prefix):
    return [k[len(prefix):] for k in gold if k.startswith(prefix)]


def test_state_dict_keys_match_the_reference(gold):
    from torch_points3d_amd.pointnet2_mp import FPModule, GlobalBaseModule, PointNet2MP, SAModule
    cfg = ref.GOLD_CFG
    net_keys = _sd_keys(gold, "sd/")
    assert len(net_keys) > 80
    net = PointNet2MP(cfg, ref.GOLD_FEAT, ref.GOLD_CLASSES)
    assert list(net.state_dict().keys()) == net_keys
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(gold["sd/" + k].shape), k
    down, up = cfg["down_conv"], cfg["up_conv"]
    sa = SAModule(ratio=down["ratios"][0], radius=down["radius"][0], radius_num_point=down["radius_num_points"][0],
                  down_conv_nn=down["down_conv_nn"][0])
    assert list(sa.state_dict().keys()) == _sd_keys(gold, "sd/model.down.")
    glob = GlobalBaseModule(**cfg["innermost"])
    assert list(glob.state_dict().keys()) == _sd_keys(gold, "sd/model.submodule.submodule.inner.")
    fp = FPModule(up_k=up["up_k"][0], up_conv_nn=up["up_conv_nn"][0])
    assert list(fp.state_dict().keys()) == _sd_keys(gold, "sd/model.submodule.submodule.up.")
    assert list(SAModule(**ref.GOLD_MS).state_dict().keys()) == _sd_keys(gold, "ms/sd/")
    # the bundled configurations build, with the reference's widths
    full = PointNet2MP("pointnet2", 3, 13)
    assert full.lin3.out_features == 13 and full.model.down._conv.local_nn[0][0].in_features == 6
    assert PointNet2MP("pointnet2ms", 3, 13).model.submodule.down.neighbour_finder.num_scales == 2


def test_fixture_is_self_consistent(gold):
    stages = ("sa1", "sa2", "glob", "fp0", "fp1", "fp2", "out")
    for k in stages:
        a, b = gold[k + "/x"], torch.as_tensor(gold["f64/" + k + "/x"])
        scale = max(1.0, float(b.abs().max()))
        assert float((a.double() - b).abs().max()) <= 1e-5 * scale, k
        assert gold["eval/" + k + "/x"].shape == a.shape
    a, b = gold["ms/x"], torch.as_tensor(gold["ms/f64/x"])
    assert float((a.double() - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
    sizes = torch.bincount(gold["batch"]).tolist()
    assert tuple(sizes) == ref.GOLD_SIZES
    l1 = ref.fps_quota(sizes, 0.25)
    assert torch.bincount(gold["sa1/batch"]).tolist() == l1 == [25, 40, 16]
    assert torch.bincount(gold["sa2/batch"]).tolist() == ref.fps_quota(l1, 0.25) == [7, 10, 4]
    for tag, nq in (("edges/sa1", 81), ("edges/sa2", 21), ("ms/edges0", 81), ("ms/edges1", 81)):
        es, col = gold[tag + "/edge_start"], gold[tag + "/col"]
        deg = es[1:] - es[:-1]
        assert es.numel() == nq + 1 and int(es[0]) == 0 and int(es[-1]) == col.numel()
        assert int(deg.min()) >= 1, "a query without an edge"  # (every sampled query is its own neighbour)
    deg = gold["edges/sa1/edge_start"][1:] - gold["edges/sa1/edge_start"][:-1]
    cap = int(gold["cap"])
    assert int(deg.max()) == cap and int((deg == cap).sum()) >= 5 and int((deg < cap).sum()) >= 5
    # the sampled rows start every cloud at its first row
    starts = torch.tensor([0, 97, 257])
    assert torch.equal(gold["sa1/idx"][torch.tensor([0, 25, 65])], starts)


def test_cpu_statement_of_the_kernels():
    """the plain-torch statement the GPU tests compare against: hand-checked on a tiny case"""
    table = torch.tensor([[2, 5, -1], [-1, -1, -1], [0, 1, 4]])
    es, col = ref.table_edges(table)
    assert es.tolist() == [0, 2, 2, 5] and col.tolist() == [2, 5, 0, 1, 4]
    pos_s = torch.arange(18.0).reshape(6, 3)
    pos_q = torch.ones(3, 3)
    x = torch.arange(6.0).reshape(6, 1)
    rows = ref.edge_rows(x, pos_s, pos_q, es, col, ld=8)
    assert rows.shape == (5, 8) and rows[0].tolist() == [2.0, 5.0, 6.0, 7.0, 0, 0, 0, 0]
    vals = torch.tensor([[1.0], [3.0], [3.0], [2.0], [0.5]])
    out, arg = ref.segment_max(vals, es)
    assert out.reshape(-1).tolist() == [3.0, 0.0, 3.0] and arg.reshape(-1).tolist() == [1, -1, 2]


# ------------------------------------------------------------------------------ the torch mirror of the modules, pinned
# tests/pointnet2_mp_ref.py restates PointConv / SAModule / GlobalBaseModule / FPModule / PointNet2MP in plain torch so
# that GPU tests can evaluate them in float64 at widths no fixture can hold.  Before it is trusted there, its float64
# run has to reproduce what the REFERENCE's own classes computed in float64 (the fixture's f64/* arrays) and the stored
# gradients.  The bar is the one test_fixture_is_self_consistent states for the fixture's own float32-vs-float64
# distance, 1e-5 * max(1, scale): the float64 arrays are met to rounding, the stored gradients are float32 ones.
def _within(got, want, what):
    want = torch.as_tensor(want).double()
    scale = max(1.0, float(want.abs().max()))
    d = float((got.detach().double() - want).abs().max())
    print("mirror vs fixture, %s: max distance %.3e (bar %.1e)" % (what, d, 1e-5 * scale))
    assert got.shape == want.shape and d <= 1e-5 * scale, (what, d, scale)


def _gold_plan(oracle, gold):
    down, up = ref.GOLD_CFG["down_conv"], ref.GOLD_CFG["up_conv"]
    plan = ref.search_plan(oracle, gold["pos"], gold["batch"], down["ratios"], down["radius"], down["radius_num_points"],
                           up["up_k"])
    for i in range(2):  # the oracle's searches ARE the fixture's
        assert torch.equal(plan["idx"][i], gold["sa%d/idx" % (i + 1)])
        assert torch.equal(plan["edges"][i][0][0], gold["edges/sa%d/edge_start" % (i + 1)])
        assert torch.equal(plan["edges"][i][0][1], gold["edges/sa%d/col" % (i + 1)])
    assert [tuple(t.shape) for t in plan["knn"]] == [(21, 1), (81, 3), (321, 3)]
    return plan


def test_float64_mirror_reproduces_the_fixture(oracle, gold):
    sd = {k[3:]: v for k, v in gold.items() if k.startswith("sd/")}
    net = ref.PointNet2MP.from_state_dict(sd, torch.float64)
    assert net.levels == 2 and list(net.state_dict().keys()) == list(sd.keys())
    x = gold["x"].double().requires_grad_(True)
    rec = net(x, gold["pos"].double(), gold["batch"], _gold_plan(oracle, gold))
    for k in ("sa1", "sa2", "glob", "fp0", "fp1", "fp2", "out"):
        _within(rec[k], gold["f64/" + k + "/x"], k)
    (rec["out"] * gold["cot"].double()).sum().backward()
    _within(x.grad, gold["grad/x"], "grad x")
    checked = 0
    for name, p in net.named_parameters():
        want = gold.get("pgrad/" + name)
        assert want is not None and p.grad is not None, name
        _within(p.grad, want, "grad " + name)
        checked += 1
    assert checked > 50
    # the float32 run of the same classes lies as close to the float64 arrays as the fixture's own float32 pass does
    net32 = ref.PointNet2MP.from_state_dict(sd, torch.float32)
    rec32 = net32(gold["x"], gold["pos"], gold["batch"], _gold_plan(oracle, gold))
    for k in ("sa1", "sa2", "glob", "fp0", "fp1", "fp2", "out"):
        _within(rec32[k], gold["f64/" + k + "/x"], k + " (float32 mirror)")


def test_float64_mirror_reproduces_the_two_scale_module(gold):
    sd = {k[len("ms/sd/"):]: v for k, v in gold.items() if k.startswith("ms/sd/")}
    sa = ref.SAModule.from_state_dict(sd, torch.float64)
    edges = [(gold["ms/edges%d/edge_start" % s], gold["ms/edges%d/col" % s]) for s in range(2)]
    x = gold["x"].double().requires_grad_(True)
    out = sa(x, gold["pos"].double(), gold["ms/idx"], edges)
    _within(out, gold["ms/f64/x"], "two-scale SAModule")
    (out * gold["ms/cot"].double()).sum().backward()
    _within(x.grad, gold["ms/grad_x"], "two-scale SAModule grad x")


def test_mirror_pieces_by_hand():
    """a query without an edge gives 0.0 and its rows are absent from BatchNorm; the blend skips -1 slots; modules build
    from a state_dict alone"""
    from torch_points3d_amd.pointnet2_mp import FPModule, GlobalBaseModule, SAModule
    torch.manual_seed(0)
    prod = SAModule(ratio=0.5, radius=1.0, radius_num_point=4, down_conv_nn=[2 + 3, 8, 6])
    sa = ref.SAModule.from_state_dict(prod.state_dict(), torch.float64)
    pos = torch.rand(6, 3).double()
    x = torch.randn(6, 2).double()
    es, col = torch.tensor([0, 2, 2, 5]), torch.tensor([0, 3, 1, 2, 5])
    out = sa._conv(x, (pos, torch.rand(3, 3).double()), (es, col))
    assert out.shape == (3, 6) and not bool(out[1].any()) and bool(out[0].any())
    assert int(sa._conv.local_nn[0][1].batch_norm.num_batches_tracked) == 1
    w = ref.knn_blend(torch.tensor([[1.0], [3.0], [100.0]]), torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [9.0, 9, 9]]),
                      torch.zeros(1, 3), torch.tensor([[0, 1, -1]]))
    assert w.tolist() == [[2.0]]
    glob = ref.GlobalBaseModule.from_state_dict(GlobalBaseModule(nn=[5, 7]).state_dict())
    assert glob(x, pos, torch.tensor([0, 0, 0, 2, 2, 2])).shape == (3, 7)
    fp = ref.FPModule.from_state_dict(FPModule(up_k=1, up_conv_nn=[4, 3]).state_dict())
    assert fp.nn[0][0].bias is None and fp.nn[0][0].in_features == 4
