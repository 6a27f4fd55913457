"""Message-passing PointNet++ kernels past their first tile, and the modules at the published widths.

tests/test_gpu_pointnet2_mp.py keeps every shape inside the first tile of every kernel.  Here: the scan of
tp3d_table_edge_start_i64 over several tiles of 4096 queries, tp3d_segment_max_bwd_f32 with a segment cut into pieces,
every register template of tp3d_fps_ragged_f32, edge rows at cap 128 and 387 + 3 columns with a hub row in the scatter
backward, and `PointNet2MP("pointnet2ms")` against the float64 run of the plain-torch mirror of
tests/pointnet2_mp_ref.py (pinned against the reference's fixture in tests/test_pointnet2_mp_cpu.py).  Every test
asserts the precondition that puts it past the tile it is about.

Bars.  Index outputs, copies, and sums of eighths: torch.equal.  Floating point as tests/test_gpu_pointnet2_mp.py
writes them, with the float32 CPU run of the mirror in the place of the reference's float32 pass: stages teacher-forced
on the float32 mirror's tensors rtol 1e-5, atol = bound(mirror32, mirror64); the chained output by its distance to the
float64 mirror, <= 4x max and <= 2x RMS of the float32 mirror's own; gradients relative L2 to the float64 mirror's,
<= max(1e-4, 4x the float32 mirror's own relative distance).  The code under test is never the yardstick.  The observed
figures are printed and recorded in DESIGN.md ("message-passing PointNet++")."""
import pytest
import torch

import pointnet2_mp_ref as ref
from randla_golden_util import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCAN_TILE = 4 * 1024  # scan_kernel: values per tile
FPS_THRESHOLDS = [128, 512, 1024, 2048, 4096, 8192, 16384, 32768]  # largest cloud <= t picks the t-th register template


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _seg_of(lengths):
    seg = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return seg


# ------------------------------------------------------------------------------------- 1. table -> edges across tiles
def _tables(Nq, W, M=977):
    """random ids with holes anywhere in a row (plain, and with the fixed empty / full rows), all full, all empty"""
    g = torch.Generator().manual_seed(Nq * 131 + W)
    ids = torch.randint(0, M, (Nq, W), generator=g)
    plain = torch.where(torch.rand(Nq, W, generator=g) < 0.4, torch.full_like(ids, -1), ids)
    fixed = plain.clone()
    for r in (1, 4097):
        if r < Nq:
            fixed[r] = ids[r]
    for r in (0, 4095, 4096, Nq - 1):
        if r < Nq:
            fixed[r] = -1
    return dict(plain=plain, fixed=fixed, full=ids, empty=torch.full_like(ids, -1))


@pytest.mark.parametrize("Nq,W", [(4095, 3), (4096, 3), (4097, 1), (8192, 2), (8193, 65), (12290, 5), (1, 130)])
def test_table_edges_across_scan_tiles(hip, Nq, W):
    tiles = (Nq + SCAN_TILE - 1) // SCAN_TILE
    assert tiles == {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 12290: 4, 1: 1}[Nq]
    for name, table in _tables(Nq, W).items():
        want_es, want_col = ref.table_edges(table)
        if name == "fixed" and Nq > 1:
            deg = want_es[1:] - want_es[:-1]
            assert int(deg[0]) == 0 and int(deg[-1]) == 0 and int(deg[1]) == W
            assert Nq <= 4097 or (int(deg[4095]) == 0 and int(deg[4096]) == 0 and int(deg[4097]) == W)
        if name == "plain":  # holes in front of hits, inside a row
            assert bool(((table[:, :-1] < 0) & (table[:, 1:] >= 0)).any()) or W == 1
        es, col = hip.table_edges(table.to(DEV))
        assert es.dtype == torch.int64 and col.dtype == torch.int64
        assert torch.equal(es.cpu(), want_es), (name, "edge_start")
        assert torch.equal(col.cpu(), want_col), (name, "col")
        if name == "empty":
            assert col.numel() == 0 and int(es[-1]) == 0
        if name == "full":
            assert col.numel() == Nq * W


def test_radius_edges_past_one_scan_tile(hip, oracle):
    g = torch.Generator().manual_seed(31)
    sizes, cap, radius = [3000, 2200], 3, 0.12
    pos = torch.rand(sum(sizes), 3, generator=g) * 2 - 1
    b = _batch_of(sizes)
    want_es, want_col = ref.table_edges(oracle.ball_query(radius, cap, pos, pos, mode="partial_dense", batch_x=b, batch_y=b)[0])
    deg = want_es[1:] - want_es[:-1]
    inside = oracle.ball_query(radius, 4 * cap, pos, pos, mode="partial_dense", batch_x=b, batch_y=b)[0]
    assert pos.shape[0] > SCAN_TILE
    assert int(((inside >= 0).sum(1) > cap).sum()) >= 100, "no query is cut at the cap"
    assert int(deg.min()) >= 1 and int((deg < cap).sum()) >= 100 and int(deg.max()) == cap
    es, col = hip.radius_edges(radius, cap, pos.to(DEV), pos.to(DEV), b.to(DEV), b.to(DEV))
    assert torch.equal(es.cpu(), want_es) and torch.equal(col.cpu(), want_col)


# ------------------------------------------------------------------------------ 2. segmented max, a segment in pieces
def _parts(E, S):
    """tp3d_segment_max_bwd_f32: pieces per segment, about 64 rows each, from the MEAN segment length, at most 1024"""
    return max(1, min(1024, (E // S + 63) // 64))


def _per(length, parts):
    """segment_max_bwd_kernel: rows per piece of a segment of `length` rows"""
    return (length + parts - 1) // parts


def _segment_max_case(hip, lengths, C, ld, seed, tie=None, want_parts=None):
    g = torch.Generator().manual_seed(seed)
    seg = _seg_of(lengths)
    E, S = int(seg[-1]), len(lengths)
    parts = _parts(E, S)
    assert parts > 1 and (want_parts is None or parts == want_parts), parts
    rows = torch.randint(-8, 9, (E, ld), generator=g).float() / 8  # eighths in [-1, 1]: maxima repeat
    if tie is not None:
        s, first, second = tie
        per = _per(lengths[s], parts)
        assert first < second < lengths[s] and first // per != second // per, "the tie must straddle a piece boundary"
        rows[int(seg[s]) + first] = rows[int(seg[s]) + second] = 2.0
    want, warg = ref.segment_max(rows, seg, C)
    cot = torch.randint(-32, 33, want.shape, generator=g).float() / 8
    rc = rows.clone().requires_grad_(True)
    (ref.segment_max(rc, seg, C)[0] * cot).sum().backward()
    rg = rows.to(DEV).requires_grad_(True)
    out, arg = hip.segment_max(rg, seg.to(DEV), C=C, return_argmax=True)
    assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu(), warg)
    # the wrapper takes d_rows from torch.empty: leave something other than zeros where it is likely to land
    junk = torch.full((E, ld), float("nan"), device=DEV)
    del junk
    (out * cot.to(DEV)).sum().backward()
    got = rg.grad.cpu()
    assert torch.equal(got, rc.grad), (lengths, C, ld)
    assert not bool(got[:, C:].any()), "padding columns of the gradient"
    if tie is not None:
        s, first, second = tie
        assert bool((warg[s] == int(seg[s]) + first).all()), "the earlier row wins"
        assert torch.equal(got[int(seg[s]) + first, :C], cot[s]) and not bool(got[int(seg[s]) + second].any())
    return parts


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("lengths,C,parts,tie", [
    ([495], 3, 8, None),
    ([700, 1, 130], 67, 5, (0, 139, 140)),  # per = 140 / 1 (four pieces empty) / 26
    ([0, 1000, 0, 65], 5, 5, None),
    ([300, 5, 129], 1024, 3, None),  # 16 channel chunks per segment in the forward
    ([70001], 2, 1024, (0, 69 * 500 - 1, 69 * 500)),  # E / S > 65536: the clamp; per = 69
], ids=["495x3", "700-1-130x67", "0-1000-0-65x5", "300-5-129x1024", "70001x2"])
def test_segment_max_with_a_segment_in_pieces(hip, lengths, C, parts, tie, pad):
    if lengths == [70001]:
        assert sum(lengths) // len(lengths) > 65536 and _per(70001, 1024) == 69
    if lengths == [700, 1, 130]:
        assert _per(700, 5) == 140 and _per(130, 5) == 26 and _per(1, 5) == 1  # (per is taken segment by segment)
    _segment_max_case(hip, lengths, C, C + pad, seed=7 * C + pad, tie=tie, want_parts=parts)


def test_global_max_pool_with_an_empty_cloud(hip):
    from torch_points3d_amd.pointnet2_mp import global_max_pool
    sizes, C = [300, 0, 5, 129], 67
    g = torch.Generator().manual_seed(17)
    batch = _batch_of(sizes)
    seg = _seg_of(sizes)
    assert _parts(sum(sizes), len(sizes)) > 1
    x = torch.randint(-8, 9, (sum(sizes), C), generator=g).float() / 8
    cot = torch.randint(-32, 33, (len(sizes), C), generator=g).float() / 8
    xc = x.clone().requires_grad_(True)
    want = ref.segment_max(xc, seg)[0]
    (want * cot).sum().backward()
    xg = x.to(DEV).requires_grad_(True)
    out = global_max_pool(xg, batch.to(DEV))
    assert tuple(out.shape) == (4, C) and torch.equal(out.cpu(), want.detach()) and not bool(out[1].any())
    (out * cot.to(DEV)).sum().backward()
    assert torch.equal(xg.grad.cpu(), xc.grad)


# ------------------------------------------------------------------------------ 3. ragged FPS, every register template
def _oracle_fps(oracle, pos, sizes, quotas):
    out, base = [], 0
    for n, q in zip(sizes, quotas):
        if n and q:
            out.append(oracle.furthest_point_sample(pos[base:base + n].unsqueeze(0), q)[0] + base)
        base += n
    return torch.cat(out)


@pytest.mark.parametrize("N", [129, 513, 1025, 2049, 4097, 8193, 16385, 32768])
def test_fps_ragged_on_every_register_template(hip, oracle, N):
    picked = min(t for t in FPS_THRESHOLDS if N <= t)
    below = [t for t in FPS_THRESHOLDS if t < picked]
    assert below and (N == below[-1] + 1 or N == FPS_THRESHOLDS[-1]), "just above the previous threshold"
    sizes = [1, 63, 0, N, 2, 65]  # the largest cloud picks the template; id 2 has no point
    quotas = [1, 63, 0, 24, 2, 65]
    assert max(sizes) == N
    g = torch.Generator().manual_seed(N)
    pos = torch.rand(sum(sizes), 3, generator=g) * 2 - 1
    got = hip.fps_ragged(pos.to(DEV), _batch_of(sizes).to(DEV), counts=quotas)
    want = _oracle_fps(oracle, pos, sizes, quotas)
    assert got.dtype == torch.int64 and got.numel() == sum(quotas)
    base = qbase = 0
    for n, q in zip(sizes, quotas):  # cloud by cloud
        assert torch.equal(got[qbase:qbase + q].cpu(), want[qbase:qbase + q]), (N, n)
        assert q == 0 or (int(want[qbase]) == base and int(want[qbase:qbase + q].max()) < base + n)
        base, qbase = base + n, qbase + q


def test_fps_ragged_first_cloud_id_is_empty(hip, oracle):
    g = torch.Generator().manual_seed(13)
    sizes = [0, 300, 70]
    pos = torch.rand(sum(sizes), 3, generator=g)
    batch = _batch_of(sizes)
    assert int(batch[0]) == 1
    got = hip.fps_ragged(pos.to(DEV), batch.to(DEV), ratio=0.25)
    assert torch.equal(got.cpu(), _oracle_fps(oracle, pos, sizes, ref.fps_quota(sizes, 0.25)))
    got = hip.fps_ragged(pos.to(DEV), batch.to(DEV), counts=[0, 5, 70])
    assert torch.equal(got.cpu(), _oracle_fps(oracle, pos, sizes, [0, 5, 70]))


# ------------------------------------------------------------------------------ 4. edge rows at published caps, widths
def test_pointconv_rows_at_cap_128_and_387_columns(hip, oracle):
    g = torch.Generator().manual_seed(41)
    cap, C = 128, 387
    sizes, qsizes = [420, 90], [30, 12]
    pos_s = torch.cat([torch.rand(300, 3, generator=g) * 0.2, torch.rand(120, 3, generator=g) * 2 - 1,
                       torch.rand(90, 3, generator=g) * 2 - 1])
    pos_q = torch.cat([torch.rand(10, 3, generator=g) * 0.2, torch.rand(20, 3, generator=g) * 2 - 1,
                       torch.rand(12, 3, generator=g) * 2 - 1])
    bs, bq = _batch_of(sizes), _batch_of(qsizes)
    es, col = ref.table_edges(oracle.ball_query(0.4, cap, pos_s, pos_q, mode="partial_dense", batch_x=bs, batch_y=bq)[0])
    deg = es[1:] - es[:-1]
    assert int(deg.max()) == cap and int((deg == cap).sum()) >= 1 and int(((deg > 0) & (deg < 64)).sum()) >= 1
    hes, hcol = hip.radius_edges(0.4, cap, pos_s.to(DEV), pos_q.to(DEV), bs.to(DEV), bq.to(DEV))
    assert torch.equal(hes.cpu(), es) and torch.equal(hcol.cpu(), col)
    x = torch.randn(sum(sizes), C, generator=g)
    for ld in (390, 392):
        want = ref.edge_rows(x, pos_s, pos_q, es, col, ld=ld)
        got = hip.pointconv_rows(x.to(DEV), pos_s.to(DEV), pos_q.to(DEV), hes, hcol, ld=ld)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), ld


def test_pointconv_rows_backward_with_a_hub_support_row(hip):
    """one support row in every one of 3000 queries (a hub bin of tp3d_rows_scatter_bwd_f32), ordinary rows beside it;
    cotangents in eighths, |v| <= 4: the hub's sum stays below 2^24 eighths, every partial sum is exact in float32"""
    g = torch.Generator().manual_seed(43)
    M, Nq, C, hub = 500, 3000, 35, 123
    others = torch.randint(0, M - 1, (Nq, 2), generator=g)
    others = others + (others >= hub).long()  # never the hub itself
    col = torch.sort(torch.cat([torch.full((Nq, 1), hub), others], 1), 1)[0].reshape(-1)
    es = torch.arange(Nq + 1) * 3
    count = torch.bincount(col, minlength=M)
    assert int(count[hub]) == Nq >= 3000 and int(count.sum() - count[hub]) == 2 * Nq and 4 * 8 * Nq < 2 ** 24
    x = torch.randn(M, C, generator=g)
    pos_s, pos_q = torch.rand(M, 3, generator=g), torch.rand(Nq, 3, generator=g)
    for ld in (C + 3, 40):
        xg = x.clone().to(DEV).requires_grad_(True)
        rows = hip.pointconv_rows(xg, pos_s.to(DEV), pos_q.to(DEV), es.to(DEV), col.to(DEV), ld=ld)
        assert torch.equal(rows.cpu(), ref.edge_rows(x, pos_s, pos_q, es, col, ld=ld))
        cot = torch.randint(-32, 33, (Nq * 3, ld), generator=g).float() / 8
        (rows * cot.to(DEV)).sum().backward()
        want = torch.zeros_like(x).index_add_(0, col, cot[:, :C])
        assert torch.equal(xg.grad.cpu(), want), ld


# ------------------------------------------------------------------------------ 5. the modules at the published widths
def _dist(a, b):
    d = a.detach().double().cpu() - b.detach().double()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double()).norm() / (b.detach().double().norm() + 1e-300))


MS_SIZES, MS_FEAT, MS_CLASSES = (700, 260, 90), 4, 5


def _ms_build(oracle, seed):
    """`pointnet2ms` at its published widths on three clouds, the searches by the CPU oracle, and the mirror's float32
    and float64 CPU runs on them (forward, one backward).  Shared, never modified.

    Cloud 0: 580 points in a ball of radius 0.09 (queries there are cut at cap 32 of the 0.1 scale) and 120 points spread
    over [-1, 1]^3, which furthest-point sampling reaches first and which keep their self edge only.  Cloud 2: 90 points
    spread over [-2, 2]^3, sparse at every first-level radius."""
    from torch_points3d_amd.pointnet2_mp import PointNet2MP, mp_config
    g = torch.Generator().manual_seed(seed)
    ball = torch.randn(580, 3, generator=g)
    ball = ball / ball.norm(dim=1, keepdim=True) * 0.09 * torch.rand(580, 1, generator=g) ** (1.0 / 3)
    pos = torch.cat([ball, torch.rand(120, 3, generator=g) * 2 - 1, torch.rand(260, 3, generator=g) - 0.5,
                     torch.rand(90, 3, generator=g) * 4 - 2])
    pos = torch.cat([pos[:700][torch.randperm(700, generator=g)], pos[700:]])
    batch = _batch_of(list(MS_SIZES))
    x = torch.randn(pos.shape[0], MS_FEAT, generator=g)
    cfg = mp_config("pointnet2ms", MS_FEAT)
    torch.manual_seed(5)
    net = PointNet2MP(cfg, MS_FEAT, MS_CLASSES)
    # train-mode dropout draws from the device's generator, which no CPU run can replay: the head runs without it (the
    # mirror has none); everything else is the published configuration
    net.dropout = 0.0
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    down = cfg["down_conv"]
    plan = ref.search_plan(oracle, pos, batch, down["ratios"], down["radius"], down["radius_num_points"],
                           cfg["up_conv"]["up_k"])
    cot = torch.randn(pos.shape[0], MS_CLASSES, generator=g)
    runs = {}
    for dtype in (torch.float32, torch.float64):
        m = ref.PointNet2MP.from_state_dict(sd, dtype)
        xin = x.clone().to(dtype).requires_grad_(True)
        rec = m(xin, pos.to(dtype), batch, plan)
        (rec["out"] * cot.to(dtype)).sum().backward()
        grads = {k: p.grad for k, p in m.named_parameters()}
        grads["x"] = xin.grad
        runs[dtype] = dict(rec={k: v.detach() for k, v in rec.items()}, grads=grads, after=m.state_dict(),
                           margin=m.margin())
    g32, g64 = runs[torch.float32]["grads"], runs[torch.float64]["grads"]
    own = max(_rel(g32[k], g64[k]) for k in g64 if not k.endswith(".0.bias"))
    return dict(net=net, sd=sd, pos=pos, batch=batch, x=x, plan=plan, cot=cot, m32=runs[torch.float32],
                m64=runs[torch.float64], cfg=cfg, seed=seed, own_grad=own)


# Where the search for inputs starts.  Of the seeds 2026 .. 2045 this one gives the float64 mirror its widest closest
# max-pool contest (ref.pool_margin: 6.9e-6; 2.6e-7 .. 4e-6 for the others, and float32 rounding of these values is of
# the order of 1e-6: the float32 MIRROR crowns another row somewhere at 8 of the 20 seeds, and its gradients then lie 1e-3
# and more from the float64 ones).  Chosen from the mirror's runs alone, before the kernels ever saw these inputs.
MS_SEED = 2028


@pytest.fixture(scope="module")
def ms_case(oracle):
    """the first seed from MS_SEED on at which the float32 MIRROR's gradients lie within 1e-3 (relative L2) of its float64
    ones, i.e. at which float32 rounding alone does not flip a max-pool winner that matters (the re-seeding of
    tests/golden/make_golden_deform.py; the criterion never looks at the code under test)"""
    for seed in range(MS_SEED, MS_SEED + 12):
        case = _ms_build(oracle, seed)
        print("pointnet2ms case, seed %d: float32 mirror's worst gradient distance %.3e" % (seed, case["own_grad"]))
        if case["own_grad"] <= 1e-3:
            return case
    raise RuntimeError("no seed at which the float32 mirror keeps its max-pool winners")


def test_ms_case_reaches_what_it_is_about(ms_case):
    c = ms_case
    es0 = c["plan"]["edges"][0][0][0]  # first level, smallest radius (0.1, cap 32)
    deg = es0[1:] - es0[:-1]
    qbatch = c["plan"]["batch"][1]
    assert torch.bincount(qbatch).tolist() == ref.fps_quota(MS_SIZES, 0.25) == [175, 65, 23]
    lonely = int(((deg == 1) & (qbatch == 0)).sum())
    print("first level, radius 0.1: %d queries of cloud 0 with their self edge only, %d at cap 32" % (
        lonely, int((deg == 32).sum())))
    assert int(deg.min()) == 1 and lonely >= 3 and int(deg.max()) == 32
    caps = c["cfg"]["down_conv"]["radius_num_points"]
    assert caps == [[32, 64, 128], [64, 128]]
    big = c["plan"]["edges"][0][2][0]
    assert int((big[1:] - big[:-1]).max()) == 128  # two 64-slot steps of the table kernels
    assert c["m32"]["rec"]["glob"].shape == (3, 1024) and c["m32"]["rec"]["sa1"].shape == (263, 384)
    print("seed %d; float32 mirror's gradients vs float64: worst relative L2 %.3e; closest max-pool contest %.2e" % (
        c["seed"], c["own_grad"], c["m64"]["margin"]))
    assert c["own_grad"] <= 1e-3


def _bag(pos, batch, x):
    from torch_points3d_amd.kpconv_blocks import PDData
    return PDData(pos=pos.to(DEV), batch=batch.to(DEV), x=x.float().to(DEV))


def _product(c):
    net = c["net"]
    net.load_state_dict(c["sd"], strict=True)  # (the buffers of an earlier test's pass are put back)
    return net.to(DEV).train()


def test_ms_searches_and_stages_teacher_forced(hip, ms_case):
    c = ms_case
    net, plan, m32, m64 = _product(c), c["plan"], c["m32"]["rec"], c["m64"]["rec"]
    blocks = [net.model, net.model.submodule, net.model.submodule.submodule]
    level_x = [c["x"], m32["sa1"], m32["sa2"]]

    def close(got, key):
        got_max, _ = _dist(got, m32[key])
        atol = bound(m32[key], m64[key].numpy())
        print("stage %s vs the float32 mirror: max %.3e (atol %.1e; mirror32 vs mirror64 %.3e)" % (
            key, got_max, atol, _dist(m32[key], m64[key])[0]))
        torch.testing.assert_close(got.detach().cpu(), m32[key], rtol=1e-5, atol=atol,
                                   msg=lambda m: "stage %s: %s" % (key, m))

    for i in range(2):
        sa = blocks[i].down
        pos, batch = plan["pos"][i].to(DEV), plan["batch"][i].to(DEV)
        out = sa(_bag(plan["pos"][i], plan["batch"][i], level_x[i]))
        assert torch.equal(out.idx.cpu(), plan["idx"][i]) and torch.equal(out.batch.cpu(), plan["batch"][i + 1])
        assert torch.equal(out.pos.cpu(), plan["pos"][i + 1])
        for s, (want_es, want_col) in enumerate(plan["edges"][i]):
            e = sa.neighbour_finder(pos, pos[out.idx], batch_x=batch, batch_y=batch[out.idx], scale_idx=s)
            assert torch.equal(e.edge_start.cpu(), want_es) and torch.equal(e[1].cpu(), want_col), (i, s)
        close(out.x, "sa%d" % (i + 1))
    glob = blocks[2].inner(_bag(plan["pos"][2], plan["batch"][2], m32["sa2"]))
    assert torch.equal(glob.batch.cpu(), torch.arange(3)) and not bool(glob.pos.any())
    close(glob.x, "glob")
    cur, cur_pos, cur_batch = m32["glob"], torch.zeros(3, 3), torch.arange(3)
    for j in range(3):
        lv = 2 - j
        idx, _ = hip.knn(c["cfg"]["up_conv"]["up_k"][j], cur_pos.to(DEV), plan["pos"][lv].to(DEV), cur_batch.to(DEV),
                         plan["batch"][lv].to(DEV))
        assert torch.equal(idx.cpu(), plan["knn"][j]), j
        up = blocks[lv].up((_bag(cur_pos, cur_batch, cur), _bag(plan["pos"][lv], plan["batch"][lv], level_x[lv])))
        close(up.x, "fp%d" % j)
        cur, cur_pos, cur_batch = m32["fp%d" % j], plan["pos"][lv], plan["batch"][lv]


def test_ms_chained_network_gradients_and_buffers(hip, ms_case):
    c = ms_case
    net = _product(c)
    data = _bag(c["pos"], c["batch"], c["x"])
    x = data.x.clone().requires_grad_(True)
    data.x = x
    out = net(data)
    want = c["m64"]["rec"]["out"]
    own_max, own_rms = _dist(c["m32"]["rec"]["out"], want)
    got_max, got_rms = _dist(out, want)
    print("chained output vs float64 mirror: max %.3e (float32 mirror %.3e), rms %.3e (float32 mirror %.3e)" % (
        got_max, own_max, got_rms, own_rms))
    assert got_max <= 4 * own_max and got_rms <= 2 * own_rms, (got_max, own_max, got_rms, own_rms)
    (out * c["cot"].to(DEV)).sum().backward()
    g32, g64 = c["m32"]["grads"], c["m64"]["grads"]
    checked, worst = 0, (0.0, None)
    failed = []
    for name, p in list(net.named_parameters()) + [("x", x)]:
        if name.endswith(".0.bias") and name.startswith("model."):  # Linear bias under train-mode BatchNorm: zero
            wn = float(g64[name[:-4] + "weight"].norm())
            assert p.grad is None or float(p.grad.norm()) < 1e-4 * wn + 1e-6, name
            continue
        own = _rel(g32[name], g64[name])
        tol = max(1e-4, 4.0 * own)
        rel = _rel(p.grad, g64[name])
        print("gradient %s: relative L2 %.3e (float32 mirror %.3e, bar %.1e)" % (name, rel, own, tol))
        if rel > tol:
            failed.append((name, rel, tol))
        worst = max(worst, (rel, name))
        checked += 1
    print("worst gradient: %s %.3e" % (worst[1], worst[0]))
    assert not failed, failed
    assert checked > 40
    sd = net.state_dict()
    for name, v in c["m32"]["after"].items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v) >= 1, name  # (one step per scale: the scales share their PointConv)
        elif "running_" in name:
            torch.testing.assert_close(sd[name].cpu(), v, rtol=1e-4, atol=1e-5, msg=name)


def test_sa_module_with_queries_that_have_no_edge(hip, oracle):
    """PointConv called directly on queries that are not support points: a query without an edge gives exactly 0.0,
    and BatchNorm inside local_nn sees the real edges only (fewer rows than queries have slots)"""
    from torch_points3d_amd.pointnet2_mp import SAModule
    g = torch.Generator().manual_seed(21)
    sizes, qsizes, cap, radius, C = [50, 131], [40, 67], 4, 0.45, 6
    pos_s = torch.rand(sum(sizes), 3, generator=g) * 2 - 1
    pos_q = torch.rand(sum(qsizes), 3, generator=g) * 3 - 1.5
    bs, bq = _batch_of(sizes), _batch_of(qsizes)
    x = torch.randn(sum(sizes), C, generator=g)
    cot = torch.randn(sum(qsizes), 48, generator=g)
    es, col = ref.table_edges(oracle.ball_query(radius, cap, pos_s, pos_q, mode="partial_dense", batch_x=bs, batch_y=bq)[0])
    deg = es[1:] - es[:-1]
    none = deg == 0
    print("standalone SAModule: %d of %d queries without an edge, %d at the cap" % (
        int(none.sum()), deg.numel(), int((deg == cap).sum())))
    assert int(none.sum()) >= 3 and int((deg == cap).sum()) >= 3 and int((~none).sum()) >= 30
    torch.manual_seed(3)
    sa = SAModule(ratio=0.25, radius=radius, radius_num_point=cap, down_conv_nn=[C + 3, 32, 48])
    sd = {k: v.clone() for k, v in sa.state_dict().items()}
    runs = {}
    for dtype in (torch.float32, torch.float64):
        m = ref.SAModule.from_state_dict(sd, dtype)
        xin = x.clone().to(dtype).requires_grad_(True)
        out = m._conv(xin, (pos_s.to(dtype), pos_q.to(dtype)), (es, col))
        (out * cot.to(dtype)).sum().backward()
        runs[dtype] = dict(out=out.detach(), gx=xin.grad, after=m.state_dict())
    m32, m64 = runs[torch.float32], runs[torch.float64]
    sa = sa.to(DEV).train()
    edges = sa.neighbour_finder(pos_s.to(DEV), pos_q.to(DEV), batch_x=bs.to(DEV), batch_y=bq.to(DEV), scale_idx=0)
    assert torch.equal(edges.edge_start.cpu(), es) and torch.equal(edges[1].cpu(), col)
    xg = x.to(DEV).requires_grad_(True)
    out = sa.conv(xg, (pos_s.to(DEV), pos_q.to(DEV)), edges, bs.to(DEV))
    got = out.detach().cpu()
    assert tuple(got.shape) == (sum(qsizes), 48)
    assert not bool(got[none].any()) and not bool(m64["out"][none].any()), "a query without an edge gives 0.0"
    assert bool(got[~none].any(1).all())
    atol = bound(m32["out"], m64["out"].numpy())
    print("standalone SAModule vs the float32 mirror: max %.3e (atol %.1e)" % (_dist(got, m32["out"])[0], atol))
    torch.testing.assert_close(got, m32["out"], rtol=1e-5, atol=atol)
    (out * cot.to(DEV)).sum().backward()
    own = _rel(m32["gx"], m64["gx"])
    rel = _rel(xg.grad, m64["gx"])
    print("standalone SAModule gradient x: relative L2 %.3e (float32 mirror %.3e)" % (rel, own))
    assert rel <= max(1e-4, 4.0 * own), (rel, own)
    after = sa.state_dict()
    for name, v in m32["after"].items():  # statistics over the E edge rows, not over Nq * cap slots
        if "running_" in name:
            torch.testing.assert_close(after[name].cpu(), v, rtol=1e-4, atol=1e-5, msg=name)
        elif name.endswith("num_batches_tracked"):
            assert int(after[name]) == int(v) == 1
