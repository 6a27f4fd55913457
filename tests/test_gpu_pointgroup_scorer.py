"""PointGroup's sparse scorers on the GPU: sparse tensors with more than 2^9 clouds (csrc/sparseconv.hip,
tp3d_sparse_set_build_clouds_i32), the cluster voxel mean with its gradient (csrc/cluster_voxel.hip,
torchpoints.cluster_voxelize), the innermost max of the encoder, and scorer_type "unet" / "encoder" of
torch_points3d_amd.pointgroup.PointGroup against the reference-generated fixtures and the float64 restatement
tests/pointgroup_scorer_ref.py.

Bars (those of tests/test_gpu_ppnet.py and tests/test_gpu_ms_svconv.py): outputs rtol 1e-5 / atol 1e-5 * max(1, |ref|max),
gradients rtol 1e-4 / atol 1e-5 * |ref|max, each relaxed to twice the fp32 reference's own distance to float64 (_close64).
Every comparison prints both distances."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import pointgroup_scorer_ref as psr
import pointgroup_util as pgu
import sparseconv_ref as sr
from test_gpu_ppnet import _close64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sc():
    from torch_points3d_amd import sparseconv
    return sparseconv


@pytest.fixture(scope="module")
def tp():
    from torch_points3d_amd import torchpoints
    return torchpoints


@pytest.fixture(scope="module")
def pg():
    from torch_points3d_amd import pointgroup
    return pointgroup


class HostReads(object):
    """counts Tensor.cpu / .item / .tolist / .numpy / .to(cpu) on device tensors while active"""

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name in ("cpu", "item", "tolist", "numpy", "to"):
            self._saved[name] = getattr(torch.Tensor, name)
            setattr(torch.Tensor, name, self._wrap(name, self._saved[name]))
        return self

    def _wrap(self, name, fn):
        def counted(t, *a, **k):
            target = name != "to" or any(str(v).startswith("cpu") for v in list(a) + list(k.values())
                                         if isinstance(v, (str, torch.device)))
            if t.is_cuda and target:
                self.count += 1
            return fn(t, *a, **k)
        return counted

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(torch.Tensor, name, fn)
        return False


# ---------------------------------------------------------------------------------------------------------- many clouds
K_CLOUDS = 70000
NAMED = [0, 511, 512, 513, 65535, 65536, 65537, K_CLOUDS - 1]


@functools.lru_cache(maxsize=None)
def many_clouds():
    """(C (N, 4) int32 rows [x, y, z, cloud] in shuffled order): the named clouds and 300 others, each a clump of 1-8 voxels
    inside a 2 x 2 x 2 block somewhere in a box of 4 000 cells; clouds 511, 512 and 65536 hold the SAME clump at the same
    place, and three more clouds hold clumps that touch it"""
    rng = np.random.RandomState(3)
    clouds = sorted(set(NAMED) | set(rng.choice(K_CLOUDS, 300, replace=False).tolist()))
    cell = pgu._box((0, 0, 0), (2, 2, 2))
    shared = np.asarray([100, -200, 300]) + cell[rng.permutation(8)[:5]]
    rows = []
    for i, c in enumerate(clouds):
        if c in (511, 512, 65536):
            v = shared
        elif i % 100 == 7:  # next to the shared clump, in a cloud of its own: a neighbour by xyz alone
            v = np.asarray([102, -200, 300]) + cell[rng.permutation(8)[:3]]
        else:
            v = rng.randint(-2000, 2000, size=3) + cell[rng.permutation(8)[:rng.randint(1, 9)]]
        rows.append(np.concatenate([v, np.full((len(v), 1), c)], 1))
    rows = np.concatenate(rows)
    C = torch.from_numpy(rows[rng.permutation(len(rows))]).int()
    assert set(NAMED) <= set(C[:, 3].tolist()) and len(C) > 1024
    return C


@pytest.mark.parametrize("ksize,stride", [(3, 1), (3, 2), (2, 2)])
def test_many_clouds_sets_and_kernel_maps(sc, ksize, stride):
    C = many_clouds()
    st = sc.SparseTensor(torch.zeros(len(C), 1, device=DEV), C.to(DEV), clouds=K_CLOUDS)
    km = st._kmap(ksize, 1, stride)
    C_out = C if stride == 1 else sr.down_coords(C, stride)
    if stride > 1:
        assert torch.equal(st.cmaps[stride].coords.cpu(), C_out)
    fwd, inv = sr.kernel_map(C, C_out, ksize, 1)
    assert torch.equal(km.forward.cpu(), fwd) and torch.equal(km.inverse.cpu(), inv)
    # the shared clump is not linked across its three clouds: every hit of a row lies in the row's own cloud
    hit = km.forward.cpu().long()
    own = C_out[:, 3:4].expand_as(hit)
    assert torch.equal(C[:, 3][hit.clamp(min=0)][hit >= 0], own[hit >= 0])


def test_many_clouds_convolution_and_its_transpose(sc):
    C = many_clouds()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(len(C), 4, generator=g)
    torch.manual_seed(1)
    down = sc.Conv3d(4, 4, kernel_size=3, stride=2).to(DEV)
    up = sc.Conv3dTranspose(4, 4, kernel_size=3, stride=2).to(DEV)
    C2 = sr.down_coords(C, 2)
    fwd, inv = sr.kernel_map(C, C2, 3, 1)
    cot = torch.randn(len(C), 4, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    mid = down(sc.SparseTensor(xg, C.to(DEV), clouds=K_CLOUDS))
    assert mid.clouds == K_CLOUDS and mid.s == 2
    out = up(mid)
    assert out.clouds == K_CLOUDS and out.s == 1
    (out.F * cot.to(DEV)).sum().backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.to(dt).clone().requires_grad_(True)  # (a leaf of its own: .to(float32) alone returns x)
        wd, wu = (m.kernel.detach().cpu().to(dt).requires_grad_(True) for m in (down, up))
        m_ref = sr.conv_by_table(xr, fwd, wd)
        o_ref = sr.conv_by_table(m_ref, inv, wu)
        (o_ref * cot.to(dt)).sum().backward()
        ref[dt] = dict(mid=m_ref.detach(), out=o_ref.detach(), dx=xr.grad, dwd=wd.grad, dwu=wu.grad)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    _close64(mid.F, r32["mid"], r64["mid"], 1e-5, 1e-5, 1.0, "strided output")
    _close64(out.F, r32["out"], r64["out"], 1e-5, 1e-5, 1.0, "transposed output")
    _close64(xg.grad, r32["dx"], r64["dx"], 1e-4, 1e-5, what="dX")
    _close64(down.kernel.grad, r32["dwd"], r64["dwd"], 1e-4, 1e-5, what="dW (strided)")
    _close64(up.kernel.grad, r32["dwu"], r64["dwu"], 1e-4, 1e-5, what="dW (transposed)")


def test_cloud_bound_is_opt_in(sc):
    C = torch.tensor([[0, 0, 0, 0], [1, 2, 3, 512]], dtype=torch.int32, device=DEV)
    x = torch.zeros(2, 1, device=DEV)
    with pytest.raises(ValueError, match="out of range"):
        sc.SparseTensor(x, C)._set(1)
    with pytest.raises(ValueError, match="out of range"):
        sc.SparseTensor(x, C, clouds=512)._set(1)
    st = sc.SparseTensor(x, C, clouds=513)
    assert st._set(1).n == 2 and st._kmap(3, 1, 2).n_out == 2
    # a box whose extent times the clouds passes the 64-bit key
    top = sc.CLOUD_LIMIT_MAX
    m = sc.COORD_LIMIT - 1
    wide = torch.tensor([[-m, -m, -m, 0], [m, m, m, top - 1]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="span too large"):
        sc.SparseTensor(x, wide, clouds=top)._set(1)
    with pytest.raises(ValueError, match="clouds must be"):
        sc.SparseTensor(x, C, clouds=top + 1)


# ------------------------------------------------------------------------------------------------------------ voxel mean
SIZE = 0.05
RUNS = [1, 2, 63, 64, 65, 129, 1025]  # slots per voxel: the 64-slot seam and the 16-piece seams


@functools.lru_cache(maxsize=None)
def voxel_case():
    """Clusters over 2 600 points.  Cluster 0: one voxel of one slot.  Clusters 1-3: the voxels of RUNS slots, spread over
    them, plus scattered single-slot voxels.  Cluster 4 repeats 40 points of cluster 1 (a point in two clusters, in the
    same xyz voxel of both).  Cluster 5 lists one of its points twice (twice in one voxel).  The last 100 points belong to
    no cluster.  Every pos / SIZE is at least 0.2 from a half-integer."""
    rng = np.random.RandomState(9)
    pos, clusters = [], [[] for _ in range(6)]

    def add(cluster, voxel, count):
        for _ in range(count):
            clusters[cluster].append(len(pos))
            pos.append((np.asarray(voxel) + rng.uniform(-0.3, 0.3, size=3)) * SIZE)

    add(0, (5, 5, 5), 1)
    for i, n in enumerate(RUNS):
        add(1 + i % 3, (10 + 2 * i, -3, 7 - i), n)
    for c in (1, 2, 3):
        for j in range(60):
            add(c, (-20 + j, 4 * c, -j // 7), 1)
    clusters[4] = clusters[1][:40] + []
    add(4, (40, 40, 40), 3)
    add(5, (-7, -7, -7), 4)
    clusters[5].append(clusters[5][1])
    for _ in range(100):
        pos.append(rng.uniform(-3, 3, size=3))
    pos = torch.from_numpy(np.asarray(pos, dtype=np.float32))
    q = pos.double() / SIZE
    inside = torch.cat([torch.tensor(c) for c in clusters]).unique()
    assert float((q[inside] - torch.floor(q[inside]) - 0.5).abs().min()) >= 0.19
    for c in clusters[1:4]:  # shuffled member order: slots of one voxel are not consecutive
        rng.shuffle(c)
    return pos, [torch.tensor(c, dtype=torch.int64) for c in clusters]


def _voxelize(tp, x, ld, rows=None):
    pos, clusters = voxel_case()
    cs = tp.ClusterSet.from_list(clusters, device=DEV)
    N = pos.shape[0]
    C = x.shape[1]
    wide = torch.full((N, ld), float("nan"), device=DEV)
    wide[:, :C] = x.to(DEV)
    xg = wide[:, :C].detach().requires_grad_(True) if ld > C else x.to(DEV).clone().requires_grad_(True)
    if ld > C:
        assert xg.stride(0) == ld
    with HostReads() as reads:
        st, starts = tp.cluster_voxelize(cs, xg, pos.to(DEV), SIZE)
    return cs, xg, st, starts, reads.count


@pytest.mark.parametrize("C,ld", [(1, 1), (3, 3), (4, 4), (5, 5), (96, 96), (97, 97), (96, 100), (4, 7)])
def test_voxel_mean_forward_and_gradient(tp, C, ld):
    pos, clusters = voxel_case()
    N, K = pos.shape[0], len(clusters)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, generator=g)
    cs, xg, st, starts, reads = _voxelize(tp, x, ld)
    assert reads == 2, "cluster_voxelize made %d device-to-host reads" % reads  # (the two of voxel_cluster)
    assert st.clouds == K and st.s == 1 and st.C.dtype == torch.int32 and starts.dtype == torch.int64

    members, owner = cs.members.cpu(), cs.member_cluster.cpu()
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.to(dt).clone().requires_grad_(True)  # (a leaf of its own: .to(float32) alone returns x)
        Cr, sr_, slot_voxel, feats = psr.voxelize_ref(members, owner, K, xr, pos, SIZE)
        ref[dt] = (Cr, sr_, slot_voxel, feats, xr)
    Cr, starts_ref, slot_voxel, f64, x64 = ref[torch.float64]
    counts = torch.bincount(slot_voxel)
    assert set(RUNS) <= set(counts.tolist()) and int(starts_ref[1]) == 1  # the seams are there; cluster 0 is one voxel
    assert torch.equal(st.C.cpu().long(), Cr) and torch.equal(starts.cpu(), starts_ref)
    cot = torch.randn(f64.shape, generator=g)
    (st.F * cot.to(DEV)).sum().backward()
    for dt in ref:
        (ref[dt][3] * cot.to(dt)).sum().backward()
    _close64(st.F, ref[torch.float32][3].detach(), f64.detach(), 1e-5, 1e-5, 1.0, "voxel mean")
    _close64(xg.grad, ref[torch.float32][4].grad, x64.grad, 1e-4, 1e-5, what="d mean / d x")
    outside = torch.ones(N, dtype=torch.bool)
    outside[members] = False
    assert int(outside.sum()) == 100
    got = xg.grad.cpu()
    assert bool((got[outside] == 0.0).all()) and not bool(torch.signbit(got[outside]).any())  # exactly +0.0
    # repeats are bit-equal
    _, xg2, st2, starts2, _ = _voxelize(tp, x, ld)
    (st2.F * cot.to(DEV)).sum().backward()
    assert torch.equal(st2.F, st.F) and torch.equal(xg2.grad, xg.grad) and torch.equal(starts2, starts)


def test_no_voxel_size_keeps_the_member_slots(tp):
    pos, clusters = voxel_case()
    cs = tp.ClusterSet.from_list(clusters[:4], device=DEV)  # (clusters without a repeated point)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(pos.shape[0], 6, generator=g).to(DEV).requires_grad_(True)
    coords = torch.round(pos / 0.01).int().to(DEV)
    with HostReads() as reads:
        st, starts = tp.cluster_voxelize(cs, x, pos.to(DEV), None, coords)
    assert reads.count == 0
    assert torch.equal(starts, cs.starts) and st.clouds == 4
    assert torch.equal(st.C[:, :3], coords[cs.members]) and torch.equal(st.C[:, 3].long(), cs.member_cluster)
    assert torch.equal(st.F.detach(), x.detach()[cs.members])
    st.F.sum().backward()
    assert torch.equal(x.grad, torch.bincount(cs.members, minlength=x.shape[0]).float()[:, None].expand_as(x))
    with pytest.raises(ValueError, match="coords"):
        tp.cluster_voxelize(cs, x, pos.to(DEV), 0)


def test_voxel_mean_holds_no_slot_rows(tp):
    """E = 2^17 member slots, C = 96: forward + backward allocate less than one (E, C) fp32 buffer beyond their inputs
    and outputs; the plain composition (x[members], index_add_, divide) holds the gathered rows and their gradient"""
    E, C, N, per = 1 << 17, 96, 1 << 16, 64
    g = torch.Generator().manual_seed(4)
    pos = (torch.rand(N, 3, generator=g) * 3.0).to(DEV)
    members = torch.cat([torch.randperm(N, generator=g), torch.randperm(N, generator=g)]).to(DEV)  # every point in two clusters
    starts = (torch.arange(E // per + 1) * per).to(DEV)
    cs = tp.ClusterSet(members, starts)
    x = torch.randn(N, C, generator=g).to(DEV).requires_grad_(True)
    slot_bytes = E * C * 4

    def peak(run):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        cot = torch.ones_like(out)
        out.backward(cot)
        torch.cuda.synchronize()
        held = out.numel() * 4 * 2 + x.grad.numel() * 4  # the output, its cotangent, the gradient
        extra = torch.cuda.max_memory_allocated() - base - held
        x.grad = None
        return extra

    fused = peak(lambda: tp.cluster_voxelize(cs, x, pos, SIZE)[0].F)

    def composition():
        _, _, slot_voxel, feats = psr.voxelize_ref(cs.members, cs.member_cluster, len(cs), x, pos, SIZE)
        return feats

    plain = peak(composition)
    print("peak beyond inputs and outputs: fused %.1f MB, composition %.1f MB, one (E, C) buffer %.1f MB"
          % (fused / 1e6, plain / 1e6, slot_bytes / 1e6))
    assert fused < slot_bytes


# ------------------------------------------------------------------------------------------------- innermost max / encoder
ENCODER = dict(down_conv=dict(down_conv_nn=[[4, 8], [8, 16]], kernel_size=3, stride=2, N=1),
               innermost=dict(aggr="max", nn=[16, 8], activation=dict(name="LeakyReLU", negative_slope=0.2)))


def test_global_max_against_float64(sc):
    g = torch.Generator().manual_seed(8)
    clouds = 700
    batch = torch.sort(torch.randint(0, clouds, (3000,), generator=g))[0]
    batch[batch == 13] = 14  # a cloud without rows
    x = torch.randn(3000, 16, generator=g)
    torch.manual_seed(3)
    m = sc._GlobalMax([16, 8], 0.2).to(DEV).eval()
    with torch.no_grad():
        m.nn[0][1].batch_norm.running_mean.normal_()
        m.nn[0][1].batch_norm.running_var.uniform_(0.5, 2.0)
    ref = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(m).cpu().to(dt).nn(x.to(dt)).detach()
        out = torch.zeros(clouds, 8, dtype=dt)
        ref[dt] = out.scatter_reduce(0, batch[:, None].expand_as(h), h, "amax", include_self=False)
    with HostReads() as reads:
        got = m(x.to(DEV), batch.to(DEV), clouds)
        perm = torch.randperm(3000, generator=g).to(DEV)
        shuffled = m(x.to(DEV)[perm], batch.to(DEV)[perm], clouds, ordered=False)
    assert reads.count == 0
    _close64(got, ref[torch.float32], ref[torch.float64], 1e-5, 1e-5, 1.0, "max per cloud")
    assert bool((got[13] == 0).all()) and torch.equal(shuffled, got)


def test_encoder_with_clouds_reads_nothing_back(sc, tp):
    pos, clusters = voxel_case()
    cs = tp.ClusterSet.from_list(clusters, device=DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(pos.shape[0], 4, generator=g).to(DEV)
    st, starts = tp.cluster_voxelize(cs, x, pos.to(DEV), SIZE)
    torch.manual_seed(2)
    enc = sc.SparseConv3dEncoder(ENCODER, 4).to(DEV).eval()
    assert isinstance(enc.inner_modules[0], sc._GlobalMax) and enc.output_nc == 8
    first = enc(st, clouds=len(cs))  # builds the coordinate sets of strides 1, 2, 4: one read each
    with HostReads() as reads:
        again = enc(st, clouds=len(cs))
        default = enc(st)  # a tensor built with clouds=K brings its K along
    assert reads.count == 0 and torch.equal(again, first) and torch.equal(default, first)
    assert first.shape == (len(cs), 8)
    # against the rows of the last stage, in float64
    data = st
    for down in enc.down_modules:
        data = down(data)
    assert data.s == 4 and data.clouds == len(cs)
    owner = data.C[:, 3].long().cpu()
    assert bool((owner[1:] >= owner[:-1]).all())  # the rows of a strided set ascend by cloud
    ref = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(enc.inner_modules[0]).cpu().to(dt).nn(data.F.detach().cpu().to(dt)).detach()
        ref[dt] = torch.zeros(len(cs), 8, dtype=dt).scatter_reduce(0, owner[:, None].expand_as(h), h, "amax", include_self=False)
    _close64(first, ref[torch.float32], ref[torch.float64], 1e-5, 1e-5, 1.0, "encoder output")


# ----------------------------------------------------------------------------------------- end to end, more than 512 clusters
def _lattice_scene():
    """two clouds of 18 x 18 x 1 blocks of 2 x 2 x 2 lattice points (step H, jitter H / 64), blocks 4 steps apart: 648 blocks"""
    rng = np.random.RandomState(12)
    block = pgu._box((0, 0, 0), (2, 2, 2))
    origins = pgu._box((0, 0, 0), (18, 18, 1)) * 4
    coords = (origins[:, None, :] + block[None, :, :]).reshape(-1, 3)
    coords = np.concatenate([coords, coords])
    batch = np.repeat([0, 1], len(coords) // 2)
    pos = (coords * pgu.H + rng.uniform(-pgu.H / 64, pgu.H / 64, size=coords.shape)).astype(np.float32)
    pgu.check_margins(pos, batch, pgu.RADIUS, pgu.NSAMPLE)
    return coords, batch, pos


@pytest.mark.parametrize("scorer_type", ["unet", "encoder"])
def test_pointgroup_scores_more_than_512_clusters(pg, tp, sc, monkeypatch, scorer_type):
    from test_gpu_region_grow import two_level_unet
    coords, batch, pos = _lattice_scene()
    n = len(pos)
    rng = np.random.RandomState(13)
    data = types.SimpleNamespace(x=torch.from_numpy(rng.randn(n, 4).astype(np.float32)).to(DEV),
                                 coords=torch.from_numpy(coords).int().to(DEV), batch=torch.from_numpy(batch).long().to(DEV),
                                 pos=torch.from_numpy(pos).to(DEV))
    inst = torch.from_numpy((1 + coords[:, 0] // 8 + 9 * (coords[:, 1] // 8)).astype(np.int64))  # 2 x 2 blocks per instance
    labels = pg.PanopticLabels(center_label=None, y=torch.from_numpy(rng.randint(-1, 5, size=n)).long().to(DEV),
                               num_instances=None, instance_labels=inst.to(DEV), instance_mask=(inst > 0).to(DEV),
                               vote_label=torch.from_numpy(rng.randn(n, 3).astype(np.float32)).to(DEV))

    def small_clusters(pos_, votes, labels_, batch_, stuff, radius):
        """PointGroup._cluster with min_cluster_size 4 and every point of one thing class: the blocks are the clusters of
        the positions; the votes of an untrained Offset head give what they give"""
        one = torch.ones_like(labels_)
        on_pos = tp.region_grow_csr(pos_, one, batch_, ignore_labels=stuff, radius=radius, min_cluster_size=4)
        on_votes = tp.region_grow_csr(votes, one, batch_, ignore_labels=stuff, radius=radius, nsample=200, min_cluster_size=4)
        both = tp.ClusterSet.cat([on_pos, on_votes])
        kind = torch.zeros(len(both), dtype=torch.uint8, device=pos_.device)
        kind[len(on_pos):] = 1
        return both, kind

    monkeypatch.setattr(pg, "cluster", small_clusters)
    torch.manual_seed(0)
    f = 8
    cfg = pg._scorer_config(scorer_type, f, 1)
    net = pg.PointGroup(4, 5, stuff_classes=[0], backbone=two_level_unet(4, f), scorer_type=scorer_type,
                        cluster_radius_search=pgu.RADIUS, cluster_voxel_size=1.5 * pgu.H,
                        **{"scorer_" + scorer_type: cfg}).to(DEV).train()
    seen = []
    net.Backbone.register_forward_hook(lambda m, a, out: seen.append(out))
    out = net(data)
    K = len(out.clusters)
    assert K >= 600 and out.cluster_scores.shape == (K,)
    scores = out.cluster_scores.detach()
    assert bool((scores > 0).all()) and bool((scores < 1).all())
    losses = net.compute_loss(labels)
    assert all(torch.isfinite(v).all() for v in losses.values())
    losses["loss"].backward()
    for name, p in net.named_parameters():
        if name.startswith("ScorerMLP"):
            assert p.grad is None, name  # built for the reference's state_dict, not on this scorer's path
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) > 0, name
    # the score loss alone reaches the backbone's first convolution through the voxel mean
    first = net.Backbone.down_modules[0].conv_in[0].kernel
    (g_first,) = torch.autograd.grad(net(data).cluster_scores.sum(), first)
    assert bool(torch.isfinite(g_first).all()) and int(torch.count_nonzero(g_first)) > 0
    # the same model on the float64 dense per-cluster restatement, from the backbone features of the first pass
    feats = seen[0].detach()
    size = net.cluster_voxel_size
    ref32 = psr.scorer_scores_ref(net, scorer_type, out.clusters, feats, data.pos, size, torch.float32)
    ref64 = psr.scorer_scores_ref(net, scorer_type, out.clusters, feats, data.pos, size, torch.float64)
    _close64(scores, ref32, ref64, 1e-5, 1e-5, 1.0, "cluster scores (%s, %d clusters)" % (scorer_type, K))


# ------------------------------------------------------------------------------------------- the reference-generated fixtures
def _bar(got, ref32, ref64, what):
    """the bar of tests/test_gpu_ms_svconv.py: rtol 1e-5, atol 1e-5 max(1, |ref64|max), relaxed to twice the reference's own
    fp32-to-float64 distance; the measured ratio goes to the parity report"""
    import golden_util
    r64 = torch.as_tensor(ref64).double()
    own = float((torch.as_tensor(ref32).double() - r64).abs().max())
    err = float((got.detach().cpu().double().reshape(r64.shape) - r64).abs().max())
    ratio = err / max(1e-5 * max(1.0, float(r64.abs().max())), 2.0 * own)
    print("%s: error / bar = %.3g" % (what, ratio))
    golden_util.report("pointgroup_scorer", what, ratio)
    _close64(got.reshape(r64.shape), ref32, ref64, 1e-5, 1e-5, floor=1.0, what=what)


@pytest.mark.parametrize("kind", psr.KINDS)
def test_fixture_passes(pg, kind):
    """scorer_type "unet" / "encoder" with the reference's weights on the reference's clusters: cluster scores, the voxel
    rows, running statistics, the gradient wrt the backbone features and every parameter gradient, against the reference's
    fp32 pass and its float64 pass (tests/golden/README_pointgroup.md)"""
    g = psr.load_fixture(kind)
    numbers = psr.fixture_numbers()["fixture"]

    class Backbone(torch.nn.Module):
        output_nc = numbers["in_feat"]

    net = pg.PointGroup(3, 5, backbone=Backbone(), scorer_type=kind, cluster_voxel_size=numbers["size"],
                        **{"scorer_" + kind: numbers[kind]})
    state = psr.fixture_state(g)
    loaded = net.load_state_dict(state, strict=False)
    assert not loaded.unexpected_keys and all(k.startswith(("ScorerMLP.", "Offset.", "Semantic.")) for k in loaded.missing_keys)
    net = net.to(DEV).train()
    net.input = types.SimpleNamespace(pos=g["pos"].to(DEV), coords=g["coords"].to(DEV))
    x = g["x"].to(DEV).requires_grad_(True)
    clusters = psr.fixture_clusters(g, DEV)
    seen = []
    scorer = net.ScorerUnet if kind == "unet" else net.ScorerEncoder
    scorer.register_forward_pre_hook(lambda m, a: seen.append(a[0]))
    with HostReads() as reads:
        scores = net._compute_score(clusters, x, None)
    assert reads.count == 2 + 3  # voxel_cluster's two, and one for each of the coordinate sets of strides 1, 2, 4
    (scores * g["cot"].to(DEV)).sum().backward()
    voxels = seen[0]
    assert torch.equal(voxels.C[:, :3].cpu(), g["voxel_coords"].int()) and torch.equal(voxels.C[:, 3].cpu().long(), g["voxel_batch"])
    t = kind + " "
    _bar(voxels.F, g["voxel_x"], g["f64/voxel_x"], t + "voxel rows")
    _bar(scores, g["scores"], g["f64/scores"], t + "scores")
    _bar(x.grad, g["grad_x"], g["f64/grad_x"], t + "grad backbone features")
    checked = 0
    for name, p in net.named_parameters():
        if name not in state:
            assert p.grad is None, name
            continue
        want64 = g["f64/pgrad/" + name].double()  # (the float64 pass's gradient, stored rounded to fp32)
        own = float(np.asarray(g["pgrad_own/" + name]).reshape(-1)[0])  # |the reference's fp32 gradient - its float64 gradient|max
        assert p.grad is not None, name
        _bar(p.grad, want64 + own, want64, t + "grad " + name)
        checked += 1
    assert checked == sum(1 for k in g if k.startswith("f64/pgrad/"))
    for k, v in net.state_dict().items():
        if "running_" in k and k in state:
            _bar(v, g["after/" + k], g["f64/after/" + k], t + k)
