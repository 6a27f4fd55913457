"""The batch-building kernels of csrc/transforms.hip on the device: torchpoints.region_cut / mask_compact /
elastic_distort, and the classes of torch_points3d_amd/transforms.py on device tensors.

References, none of them the kernels: the numpy float64 restatement of the predicates (the same calls on CPU tensors,
which tests/test_transforms_cpu.py pins against brute-force loops, sklearn's KDTree and scipy), and the transform
classes applied cloud by cloud on the host with the same draws.  The region kernels only compare and count, and the
warp is stated operation by operation in double without fma, so every comparison of an operator is torch.equal.
Shapes: around the wave (63, 64, 65), around the row tile (TILE - 1, TILE, TILE + 1, 2 TILE + 1), 1 / 2 / 64 / 65
regions, empty and all-holding regions, empty scenes."""
import numpy as np
import pytest
import torch

from canary import Canary
from torch_points3d_amd import _lib
from torch_points3d_amd import torchpoints as tp
from torch_points3d_amd import transforms as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = tp.region_tile_rows()  # tp3d_region_tile_rows(): the shapes below follow the kernel's tile
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def D(t):
    return None if t is None else torch.as_tensor(t).to(DEV)


def grid_points(rng, N, span=4.0):
    """fp32 points on a lattice of 1/64: differences, squares and their sums are exact, so a point can sit exactly ON a
    radius and many points share coordinates"""
    return (rng.randint(0, int(span * 64), (N, 3)).astype(np.float32) / 64.0)


def same_cut(got, want, with_pos=True):
    assert torch.equal(got.start.cpu(), want.start)
    assert torch.equal(got.status.cpu(), want.status)
    n = min(int(want.status[0]), got.index.shape[0])
    assert want.index.shape[0] == n
    assert torch.equal(got.index[:n].cpu(), want.index)
    if want.batch is not None:
        assert torch.equal(got.batch[:n].cpu(), want.batch)
    if with_pos and want.pos is not None:
        assert torch.equal(got.pos[:n].cpu(), want.pos)  # an fp32 subtraction: bit-equal
    if want.seg is not None:
        assert torch.equal(got.seg.cpu(), want.seg)


def both(pos, centre, param, **kw):
    """(device result, host restatement) of one region_cut"""
    dev_kw = {k: (D(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return tp.region_cut(D(pos), D(centre), D(param) if torch.is_tensor(param) else param, **dev_kw), \
        tp.region_cut(pos, centre, param, **kw)


def test_tile_is_the_documented_one():
    assert _lib.load().tp3d_region_tile_rows() == TILE and TILE % 64 == 0 and TILE >= 256
    assert _lib.ABI_VERSION == 39


@pytest.mark.parametrize("kind", ["sphere", "cylinder", "box", "ellipsoid"])
@pytest.mark.parametrize("B", [1, 2, 64, 65])
def test_region_cut_sizes(kind, B):
    rng = np.random.RandomState(B * 7 + len(kind))
    for N in SIZES:
        pos = torch.from_numpy(grid_points(rng, N))
        centre = torch.from_numpy(grid_points(rng, B))
        param = torch.from_numpy(rng.randint(32, 128, (B, 3)).astype(np.float32) / 64.0)
        rot = None
        if kind in ("box", "ellipsoid"):
            q, _ = np.linalg.qr(rng.randn(B, 3, 3))
            rot = torch.from_numpy(q.astype(np.float32))
        for closed in (False, True):
            got, want = both(pos, centre, param, kind=kind, rot=rot, closed=closed, align_origin=True)
            same_cut(got, want)
            assert got.index.shape[0] == int(want.status[0])  # exact arrays without a capacity
        seg = torch.tensor([0, N // 3, N])
        got, want = both(pos, centre, param, kind=kind, rot=rot, mode="outside_all", seg=seg)
        same_cut(got, want)


def test_empty_full_identical_and_overlapping_regions():
    rng = np.random.RandomState(3)
    N = 2 * TILE + 1
    pos = torch.from_numpy(grid_points(rng, N))
    centre = torch.tensor([[100.0, 100.0, 100.0],  # empty
                           [2.0, 2.0, 2.0],         # holds every row
                           [1.0, 1.0, 1.0], [1.0, 1.0, 1.0],  # identical
                           [1.25, 1.0, 1.0]])       # overlaps the two before
    param = torch.tensor([0.5, 100.0, 1.0, 1.0, 1.0])
    got, want = both(pos, centre, param, closed=True, align_origin=True)
    same_cut(got, want)
    counts = (got.start[1:] - got.start[:-1]).cpu().tolist()
    assert counts[0] == 0 and counts[1] == N and counts[2] == counts[3] > 0 and counts[4] > 0
    assert torch.equal(got.index[got.start[1]:got.start[2]].cpu(), torch.arange(N))
    lists = [set(got.index[got.start[b]:got.start[b + 1]].cpu().tolist()) for b in range(5)]
    assert lists[2] == lists[3] and lists[2] & lists[4] and lists[2] != lists[4]


def test_point_on_the_radius_and_zero_distance():
    # |(3, 4, 12) / 64| = 13 / 64 exactly: the row sits on the sphere of radius 13 / 64, and on the cylinder of 5 / 64
    pos = torch.tensor([[3.0, 4.0, 12.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]) / 64.0
    centre = torch.zeros((1, 3))
    for kind, r in (("sphere", 13.0 / 64.0), ("cylinder", 5.0 / 64.0)):
        for closed, skip_zero in ((False, False), (True, False), (False, True), (True, True)):
            got, want = both(pos, centre, r, kind=kind, closed=closed, skip_zero=skip_zero)
            same_cut(got, want)
            rows = got.index.cpu().tolist()
            assert (0 in rows) == closed          # on the radius: only the closed predicate holds it
            assert (1 in rows) == (not skip_zero)  # the centre itself
            assert 2 in rows
    # a box: a row exactly on the face
    got, want = both(torch.tensor([[0.5, 0.0, 0.0], [0.25, 0.0, 0.0]]), centre, torch.tensor([[0.5, 1.0, 1.0]]), kind="box")
    same_cut(got, want)
    assert got.index.cpu().tolist() == [1]
    got, _ = both(torch.tensor([[0.5, 0.0, 0.0], [0.25, 0.0, 0.0]]), centre, torch.tensor([[0.5, 1.0, 1.0]]), kind="box",
                  closed=True)
    assert got.index.cpu().tolist() == [0, 1]


def test_three_scenes_with_an_empty_one():
    rng = np.random.RandomState(5)
    seg = torch.tensor([0, 1, TILE + 2, TILE + 2])  # scenes of 1, TILE + 1 and 0 rows
    N = TILE + 2
    pos = torch.from_numpy(grid_points(rng, N, span=2.0))
    centre = torch.cat([pos[0:1], pos[5:6], pos[7:8], pos[9:10], pos[0:1]])
    scene = torch.tensor([0, 1, 2, 1, 1])
    got, want = both(pos, centre, 1.5, seg=seg, scene=scene, closed=True, align_origin=True)
    same_cut(got, want)
    counts = (got.start[1:] - got.start[:-1]).cpu().tolist()
    assert counts[0] == 1 and counts[2] == 0 and counts[1] > 1
    idx = got.index.cpu()
    assert all(int(seg[1]) <= i < int(seg[2]) for i in idx[got.start[1]:got.start[2]].tolist())
    assert 0 not in idx[got.start[4]:got.start[5]].tolist()  # region 4 sits on row 0 but names scene 1
    got, want = both(pos, centre, 1.5, seg=seg, scene=scene, mode="outside_all")
    same_cut(got, want)
    # every row of one cloud dropped: scene 0's only row lies in region 0
    assert got.seg.cpu().tolist()[:2] == [0, 0] and int(got.seg[-1]) == got.index.shape[0]
    got, want = both(pos, centre[:1].expand(3, 3).contiguous(), 100.0, seg=seg, scene=torch.tensor([0, 1, 2]),
                     mode="outside_all")
    same_cut(got, want)
    assert got.index.numel() == 0 and got.seg.cpu().tolist() == [0, 0, 0, 0]


def test_capacity_exact_short_and_none():
    rng = np.random.RandomState(6)
    pos = torch.from_numpy(grid_points(rng, 2 * TILE + 1))
    centre = torch.from_numpy(grid_points(rng, 5))
    exact = tp.region_cut(pos, centre, 1.0, closed=True, align_origin=True)
    T = int(exact.status[0])
    assert T > 10
    for cap in (T, T - 1, T + 7, 0):
        with Canary() as guard:
            got = tp.region_cut(D(pos), D(centre), 1.0, closed=True, align_origin=True, capacity=cap)
            guard.check()  # the arrays have guard bands on both sides: nothing was written past `cap` entries
        want = tp.region_cut(pos, centre, 1.0, closed=True, align_origin=True, capacity=cap)
        assert got.index.shape[0] == cap and got.pos.shape[0] == cap and got.batch.shape[0] == cap
        assert got.status.cpu().tolist() == [T, int(T > cap)]
        same_cut(got, want)
    keep = tp.region_cut(pos, centre, 1.0, mode="outside_all")
    K = int(keep.status[0])
    for cap in (K, K - 1):
        with Canary() as guard:
            got = tp.region_cut(D(pos), D(centre), 1.0, mode="outside_all", seg=D(torch.tensor([0, 100, pos.shape[0]])),
                                capacity=cap)
            guard.check()
        want = tp.region_cut(pos, centre, 1.0, mode="outside_all", seg=torch.tensor([0, 100, pos.shape[0]]), capacity=cap)
        same_cut(got, want)
        assert (got.seg.cpu().tolist() == [0, 0, 0]) == (cap < K)


def test_workspace_shrinks_between_calls_and_repeats_are_bit_equal():
    rng = np.random.RandomState(7)
    big = torch.from_numpy(grid_points(rng, 2 * TILE + 1))
    small = torch.from_numpy(grid_points(rng, 65))
    cb, cs = torch.from_numpy(grid_points(rng, 65)), torch.from_numpy(grid_points(rng, 2))
    first = tp.region_cut(D(big), D(cb), 1.0, closed=True)
    got, want = both(small, cs, 1.0, closed=True)  # the same workspace, now mostly stale
    same_cut(got, want)
    again = tp.region_cut(D(big), D(cb), 1.0, closed=True)
    for a, b in zip(first, again):
        assert (a is None and b is None) or torch.equal(a, b)
    same_cut(again, tp.region_cut(big, cb, 1.0, closed=True))


@pytest.mark.parametrize("N", SIZES)
def test_mask_compact(N):
    rng = np.random.RandomState(N)
    seg = torch.tensor([0, N // 3, N // 3, N])
    for density in (0.0, 0.3, 1.0):
        mask = torch.from_numpy(rng.rand(N) < density)
        got, want = tp.mask_compact(D(mask), D(seg)), tp.mask_compact(mask, seg)
        same_cut(got, want)
        assert torch.equal(got.index.cpu(), torch.nonzero(mask)[:, 0])
    got = tp.mask_compact(D(mask.to(torch.float32)))
    assert got.seg is None and torch.equal(got.index.cpu(), torch.nonzero(mask)[:, 0])
    if N > 1:
        cap = N - 1
        got, want = tp.mask_compact(D(mask), D(seg), capacity=cap), tp.mask_compact(mask, seg, capacity=cap)
        same_cut(got, want)
        assert got.status.cpu().tolist() == [N, 1]


# ---------------------------------------------------------------------------------------------------- elastic distortion
def elastic_batch():
    """three clouds: a flat one (3 cells along z), a one-point cloud, a non-cubic one whose first rows sit exactly on the
    first interior and the last axis values"""
    rng = np.random.RandomState(11)
    flat = (rng.rand(300, 3) * np.array([3.0, 2.0, 0.0])).astype(np.float32) + np.float32(1.5)
    one = np.array([[0.25, -1.0, 7.0]], dtype=np.float32)
    box = (rng.rand(2 * TILE + 1, 3) * np.array([5.0, 0.5, 2.25])).astype(np.float32) - np.float32(1.0)
    pos = np.concatenate([flat, one, box])
    seg = np.array([0, 300, 301, 301 + box.shape[0]], dtype=np.int64)
    return torch.from_numpy(pos), torch.from_numpy(seg)


@pytest.mark.parametrize("granularity,magnitude", [(0.2, 0.4), (0.8, 1.6)])
def test_elastic_distort_is_the_float64_evaluation_bit_for_bit(granularity, magnitude):
    """The kernel states the blur and the interpolation operation by operation in double with no fma, so the float64
    evaluation on the host (which tests/test_transforms_cpu.py shows bit-equal to scipy, the reference's own route) is
    matched exactly: equality is asserted, no tolerance is used."""
    pos, seg = elastic_batch()
    want, grids = tp.elastic_distort(pos, seg, granularity, magnitude, generator=torch.Generator().manual_seed(3),
                                     return_grids=True)
    assert grids.dims[0][2] == 3 and len(set(grids.dims[2].tolist())) == 3  # a flat cloud, a non-cubic grid
    noise = torch.randn(int(grids.goff[-1]), generator=torch.Generator().manual_seed(3))
    got = tp.elastic_distort(D(pos), D(seg), granularity, magnitude, noise=D(noise))
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(want, pos)
    again = tp.elastic_distort(D(pos), D(seg), granularity, magnitude, noise=D(noise))
    assert torch.equal(again, got)


def test_elastic_rows_on_the_first_and_last_axis_value():
    # min = 0 and granularity 0.5 (exact in fp32): the axes are -0.5, 0, 0.5, ..., and the rows at the minimum and the
    # maximum of the cloud sit exactly on axis values; the last axis value itself is min + g (dim - 2) >= max
    pos = torch.tensor([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5], [1.0, 0.5, 0.25], [2.0, 0.0, 0.5], [0.5, 1.0, 0.0]])
    seg = torch.tensor([0, 5])
    want, grids = tp.elastic_distort(pos, seg, 0.5, 1.0, generator=torch.Generator().manual_seed(1), return_grids=True)
    assert grids.dims.tolist() == [[7, 5, 4]] and grids.axes[0, 0].tolist() == [-0.5, 0.5, 2.5]
    noise = torch.randn(int(grids.goff[-1]), generator=torch.Generator().manual_seed(1))
    got = tp.elastic_distort(D(pos), D(seg), 0.5, 1.0, noise=D(noise))
    assert torch.equal(got.cpu(), want)
    # The entry points themselves, with rows the wrapper cannot produce (its axes start one cell below the minimum): one
    # exactly on the first axis value, one exactly on the last, and two just outside, which are copied.
    far = pos.clone()
    far[0, 0] = -0.5
    far[1, 0] = 2.5
    far[2, 0] = 2.5 + 2.0 ** -10
    far[3, 2] = -0.5 - 2.0 ** -10
    blurred_host = tp.elastic_blur_numpy(noise.numpy().reshape(7, 5, 4, 3))
    want_far = torch.from_numpy(tp.elastic_apply_numpy(far.numpy(), blurred_host, grids.dims[0], grids.axes[0], 1.0))
    assert torch.equal(want_far[2:4], far[2:4]) and not torch.equal(want_far[:2], far[:2])
    dev = torch.device(DEV)
    dims, goff, axes = (torch.from_numpy(a).to(DEV) for a in grids)
    far_d, seg_d, blurred = D(far), D(seg), D(noise).clone()
    tmp, out = torch.empty_like(blurred), torch.empty_like(far_d)
    _lib.call("tp3d_elastic_blur_f32", _lib.ptr(blurred), _lib.ptr(tmp), _lib.ptr(dims), _lib.ptr(goff), 1, blurred.numel(), 2,
              _lib.stream_ptr(dev))
    assert torch.equal(blurred.cpu(), torch.from_numpy(blurred_host).reshape(-1))
    _lib.call("tp3d_elastic_apply_f32", _lib.ptr(far_d), _lib.ptr(seg_d), 1, 5, _lib.ptr(blurred), _lib.ptr(dims),
              _lib.ptr(goff), _lib.ptr(axes), 1.0, _lib.ptr(out), _lib.stream_ptr(dev))
    assert torch.equal(out.cpu(), want_far)


# ---------------------------------------------------------------------------------------------------- the classes
import transforms_cases as tc  # noqa: E402


@pytest.mark.parametrize("name", tc.NAMES)
def test_class_against_the_reference_fixture(name):
    """every class on device tensors through `apply` with the reference's recorded draws (tests/golden/transforms.npz)"""
    tc.check(name, DEV)


# ---------------------------------------------------------------------------------------------------- SceneSampler
def two_areas():
    from torch_points3d_amd.dense import Data
    rng = np.random.RandomState(21)
    areas = []
    for n, span in ((3 * TILE + 5, 3.0), (TILE - 7, 2.0)):
        areas.append(Data(pos=D(grid_points(rng, n, span)), y=D(rng.randint(0, 4, n)), x=D(rng.randn(n, 2).astype(np.float32))))
    return areas


def test_scene_sampler_batch_is_sphere_sampling_per_drawn_centre():
    areas = two_areas()
    for kind, cls in (("sphere", TR.SphereSampling), ("cylinder", TR.CylinderSampling)):
        s = TR.SceneSampler(areas, radius=0.5, kind=kind, sample_per_epoch=8)
        batch = s.sample(6, torch.Generator().manual_seed(4))
        assert batch.centre.shape == (6, 3) and int(batch.cut.status[1]) == 0
        assert torch.equal(batch.centre_label, s.centres[:, 4].long()[s.draw(6, torch.Generator().manual_seed(4))["row"].to(DEV)])
        for b in range(6):
            row = s.draw(6, torch.Generator().manual_seed(4))["row"][b]
            area = int(s.centres[row, 3])
            one = cls(0.5, batch.centre[b].cpu(), align_origin=False)(areas[area])  # the reference's _get_random
            m = batch.batch == b
            assert int(m.sum()) == one.pos.shape[0] > 0
            assert torch.equal(batch.pos[m], one.pos) and torch.equal(batch.y[m], one.y) and torch.equal(batch.x[m], one.x)
            inside = tp.region_holds_numpy(areas[area].pos.cpu().numpy(), batch.centre[b].cpu().numpy(),
                                           np.full(3, 0.5, np.float32), None, kind, True, False)
            assert torch.equal((batch.origin_id[m] - s.seg[area]).cpu(), torch.from_numpy(np.nonzero(inside)[0]))
    grid = TR.SceneSampler(areas, radius=1.0, kind="sphere", sample_per_epoch=-1)
    seen = 0
    for out in grid.test_batches(max_clouds=16):
        assert out.center_label.shape[0] == out.centre.shape[0] <= 16 and torch.equal(out.pos, grid.data.pos[out.origin_id])
        seen += out.centre.shape[0]
    assert seen >= 8


def test_scene_sampler_with_a_capacity_waits_for_the_host_at_most_once():
    import warnings
    s = TR.SceneSampler(two_areas(), radius=0.5, kind="sphere", sample_per_epoch=8)
    params = s.draw(4, torch.Generator().manual_seed(9))
    exact = s.apply(params)
    T = int(exact.cut.status[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fitted = s.apply(params, capacity=T + 100)
            short = s.apply(params, capacity=T - 1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    print("host synchronisations of two sample() calls with a capacity: %d" % len(syncs))
    assert len(syncs) <= 1
    assert fitted.cut.status.cpu().tolist() == [T, 0] and short.cut.status.cpu().tolist() == [T, 1]
    assert fitted.pos.shape[0] == T + 100
    for key in ("pos", "y", "x", "origin_id", "batch"):
        assert torch.equal(getattr(fitted, key)[:T], getattr(exact, key)), key
        assert torch.equal(getattr(short, key), getattr(exact, key)[:T - 1]), key


def test_drawn_centres_on_device_bags_are_the_host_ones():
    """CubeCrop, RandomSphereDropout and IrregularSampling take their centre from one point per occupied voxel.  With the
    same draws the device bag (voxel_cluster) and the host bag (the numpy grouping) must choose the same points, so
    the same rows survive; __call__ with a seeded generator is then repeatable."""
    data = tc.bag(tc.CLOUDS, "cpu")
    dev = tc.bag(tc.CLOUDS, DEV)
    for t in (TR.CubeCrop(c=0.4, grid_size_center=0.05), TR.RandomSphereDropout(num_sphere=3, radius=0.3, grid_size_center=0.05),
              TR.IrregularSampling(d_half=0.6, grid_size_center=0.1)):
        params = t.draw(2, torch.Generator().manual_seed(5))
        if isinstance(t, TR.IrregularSampling):
            params["point_u"] = torch.rand(data.pos.shape[0], generator=torch.Generator().manual_seed(6))
        want, got = t.apply(data, params), t.apply(dev, params)
        assert 0 < want.ids.shape[0] < data.ids.shape[0]
        assert torch.equal(got.ids.cpu(), want.ids) and torch.equal(got.batch.cpu(), want.batch)
        one, two = t(dev, torch.Generator().manual_seed(8)), t(dev, torch.Generator().manual_seed(8))
        assert torch.equal(one.ids, two.ids)
