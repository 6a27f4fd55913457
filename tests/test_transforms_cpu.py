"""The host side of the batch builder: the numpy restatements inside torchpoints.region_cut / mask_compact /
elastic_distort (what CPU tensors take, and what tests/test_gpu_transforms.py holds the kernels to), and the classes of
torch_points3d_amd/transforms.py on CPU bags.

References, none of them the code under test: serial Python loops over Python floats (IEEE double, one rounding per
operation) written here, sklearn's KDTree.query_radius, an evaluation of the warp with scipy's correlate1d and interpn
written from the operator's description, per-cloud torch expressions for the pose classes, and the recorded results of
the reference's own classes in tests/golden/transforms.npz (tests/golden/README_transforms.md).  sklearn and scipy are
imported at module level: without them the file fails to import rather than dropping checks silently."""
import math
import os

import numpy as np
import pytest
import scipy.interpolate
import scipy.ndimage
import sklearn.neighbors
import torch

from torch_points3d_amd import _lib
from torch_points3d_amd import torchpoints as tp
from torch_points3d_amd import transforms as TR
from torch_points3d_amd.dense import Data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transforms.npz")


def lattice(rng, N, span=4.0):
    return rng.randint(0, int(span * 64), (N, 3)).astype(np.float32) / 64.0


def holds_serial(p, c, h, R, kind, closed, skip_zero):
    """the predicate for one point, in Python floats"""
    dx, dy, dz = float(p[0]) - float(c[0]), float(p[1]) - float(c[1]), float(p[2]) - float(c[2])
    d2 = dx * dx + dy * dy
    if kind != "cylinder":
        d2 = d2 + dz * dz
    if skip_zero and d2 == 0.0:
        return False
    if kind in ("sphere", "cylinder"):
        r2 = float(h[0]) * float(h[0])
        return d2 <= r2 if closed else d2 < r2
    q = [dx, dy, dz]
    if R is not None:
        q = [(float(R[i][0]) * dx + float(R[i][1]) * dy) + float(R[i][2]) * dz for i in range(3)]
    if kind == "box":
        return all((abs(q[i]) <= float(h[i])) if closed else (abs(q[i]) < float(h[i])) for i in range(3))
    v = ((q[0] * q[0]) / (float(h[0]) * float(h[0])) + (q[1] * q[1]) / (float(h[1]) * float(h[1]))) \
        + (q[2] * q[2]) / (float(h[2]) * float(h[2]))
    return v <= 1.0 if closed else v < 1.0


def test_header_declares_the_entry_points_at_abi_39():
    for name in ("tp3d_region_tile_rows", "tp3d_region_workspace_bytes", "tp3d_region_count_f32", "tp3d_region_emit_f32",
                 "tp3d_elastic_blur_f32", "tp3d_elastic_apply_f32"):
        assert name in _lib.FUNCTIONS
    assert _lib.ABI_VERSION == 39
    assert len(_lib.SIGNATURES["tp3d_region_count_f32"]) == 19 and len(_lib.SIGNATURES["tp3d_region_emit_f32"]) == 22


@pytest.mark.parametrize("kind", ["sphere", "cylinder", "box", "ellipsoid"])
@pytest.mark.parametrize("closed,skip_zero", [(False, False), (True, False), (False, True), (True, True)])
def test_region_cut_against_serial_loops(kind, closed, skip_zero):
    rng = np.random.RandomState(len(kind) + 2 * closed + skip_zero)
    N, B = 257, 5
    pos = lattice(rng, N, 2.0)
    centre = np.concatenate([pos[:2], lattice(rng, B - 2, 2.0)])  # two centres ON a point: zero distances
    param = rng.randint(32, 96, (B, 3)).astype(np.float32) / 64.0
    rot = None
    if kind in ("box", "ellipsoid"):
        rot = np.linalg.qr(rng.randn(B, 3, 3))[0].astype(np.float32)
    seg = np.array([0, 100, 100, N])
    scene = np.array([0, 2, 2, 1, 0])
    cut = tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centre), torch.from_numpy(param), kind=kind,
                        rot=None if rot is None else torch.from_numpy(rot), seg=torch.from_numpy(seg),
                        scene=torch.from_numpy(scene), closed=closed, skip_zero=skip_zero, align_origin=True)
    index, batch, rows_in_any = [], [], set()
    for b in range(B):
        for i in range(seg[scene[b]], seg[scene[b] + 1]):
            if holds_serial(pos[i], centre[b], param[b], None if rot is None else rot[b], kind, closed, skip_zero):
                index.append(i)
                batch.append(b)
                rows_in_any.add(i)
    assert cut.index.tolist() == index and cut.batch.tolist() == batch
    assert cut.start.tolist() == [batch.index(b) if b in batch else (len(batch) if all(x < b for x in batch) else
                                                                      next(k for k, x in enumerate(batch) if x > b))
                                  for b in range(B)] + [len(batch)]
    c = centre[batch].copy()
    if kind == "cylinder":
        c[:, 2] = 0
    assert np.array_equal(cut.pos.numpy(), pos[index] - c)  # an fp32 subtraction
    assert cut.status.tolist() == [len(index), 0]
    out = tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centre), torch.from_numpy(param), kind=kind,
                        rot=None if rot is None else torch.from_numpy(rot), seg=torch.from_numpy(seg),
                        scene=torch.from_numpy(scene), closed=closed, skip_zero=skip_zero, mode="outside_all")
    kept = [i for i in range(N) if i not in rows_in_any]
    assert out.index.tolist() == kept
    assert out.seg.tolist() == [sum(1 for i in kept if i < s) for s in seg]
    if len(index) > 1:
        short = tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centre), torch.from_numpy(param), kind=kind,
                              rot=None if rot is None else torch.from_numpy(rot), seg=torch.from_numpy(seg),
                              scene=torch.from_numpy(scene), closed=closed, skip_zero=skip_zero, capacity=len(index) - 1)
        assert short.status.tolist() == [len(index), 1] and short.index.tolist() == index[:-1]


def test_closed_spheres_and_cylinders_are_the_kdtree_query():
    neighbors = sklearn.neighbors
    rng = np.random.RandomState(0)
    pos = lattice(rng, 3000)
    # two rows exactly on the radii used below, around centre 0: |(39, 52, 0)| = 65 and |(3, 4, 12)| = 13, in 1 / 64
    pos = np.concatenate([pos, pos[5:6] + np.float32([[39, 52, 0]]) / 64, pos[5:6] + np.float32([[3, 4, 12]]) / 64])
    centres = pos[[5, 77, 900]]
    tree3, tree2 = neighbors.KDTree(pos, leaf_size=50), neighbors.KDTree(pos[:, :2], leaf_size=50)
    for r in (13.0 / 64.0, 65.0 / 64.0):
        s = tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centres), r, closed=True)
        c = tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centres), r, kind="cylinder", closed=True)
        for b in range(3):
            assert np.array_equal(np.sort(tree3.query_radius(centres[b:b + 1], r=r)[0]), s.index[s.start[b]:s.start[b + 1]].numpy())
            assert np.array_equal(np.sort(tree2.query_radius(centres[b:b + 1, :2], r=r)[0]),
                                  c.index[c.start[b]:c.start[b + 1]].numpy())
        assert 3000 + (r < 1) in s.index[:s.start[1]].tolist()  # the row on the radius: sklearn's ball is closed
        assert 3000 + (r < 1) not in tp.region_cut(torch.from_numpy(pos), torch.from_numpy(centres), r).index[:s.start[1]].tolist()


def test_mask_compact_is_nonzero_with_cloud_offsets():
    rng = np.random.RandomState(1)
    mask = torch.from_numpy(rng.rand(500) < 0.4)
    seg = torch.tensor([0, 0, 130, 500])
    cut = tp.mask_compact(mask, seg)
    assert torch.equal(cut.index, torch.nonzero(mask)[:, 0])
    assert cut.seg.tolist() == [0, 0, int(mask[:130].sum()), int(mask.sum())]
    assert cut.start.tolist() == [0, int(mask.sum())] and cut.batch is None
    short = tp.mask_compact(mask, seg, capacity=3)
    assert short.index.tolist() == torch.nonzero(mask)[:3, 0].tolist() and short.status.tolist() == [int(mask.sum()), 1]


# ---------------------------------------------------------------------------------------------------- elastic distortion
def scipy_elastic(coords, noise, granularity, magnitude):
    """An evaluation of the warp with scipy's own routines, written from the operator's description (not the code
    under test, and the route the reference takes: its recorded output is compared in the fixture test below):
    two rounds of a 3-tap mean along each spatial axis with zero padding (`correlate1d` on the float32 grid), then
    `interpn` over axes that run from one cell below the cloud's minimum in steps of the granularity.
    Returns (warped fp32 positions, the grid after round 1, after round 2, the three axes)."""
    third = np.float32(1) / np.float32(3)
    cells = noise.shape[:3]
    rounds = []
    for _ in range(2):
        for axis in range(3):
            noise = scipy.ndimage.correlate1d(noise, [third, third, third], axis=axis, mode="constant", cval=0.0)
        rounds.append(noise)
    lowest = coords.min(0)
    axes = []
    for d in range(3):
        first = np.float32(lowest[d]) - np.float32(granularity)            # an fp32 difference
        last = np.float64(lowest[d]) + granularity * float(cells[d] - 2)   # a float64 sum
        axes.append(np.linspace(first, last, cells[d]))
    shift = scipy.interpolate.interpn(axes, noise, coords, method="linear", bounds_error=False, fill_value=0.0)
    return (coords + shift * magnitude).astype(np.float32), rounds[0], rounds[1], axes


ELASTIC_CLOUDS = [(500, (3.0, 2.0, 1.0), 0.2, 0.4), (300, (3.0, 2.0, 0.0), 0.8, 1.6), (1, (0.0, 0.0, 0.0), 0.2, 0.4),
                  (400, (5.0, 0.1, 2.2), 0.8, 1.6), (64, (0.4, 0.4, 0.4), 0.2, 0.4)]


def elastic_cloud(k):
    n, ext, g, mag = ELASTIC_CLOUDS[k]
    rng = np.random.RandomState(k)
    pos = (rng.rand(n, 3) * np.array(ext)).astype(np.float32) + np.float32(1.5)
    grids = tp.elastic_grids(pos.min(0), pos.max(0), [0, n], g)
    d = grids.dims[0]
    return pos, grids, rng.randn(d[0], d[1], d[2], 3).astype(np.float32), g, mag


@pytest.mark.parametrize("k", range(len(ELASTIC_CLOUDS)))
def test_elastic_restatement_is_scipy_bit_for_bit(k):
    pos, grids, noise, g, mag = elastic_cloud(k)
    want, round1, round2, ax = scipy_elastic(pos, noise, g, mag)
    assert np.array_equal(tp.elastic_blur_numpy(noise, rounds=1), round1)
    assert np.array_equal(tp.elastic_blur_numpy(noise), round2)
    for d in range(3):  # the (start, step, stop) table reproduces numpy.linspace
        start, step, stop = grids.axes[0][d]
        grid = np.arange(grids.dims[0][d]) * step + start
        grid[-1] = stop
        assert np.array_equal(grid, ax[d])
    got = tp.elastic_distort(torch.from_numpy(pos), torch.tensor([0, pos.shape[0]]), g, mag, noise=[noise])
    assert np.array_equal(got.numpy(), want)


def test_elastic_batch_is_cloud_by_cloud():
    clouds = [elastic_cloud(k) for k in (0, 2, 4)]
    g, mag = 0.2, 0.4
    pos = torch.from_numpy(np.concatenate([c[0] for c in clouds]))
    seg = torch.tensor(np.concatenate([[0], np.cumsum([c[0].shape[0] for c in clouds])]))
    seg = torch.cat([seg[:2], seg[1:2], seg[2:]])  # an empty cloud in the middle
    noises = [clouds[0][2], np.zeros((3, 3, 3, 3), np.float32), clouds[1][2], clouds[2][2]]
    got, grids = tp.elastic_distort(pos, seg, g, mag, noise=noises, return_grids=True)
    assert grids.dims[1].tolist() == [3, 3, 3]
    at = 0
    for c in clouds:
        want = tp.elastic_distort(torch.from_numpy(c[0]), torch.tensor([0, c[0].shape[0]]), g, mag, noise=[c[2]])
        assert torch.equal(got[at:at + c[0].shape[0]], want)
        at += c[0].shape[0]
    drawn = tp.elastic_distort(pos, seg, g, mag, generator=torch.Generator().manual_seed(5))
    again = tp.elastic_distort(pos, seg, g, mag, generator=torch.Generator().manual_seed(5))
    assert torch.equal(drawn, again) and not torch.equal(drawn, pos)
    with pytest.raises(ValueError):
        tp.elastic_distort(pos, seg, g, mag, noise=torch.zeros(7))


# ---------------------------------------------------------------------------------------------------- the classes
def toy_batch(seed=0, sizes=(120, 1, 200)):
    rng = np.random.RandomState(seed)
    N = sum(sizes)
    return Data(pos=torch.from_numpy(lattice(rng, N, 2.0)), y=torch.from_numpy(rng.randint(0, 4, N)),
                x=torch.from_numpy(rng.randn(N, 2).astype(np.float32)), origin_id=torch.arange(N),
                norm=torch.nn.functional.normalize(torch.from_numpy(rng.randn(N, 3).astype(np.float32)), dim=1),
                batch=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)), scalar=torch.tensor([7.0]))


def cloud(data, b):
    m = data.batch == b
    return Data(**{k: (v[m] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == data.batch.shape[0] else v)
                   for k, v in vars(data).items() if k != "batch"})


def test_sphere_and_cylinder_sampling_per_cloud_and_collated():
    data = toy_batch()
    centres = torch.stack([data.pos[3], data.pos[120], data.pos[130]])
    for cls, kind in ((TR.SphereSampling, "sphere"), (TR.CylinderSampling, "cylinder")):
        out = cls(0.5, centres, align_origin=True)(data)
        at = 0
        for b in range(3):
            one = cls(0.5, centres[b], align_origin=True)(cloud(data, b))  # the reference's call: one cloud, one centre
            n = one.pos.shape[0]
            assert n > 0 and getattr(one, "batch", None) is None
            for key in ("pos", "y", "x", "origin_id", "norm"):
                assert torch.equal(getattr(out, key)[at:at + n], getattr(one, key)), (kind, b, key)
            assert (out.batch[at:at + n] == b).all()
            c = centres[b].clone()
            if kind == "cylinder":
                c[2] = 0
            assert torch.equal(one.pos, cloud(data, b).pos[one.origin_id - int((data.batch < b).sum())] - c)
            at += n
        assert at == out.pos.shape[0] and torch.equal(out.scalar, data.scalar)
    several = TR.SphereSampling(0.5, centres[1:], align_origin=False)(cloud(data, 2))  # two spheres out of one cloud
    assert several.batch.unique().tolist() == [0, 1]


def test_crops_and_dropouts_keep_the_reference_quirks():
    data = toy_batch(1)
    seg = [0, 120, 121, 321]
    # SphereCrop loses its own centre point (dist > 0) ...
    out = TR.SphereCrop(0.5).apply(data, {"centre_index": torch.tensor([3, 0, 10])})
    assert 3 not in out.origin_id.tolist() and 131 not in out.origin_id.tolist()
    assert (out.batch == 1).sum() == 0  # ... so a one-point cloud comes back empty
    d = ((data.pos.double() - data.pos[3].double()) ** 2).sum(1)
    want = [i for i in range(120) if 0 < d[i] < 0.25]
    assert out.origin_id[out.batch == 0].tolist() == want
    # FixedSphereDropout keeps a point that coincides with a centre, RandomSphereDropout does not
    fixed = TR.FixedSphereDropout(centers=[data.pos[3].tolist()], radius=0.5)(cloud(data, 0))
    assert sorted(set(range(120)) - set(fixed.origin_id.tolist())) == want
    rnd = TR.RandomSphereDropout(num_sphere=1, radius=0.5).apply(cloud(data, 0), {"centre": data.pos[3:4]})
    assert sorted(set(range(120)) - set(rnd.origin_id.tolist())) == sorted(want + [i for i in range(120) if d[i] == 0])
    # per cloud: a batch drops inside every cloud's own spheres only
    both = TR.RandomSphereDropout(num_sphere=2, radius=0.4).apply(data, TR.RandomSphereDropout(2, 0.4).draw(3, torch.Generator().manual_seed(2)))
    assert both.batch.shape[0] == both.pos.shape[0] < data.pos.shape[0]
    assert torch.equal(both.pos, data.pos[both.origin_id])
    # CubeCrop / EllipsoidCrop: the rotated predicate
    rot = TR.Random3AxisRotation(rot_x=180, rot_y=180, rot_z=180).draw(3, torch.Generator().manual_seed(4))
    cube = TR.CubeCrop(c=0.5).apply(data, dict(rot, centre=torch.stack([data.pos[5], data.pos[120], data.pos[200]])))
    ell = TR.EllipsoidCrop(a=0.5, b=0.75, c=1.0).apply(data, dict(rot, centre_index=torch.tensor([5, 0, 79])))
    for b, ci in enumerate((5, 120, 200)):
        q = (data.pos[seg[b]:seg[b + 1]].double() - data.pos[ci].double()) @ rot["matrix"][b].double().T
        assert cube.origin_id[cube.batch == b].tolist() == (torch.nonzero((q.abs() < 0.5).all(1))[:, 0] + seg[b]).tolist()
        v = (q ** 2 / torch.tensor([0.25, 0.5625, 1.0], dtype=torch.float64)).sum(1)
        assert ell.origin_id[ell.batch == b].tolist() == (torch.nonzero(v < 1)[:, 0] + seg[b]).tolist()
    assert "CubeCrop(c=0.5, rotation=Random3AxisRotation(apply_rotation=True, rot_x=180, rot_y=180, rot_z=180))" == repr(TR.CubeCrop(c=0.5))


def test_periodic_and_irregular_sampling_masks():
    data = toy_batch(2)
    p = TR.PeriodicSampling(period=0.5, prop=0.3)
    params = p.draw(3, torch.Generator().manual_seed(0))
    out = p.apply(data, params)
    kept = []
    for b in range(3):
        one = cloud(data, b)
        max_p, min_p = one.pos.max(0)[0], one.pos.min(0)[0]
        center = p.box_multiplier * params["u"][b] * (max_p - min_p) + min_p
        mask = torch.cos(p.pulse * torch.norm(one.pos - center, dim=1)) > p.thresh
        kept += one.origin_id[mask].tolist()
    assert out.origin_id.tolist() == kept and 0 < len(kept) < data.pos.shape[0]
    irr = TR.IrregularSampling(d_half=0.5, grid_size_center=0.1)
    u = torch.rand(data.pos.shape[0], generator=torch.Generator().manual_seed(1))
    centre = torch.stack([data.pos[7], data.pos[120], data.pos[150]])
    out = irr.apply(data, {"centre": centre, "point_u": u})
    d_p = ((data.pos - centre[data.batch]).abs() ** 2).sum(1)
    want = u < 0.5 ** (d_p / 0.5 ** 2)  # the keep probability halves per d_half ** p
    assert out.origin_id.tolist() == torch.nonzero(want)[:, 0].tolist()
    drawn = irr.apply(data, irr.draw(3, torch.Generator().manual_seed(3)))  # centres from the voxel representatives
    assert 0 < drawn.pos.shape[0] < data.pos.shape[0]


def test_pose_classes_are_the_reference_formulas_per_cloud():
    data = toy_batch(3)
    g = torch.Generator().manual_seed(0)
    rot = TR.Random3AxisRotation(rot_x=30, rot_y=180, rot_z=0)
    params = rot.draw(3, g)
    M = params["matrix"]
    assert torch.allclose(M @ M.transpose(1, 2), torch.eye(3).expand(3, 3, 3), atol=1e-6)
    out = rot.apply(data, params)
    scale = TR.RandomScaleAnisotropic(scales=[0.8, 1.2])
    sp = scale.draw(3, g)
    sout = scale.apply(data, sp)
    sym = TR.RandomSymmetry(axis=[True, False, True])
    fp = {"flip": torch.tensor([[True, False, True], [True, False, False], [False, False, True]])}
    yout = sym.apply(data, fp)
    tr = TR.RandomTranslation(delta_max=[1.0, 2.0, 3.0], delta_min=[-1.0, 0.0, 1.0])
    tparams = tr.draw(3, g)
    tout = tr.apply(data, tparams)
    for b in range(3):
        one, m = cloud(data, b), data.batch == b
        torch.testing.assert_close(out.pos[m], one.pos @ M[b].T, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(out.norm[m], one.norm @ M[b].T, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(sout.pos[m], one.pos * sp["scale"][b], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(sout.norm[m], torch.nn.functional.normalize(one.norm / sp["scale"][b], dim=1), rtol=1e-5, atol=1e-5)
        want = one.pos.clone()
        for i in range(3):
            if fp["flip"][b, i]:
                want[:, i] = want[:, i].max() - want[:, i]
        assert torch.equal(yout.pos[m], want)
        assert torch.equal(tout.pos[m], one.pos + tparams["trans"][b])
        assert (tparams["trans"][b] >= tr.delta_min).all() and (tparams["trans"][b] <= tr.delta_max).all()
    assert torch.equal(data.pos, toy_batch(3).pos)  # nothing is changed in place
    # the composition for one explicit order, against the textbook axis rotations
    th = torch.tensor([0.3, -1.0, 2.0])
    R = TR.rotation_from_axis_angles(th, (2, 0, 1))
    cx, sx, cy, sy, cz, sz = math.cos(0.3), math.sin(0.3), math.cos(-1.0), math.sin(-1.0), math.cos(2.0), math.sin(2.0)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    np.testing.assert_allclose(R.numpy(), Ry @ Rx @ Rz, atol=1e-6)  # z first, then x, then y
    # draws: every angle inside its limit (an axis without one stays fixed), every order of the three axes occurs
    many = TR.Random3AxisRotation(rot_x=0, rot_y=0, rot_z=30).draw(64, torch.Generator().manual_seed(1))["matrix"]
    assert torch.allclose(many[:, 2, 2], torch.ones(64)) and float(many[:, 0, 0].min()) >= math.cos(math.radians(30)) - 1e-6
    assert float(many[:, 0, 1].min()) < 0 < float(many[:, 0, 1].max())
    noise = TR.RandomNoise(sigma=0.1, clip=0.05)
    nout = noise.apply(data, {"noise": torch.ones_like(data.pos)})
    assert torch.equal(nout.pos, data.pos + 0.05)
    n1, n2 = noise.apply(data, {"seed": 5}), noise.apply(data, {"seed": 5})
    assert torch.equal(n1.pos, n2.pos) and float((n1.pos - data.pos).abs().max()) <= 0.05 + 1e-6
    assert torch.equal(TR.ScalePos(scale=2.0)(data).pos, data.pos * 2.0)


def test_sparse_coordinate_classes():
    data = toy_batch(4)
    data.coords = torch.round(data.pos / 0.05).int()
    shift = TR.ShiftVoxels()
    sp = shift.draw(3, torch.Generator().manual_seed(0))
    out = shift.apply(data, sp)
    assert sp["shift"].dtype == torch.int32 and int(sp["shift"].min()) >= 0 and int(sp["shift"].max()) < 100
    assert torch.equal(out.coords, data.coords + sp["shift"][data.batch])
    with pytest.raises(Exception):
        shift.apply(toy_batch(4), sp)
    flip = TR.RandomCoordsFlip(ignored_axis=["z"], p=0.95)
    fp = {"flip": torch.tensor([[True, False, False], [True, True, False], [False, True, False]])}
    out = flip.apply(data, fp)
    for b in range(3):
        m = data.batch == b
        want = data.coords[m].clone()
        for ax in range(3):
            if fp["flip"][b, ax]:
                want[:, ax] = want[:, ax].max() - want[:, ax]
        assert torch.equal(out.coords[m], want)
    drawn = flip.draw(200, torch.Generator().manual_seed(1))["flip"]
    assert not drawn[:, 2].any() and 0.85 < float(drawn[:, :2].float().mean()) < 1.0
    assert repr(flip) == "RandomCoordsFlip(flip_axis={0, 1}, prob=0.95, is_temporal=False)"


def test_elastic_distortion_class_applies_per_cloud():
    data = toy_batch(5)
    el = TR.ElasticDistortion(granularity=[0.2, 0.8], magnitude=[0.4, 1.6])
    out = el.apply(data, {"apply": torch.tensor([True, False, True]), "seed": 3})
    m = data.batch == 1
    assert torch.equal(out.pos[m], data.pos[m]) and not torch.equal(out.pos[~m], data.pos[~m])
    seg = torch.tensor([0, 120, 121, 321])
    gen = torch.Generator().manual_seed(3)
    pos = data.pos
    for g, mag in ((0.2, 0.4), (0.8, 1.6)):
        new = tp.elastic_distort(pos, seg, g, mag, generator=gen)
        pos = torch.where((data.batch != 1).unsqueeze(1), new, pos)
    assert torch.equal(out.pos, pos)
    assert TR.ElasticDistortion(apply_distorsion=False).apply(data, {}) is data
    assert repr(el) == "ElasticDistortion(apply_distorsion=True, granularity=[0.2, 0.8], magnitude=[0.4, 1.6])"


def test_draws_are_reproducible_for_a_seeded_generator():
    for t in (TR.RandomSphere(0.5), TR.SphereCrop(1.0), TR.CubeCrop(), TR.EllipsoidCrop(), TR.RandomSphereDropout(3, 0.5),
              TR.PeriodicSampling(), TR.IrregularSampling(), TR.Random3AxisRotation(rot_x=10, rot_z=180),
              TR.RandomScaleAnisotropic([0.9, 1.1]), TR.RandomSymmetry([True, True, False]), TR.RandomTranslation(),
              TR.RandomNoise(), TR.ShiftVoxels(), TR.RandomCoordsFlip(["z"], p=0.5),  # (at p = 0.95 two seeds can both flip all 8)
              TR.ElasticDistortion()):
        a = t.draw(4, torch.Generator().manual_seed(11))
        b = t.draw(4, torch.Generator().manual_seed(11))
        c = t.draw(4, torch.Generator().manual_seed(12))
        assert a.keys() == b.keys() and len(a) > 0
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), (t, k)
        assert any(not torch.equal(torch.as_tensor(a[k]), torch.as_tensor(c[k])) for k in a), t
    data = toy_batch(6)
    one = TR.RandomSphere(0.5)(data, torch.Generator().manual_seed(2))
    two = TR.RandomSphere(0.5)(data, torch.Generator().manual_seed(2))
    assert torch.equal(one.pos, two.pos) and torch.equal(one.batch, two.batch)


def test_grid_sphere_sampling_collates_every_region():
    data = toy_batch(7)
    grid = TR.GridSphereSampling(radius=0.75, grid_size=1.0, center=False)
    out = grid(data)
    c, cb = grid.centres(data)
    K = c.shape[0]
    assert out.center_label.shape[0] == K and out.region_cloud.tolist() == cb.tolist() and cb.tolist() == sorted(cb.tolist())
    parts = TR.GridSphereSampling.to_list(out)
    assert len(parts) == K
    seg = [0, 120, 121, 321]
    for k in range(K):
        b = int(cb[k])
        lo, hi = seg[b], seg[b + 1]
        d = ((data.pos[lo:hi].double() - c[k].double()) ** 2).sum(1)
        assert parts[k].origin_id.tolist() == (torch.nonzero(d <= 0.75 ** 2)[:, 0] + lo).tolist()
        assert int(parts[k].center_label) == int(data.y[lo + int(torch.argmin(d))])
        assert torch.equal(parts[k].pos, data.pos[parts[k].origin_id])
    # the centres are the voxel means of the 1.0 grid
    cells = torch.round(cloud(data, 0).pos / 1.0)
    assert (cb == 0).sum() == torch.unique(cells, dim=0).shape[0]
    cyl = TR.GridCylinderSampling(radius=0.75, grid_size=1.0, center=True)
    cc, ccb = cyl.centres(data)
    assert (cc[:, 2] == 0).all() and cc.shape[0] <= K
    assert repr(cyl) == "GridCylinderSampling(radius=0.75, center=True)"
    assert cyl(data).center_label.shape[0] == cc.shape[0]


def test_scene_sampler_weights_and_centre_table():
    # two toy areas: area 0 has 3 occupied 0.2-voxels (labels 0, 0, 1), area 1 has 2 (labels 1, 2)
    a0 = Data(pos=torch.tensor([[0.01, 0.0, 0.0], [0.03, 0.02, 0.0], [0.5, 0.0, 0.0], [1.0, 1.0, 0.0], [1.02, 1.0, 0.0],
                                [1.04, 1.0, 0.02]]), y=torch.tensor([0, 0, 0, 1, 1, 0]))
    a1 = Data(pos=torch.tensor([[0.0, 0.0, 1.0], [0.02, 0.0, 1.0], [3.0, 0.0, 0.0]]), y=torch.tensor([2, 1, 2]))
    s = TR.SceneSampler([a0, a1], radius=2.0, kind="sphere", sample_per_epoch=10)
    assert s.seg.tolist() == [0, 6, 9] and s.data.batch.tolist() == [0] * 6 + [1] * 3
    table = s.centres
    assert table.shape == (5, 5) and table[:, 3].tolist() == [0, 0, 0, 1, 1]
    # voxels ascend in (z, y, x); the mean of a voxel's points in fp32; the majority label, ties to the lowest
    want = torch.tensor([[0.02, 0.01, 0.0], [0.5, 0.0, 0.0], [1.02, 1.0, 0.02 / 3], [3.0, 0.0, 0.0], [0.01, 0.0, 1.0]])
    torch.testing.assert_close(table[:, :3], want, rtol=1e-6, atol=1e-7)
    assert table[:, 4].tolist() == [0, 0, 1, 2, 1]
    counts = np.array([2, 2, 1])
    w = np.sqrt(counts.mean() / counts)
    np.testing.assert_allclose(s.label_weights, w / w.sum(), rtol=1e-12)
    assert s.labels.tolist() == [0, 1, 2]
    params = s.draw(64, torch.Generator().manual_seed(0))
    again = s.draw(64, torch.Generator().manual_seed(0))
    assert torch.equal(params["row"], again["row"]) and set(params["label"].tolist()) == {0.0, 1.0, 2.0}
    assert torch.equal(table[params["row"], 4].double(), params["label"].double())
    # the reference's int(random() * (n - 1)) never picks the last centre of a label with several
    assert 1 not in params["row"][params["label"] == 0].tolist()
    batch = s.apply({"row": torch.tensor([0, 3, 2])})
    for b, row in enumerate((0, 3, 2)):
        area = int(table[row, 3])
        lo, hi = s.seg[area], s.seg[area + 1]
        d = ((s.data.pos[lo:hi].double() - table[row, :3].double()) ** 2).sum(1)
        assert batch.origin_id[batch.batch == b].tolist() == (torch.nonzero(d <= 4.0)[:, 0] + lo).tolist()
    assert torch.equal(batch.pos, s.data.pos[batch.origin_id]) and torch.equal(batch.y, s.data.y[batch.origin_id])
    test = TR.SceneSampler([a0, a1], radius=2.0, kind="cylinder", sample_per_epoch=-1)
    got = list(test.test_batches(max_clouds=2))
    assert sum(int(b.center_label.shape[0]) for b in got) == sum(int(b.centre.shape[0]) for b in got) >= 2
    assert all(int(b.batch.max()) < 2 for b in got)


# ---------------------------------------------------------------------------------------------------- the fixture
import transforms_cases as tc  # noqa: E402


@pytest.mark.parametrize("name", tc.NAMES)
def test_class_against_the_reference_fixture(name):
    """every class through `apply` with the reference's recorded draws, on single clouds and on the collated batch"""
    tc.check(name, "cpu")
