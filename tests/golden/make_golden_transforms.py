"""Generator of tests/golden/transforms.npz: the REFERENCE's sampling and augmentation transforms on the CPU (data only).

Runs the reference's own classes, unmodified, imported from the reference tree through check_dropin.install (the
stand-ins of make_golden.py / check_dropin.py: torch_geometric's Data, torch_scatter / torch_cluster bound to
oracle/voxel_ref.py, `numba.jit` a pass-through, `torch_points_kernels.points_cpu` this package's host library):
core/data_transform/transforms.py, features.py (through it), grid_transform.py and sparse_transforms.py.  sklearn's KDTree
and scipy are the installed ones.

Every class runs on two clouds, A and B, one cloud at a time as the reference does.  The random draws are recorded by
wrapping `random.random`, `torch.rand`, `torch.randint`, `torch.randn`, `np.random.randn` and `np.random.randint` around
each call (`Draws`); the rotation matrices, which also consume `random.shuffle`, are caught at
`generate_random_rotation_matrix`.  Where a recorded index points into the class's own GridSampling3D(mode="last")
result (CubeCrop, RandomSphereDropout, IrregularSampling), that sampling is rebuilt from the call's seed to turn the index
into a centre.  The archive holds inputs, draws and outputs, nothing of the reference's text.

Inputs are rounded to 10 mantissa bits before anything runs; the rounded values ARE the inputs.  Index lists are stored
ascending (the KDTree returns tree order; ascending order is this project's definition).

The generator asserts on its own inputs, and prints the smallest gaps it found:
  * no point lies within a relative 1e-5 of any region boundary used (spheres, cylinders, cubes, ellipsoids), so the
    float64 predicates of the kernels and the reference's fp32 masks differ on no row;
  * no grid centre of GridSphereSampling / GridCylinderSampling ties for its nearest point;
  * no point of PeriodicSampling / IrregularSampling lies within 1e-5 of its keep threshold (their masks are fp32 torch
    compositions, whose cos / exp may differ in the last bits between the host and the device).

    python tests/golden/make_golden_transforms.py
"""
import io
import os
import random
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import check_dropin as cd  # noqa: E402

GAPS = {}


def quantise(t):
    return (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def note_gap(name, values, bound):
    """relative distances to a boundary: all must exceed 1e-5"""
    v = float(np.min(np.abs(np.asarray(values, dtype=np.float64)))) if len(values) else float("inf")
    GAPS[name] = min(GAPS.get(name, float("inf")), v / bound if bound else v)
    assert v / (bound if bound else 1.0) > 1e-5, (name, v, bound)


def sphere_gap(name, pos, centre, r, planar=False, skip_zero=False):
    k = 2 if planar else 3
    d = pos.double().numpy()[:, :k] - np.asarray(centre, dtype=np.float64).reshape(1, -1)[:, :k]
    d2 = (d * d).sum(1)
    if skip_zero:
        d2 = d2[d2 > 0]
    note_gap(name, d2 - r * r, r * r)


def clouds():
    g = torch.Generator().manual_seed(2031)
    out = {}
    for name, n, span in (("A", 400, (2.0, 1.5, 1.0)), ("B", 250, (1.0, 2.5, 0.6))):
        pos = quantise(torch.rand(n, 3, generator=g) * torch.tensor(span) + 0.5)
        out[name] = dict(pos=pos, y=torch.randint(0, 5, (n,), generator=g), x=quantise(torch.randn(n, 2, generator=g)),
                         norm=quantise(torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)))
    return out


def fresh(c, **extra):
    n = c["pos"].shape[0]
    return cd.Data(pos=c["pos"].clone(), y=c["y"].clone(), x=c["x"].clone(), norm=c["norm"].clone(), ids=torch.arange(n), **extra)


def sorted_by_ids(d):
    order = torch.sort(d.ids)[1]
    return order, d.ids[order]


class Draws(object):
    """Records what a call draws: while the context is active `random.random`, `torch.rand`, `torch.randint`,
    `torch.randn`, `np.random.randn` and `np.random.randint` are wrapped, and every value they hand out is kept, per
    function, in call order.  The transforms reach these through the module attributes, so they draw through the wrappers."""
    WRAPPED = ((random, "random"), (torch, "rand"), (torch, "randint"), (torch, "randn"), (np.random, "randn"),
               (np.random, "randint"))

    def __enter__(self):
        self.log = {name: [] for _, name in self.WRAPPED}
        self.log["np.randn"], self.log["np.randint"] = [], []
        self._orig = []
        for module, name in self.WRAPPED:
            orig = getattr(module, name)
            key = ("np." + name) if module is np.random else name
            self._orig.append((module, name, orig))

            def wrapper(*a, _orig=orig, _key=key, **k):
                value = _orig(*a, **k)
                self.log[_key].append(value.clone() if torch.is_tensor(value) else np.copy(value))
                return value

            setattr(module, name, wrapper)
        return self

    def __exit__(self, *exc):
        for module, name, orig in self._orig:
            setattr(module, name, orig)
        return False


def drawn(transform, data):
    """(result, the recorded draws) of one call of a reference transform"""
    with Draws() as rec:
        out = transform(data)
    return out, rec.log


def main():
    from torch_points_kernels import points_cpu  # this package's host library, before any stand-in of that name exists
    import scipy.interpolate  # noqa: F401  (the reference does `import scipy` and reaches into the submodules)
    import scipy.ndimage  # noqa: F401
    T = cd.install(points_cpu, None)
    import torch_points3d.core.data_transform.grid_transform as GT
    import torch_points3d.core.data_transform.sparse_transforms as ST
    import torch_points3d.core.data_transform.features as FT

    arrays = {}
    seed = [100]

    def reseed():
        seed[0] += 1
        cd.seed_all(seed[0])
        return seed[0]

    matrices = []
    make_matrix = FT.Random3AxisRotation.generate_random_rotation_matrix

    def recording_matrix(self):
        m = make_matrix(self)
        matrices.append(m.clone())
        return m

    FT.Random3AxisRotation.generate_random_rotation_matrix = recording_matrix

    for name, c in clouds().items():
        pos, n = c["pos"], c["pos"].shape[0]
        for k, v in c.items():
            arrays["%s/%s" % (name, k)] = v
        put = lambda key, v: arrays.__setitem__("%s/%s" % (name, key), v)  # noqa: E731

        # ---- sphere / cylinder around a point of the cloud
        centre = pos[17].clone()
        for cls, key, planar in ((T.SphereSampling, "sphere", False), (T.CylinderSampling, "cylinder", True)):
            r = 0.45
            sphere_gap(key, pos, centre, r, planar=planar)
            out = cls(r, centre.numpy().copy(), align_origin=True)(fresh(c))
            order, ids = sorted_by_ids(out)
            put(key + "/centre", centre), put(key + "/ids", ids), put(key + "/pos", out.pos[order]), put(key + "/y", out.y[order])

        # ---- RandomSphere (strategy random: np.random.randint picks the centre)
        reseed()
        out, log = drawn(T.RandomSphere(0.4, strategy="random", center=True), fresh(c))
        i = int(log["np.randint"][0])
        sphere_gap("random_sphere", pos, pos[i], 0.4)
        order, ids = sorted_by_ids(out)
        put("random_sphere/centre_index", torch.tensor([i])), put("random_sphere/ids", ids), put("random_sphere/pos", out.pos[order])

        # ---- the grid classes: every region of the 0.8 grid
        for cls, key, planar in ((T.GridSphereSampling, "grid_sphere", False), (T.GridCylinderSampling, "grid_cylinder", True)):
            parts = cls(0.5, grid_size=0.8, center=True)(fresh(c))
            low = T.GridSampling3D(size=0.8)(fresh(c))
            cen = low.pos if not planar else torch.from_numpy(np.unique(low.pos[:, :-1].numpy(), axis=0))
            assert len(parts) == cen.shape[0]
            starts, ids_all, pos_all, labels = [0], [], [], []
            for k, part in enumerate(parts):
                sphere_gap(key, pos, cen[k], 0.5, planar=planar)
                d = pos.double()[:, :cen.shape[1]] - cen[k].double()
                d2 = torch.sort((d * d).sum(1))[0]
                note_gap(key + "/nearest_tie", [float(d2[1] - d2[0])], float(d2[1]))
                order, ids = sorted_by_ids(part)
                ids_all.append(ids), pos_all.append(part.pos[order]), labels.append(part.center_label.reshape(-1))
                starts.append(starts[-1] + ids.shape[0])
            put(key + "/centres", cen), put(key + "/start", torch.tensor(starts)), put(key + "/ids", torch.cat(ids_all))
            put(key + "/pos", torch.cat(pos_all)), put(key + "/center_label", torch.cat(labels))

        # ---- SphereCrop: torch.randint picks the centre row; dist > 0 loses it
        reseed()
        out, log = drawn(T.SphereCrop(radius=0.5), fresh(c))
        i = int(log["randint"][0])
        sphere_gap("sphere_crop", pos, pos[i], 0.5, skip_zero=True)
        put("sphere_crop/centre_index", torch.tensor([i])), put("sphere_crop/ids", torch.sort(out.ids)[0])

        # ---- CubeCrop: centre among the `last` representatives of the 0.05 grid, a random rotation
        s = reseed()
        del matrices[:]
        out, log = drawn(T.CubeCrop(c=0.4, rot_x=180, rot_y=180, rot_z=180, grid_size_center=0.05), fresh(c))
        # the recorded index points into the class's own `last` sampling, which is rebuilt from the same seed
        cd.seed_all(s)
        data_c = T.GridSampling3D(0.05, mode="last")(fresh(c))
        cen = data_c.pos[log["randint"][0]][0]
        M = matrices[0]
        q = (pos.double() - cen.double()) @ M.double().T
        note_gap("cube_crop", (q.abs() - 0.4).numpy().reshape(-1), 0.4)
        put("cube_crop/centre", cen), put("cube_crop/matrix", M), put("cube_crop/ids", torch.sort(out.ids)[0])

        # ---- EllipsoidCrop: a row of the cloud, a random rotation
        reseed()
        del matrices[:]
        out, log = drawn(T.EllipsoidCrop(a=0.5, b=0.7, c=0.3, rot_x=180, rot_y=180, rot_z=180), fresh(c))
        i = int(log["randint"][0])
        M = matrices[0]
        q = (pos.double() - pos[i].double()) @ M.double().T
        v = (q ** 2 / torch.tensor([0.5 ** 2, 0.7 ** 2, 0.3 ** 2], dtype=torch.float64)).sum(1)
        note_gap("ellipsoid_crop", (v - 1.0).numpy(), 1.0)
        put("ellipsoid_crop/centre_index", torch.tensor([i])), put("ellipsoid_crop/matrix", M)
        put("ellipsoid_crop/ids", torch.sort(out.ids)[0])

        # ---- RandomSphereDropout / FixedSphereDropout (open balls of the host ball_query)
        s = reseed()
        out, log = drawn(T.RandomSphereDropout(num_sphere=3, radius=0.3, grid_size_center=0.05), fresh(c))
        cd.seed_all(s)
        data_c = T.GridSampling3D(0.05, mode="last")(fresh(c))
        cen = data_c.pos[log["randint"][0]]
        for k in range(3):
            sphere_gap("random_sphere_dropout", pos, cen[k], 0.3, skip_zero=True)
        put("random_sphere_dropout/centre", cen), put("random_sphere_dropout/ids", out.ids)
        far = int(torch.nonzero(((pos - torch.tensor([1.0, 1.0, 0.8])) ** 2).sum(1) > 0.6 ** 2)[0])
        fixed = [[1.0, 1.0, 0.8], pos[far].tolist()]  # the second centre IS a point: dist > 0 keeps it
        for k in range(2):
            sphere_gap("fixed_sphere_dropout", pos, fixed[k], 0.35, skip_zero=True)
        out = T.FixedSphereDropout(centers=fixed, radius=0.35)(fresh(c))
        put("fixed_sphere_dropout/centre", torch.tensor(fixed)), put("fixed_sphere_dropout/ids", out.ids)
        assert far in out.ids.tolist() and out.ids.shape[0] < n - 2

        # ---- PeriodicSampling / IrregularSampling (torch compositions + the mask)
        reseed()
        out, log = drawn(T.PeriodicSampling(period=0.4, prop=0.3), fresh(c))
        u = log["rand"][0]
        per = T.PeriodicSampling(period=0.4, prop=0.3)
        cen = (per.box_multiplier * u * (pos.max(0)[0] - pos.min(0)[0]) + pos.min(0)[0]).double()
        note_gap("periodic", (torch.cos(per.pulse * (pos.double() - cen).norm(dim=1)) - per.thresh).numpy(), 1.0)
        put("periodic/u", u), put("periodic/ids", out.ids)
        s = reseed()
        out, log = drawn(T.IrregularSampling(d_half=0.6, p=2, grid_size_center=0.1), fresh(c))
        cd.seed_all(s)
        data_c = T.GridSampling3D(0.1, mode="last")(fresh(c))
        cen = data_c.pos[log["randint"][0]][0]
        point_u = log["rand"][0]
        d_p = ((pos.double() - cen.double()).abs() ** 2).sum(1)
        note_gap("irregular", (point_u.double() - 0.5 ** (d_p / 0.6 ** 2)).numpy(), 1.0)  # keep probability halves per d_half^p
        put("irregular/centre", cen), put("irregular/point_u", point_u), put("irregular/ids", out.ids)

        # ---- pose
        s = reseed()
        del matrices[:]
        out = T.Random3AxisRotation(rot_x=20, rot_y=180, rot_z=5)(fresh(c))
        put("rotation/matrix", matrices[0]), put("rotation/pos", out.pos), put("rotation/norm", out.norm)
        reseed()
        out, log = drawn(T.RandomScaleAnisotropic(scales=[0.8, 1.25]), fresh(c))
        put("scale/scale", 0.8 + log["rand"][0] * (1.25 - 0.8)), put("scale/pos", out.pos), put("scale/norm", out.norm)
        reseed()
        out, log = drawn(T.RandomSymmetry(axis=[True, False, True]), fresh(c))
        assert len(log["rand"]) == 2  # one uniform per active axis, in axis order
        put("symmetry/flip", torch.tensor([bool(log["rand"][0] < 0.5), False, bool(log["rand"][1] < 0.5)]))
        put("symmetry/pos", out.pos)
        reseed()
        lo, hi = torch.tensor([-0.5, 0.0, -0.2]), torch.tensor([0.5, 1.0, 0.2])
        out, log = drawn(FT.RandomTranslation(delta_max=hi.tolist(), delta_min=lo.tolist()), fresh(c))
        put("translation/trans", log["rand"][0] * (hi - lo) + lo), put("translation/pos", out.pos)
        reseed()
        out, log = drawn(T.RandomNoise(sigma=0.02, clip=0.03), fresh(c))
        put("noise/noise", log["randn"][0]), put("noise/pos", out.pos)
        coords = torch.round(pos / 0.05).int()
        reseed()
        out, log = drawn(T.ShiftVoxels(), fresh(c, coords=coords.clone()))
        put("coords", coords), put("shift/shift", (log["rand"][0] * 100).int()), put("shift/coords", out.coords)
        reseed()
        out, log = drawn(ST.RandomCoordsFlip(ignored_axis=["z"], p=0.6), fresh(c, coords=coords.clone()))
        assert len(log["random"]) == 2  # one uniform per flippable axis (x, y), in axis order
        put("coords_flip/flip", torch.tensor([bool(log["random"][0] < 0.6), bool(log["random"][1] < 0.6), False]))
        put("coords_flip/coords", out.coords)

        # ---- ElasticDistortion: the application draw and the noise grids as the class drew them
        while True:  # a seed whose application draw (< 0.95) applies the distortion
            reseed()
            out, log = drawn(GT.ElasticDistortion(granularity=[0.2, 0.8], magnitude=[0.4, 1.6]), fresh(c))
            if float(log["random"][0]) < 0.95:
                break
        assert len(log["np.randn"]) == 2
        for lvl, g in enumerate(log["np.randn"]):
            put("elastic/noise%d" % lvl, torch.from_numpy(g.astype(np.float32)))
        put("elastic/pos", out.pos)

    path = os.path.join(HERE, "transforms.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:  # np.savez_compressed with fixed time stamps: the same bytes every run
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k].numpy() if torch.is_tensor(arrays[k]) else arrays[k]),
                                      allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(arrays)))
    for k in sorted(GAPS):
        print("smallest relative gap  %-28s %.3e" % (k, GAPS[k]))


if __name__ == "__main__":
    main()
