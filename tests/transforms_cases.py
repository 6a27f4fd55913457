"""tests/golden/transforms.npz (the reference's own transform classes, one cloud at a time; make_golden_transforms.py)
against the classes of torch_points3d_amd/transforms.py, fed the recorded draws through `apply`.  Shared by
tests/test_transforms_cpu.py (CPU tensors, the numpy restatements) and tests/test_gpu_transforms.py (device tensors, the
kernels): `check(name, device)` runs one class on cloud A alone, on cloud B alone (bags without `batch`, the
reference's case) and on the collated batch [A, B], whose clouds must come out as the two single results.

Index lists, batch vectors, labels and `center_label` are compared with torch.equal; centred positions are an fp32
subtraction and compared bit-equal; the pose classes at rtol = atol = 1e-5; the elastic warp bit-equal (the generator's
route -- scipy in float64 -- and the kernel's arithmetic are the same operations in the same order)."""
import os

import numpy as np
import torch

from torch_points3d_amd import transforms as TR
from torch_points3d_amd.dense import Data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transforms.npz")
CLOUDS = ("A", "B")
_cache = {}


def golden():
    if "z" not in _cache:
        z = np.load(GOLDEN)
        _cache["z"] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _cache["z"]


def bag(names, dev, with_coords=False):
    """the clouds `names` as one bag on `dev`; a `batch` attribute only when there are several"""
    z = golden()
    keys = ["pos", "y", "x", "norm"] + (["coords"] if with_coords else [])
    out = Data(**{k: torch.cat([z["%s/%s" % (n, k)] for n in names]).to(dev) for k in keys})
    sizes = [z[n + "/pos"].shape[0] for n in names]
    out.ids = torch.cat([torch.arange(s) for s in sizes]).to(dev)
    if len(names) > 1:
        out.batch = torch.repeat_interleave(torch.arange(len(names)), torch.tensor(sizes)).to(dev)
    return out


def per_cloud(out, names):
    """the bag `out` split into its clouds (host tensors)"""
    n = out.pos.shape[0]
    batch = getattr(out, "batch", None)
    parts = []
    for b in range(len(names)):
        m = torch.ones(n, dtype=torch.bool) if batch is None else (batch.cpu() == b)
        parts.append({k: v.cpu()[m] for k, v in vars(out).items() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == n})
    return parts


def stack(key, names, cat=False):
    z = golden()
    items = [z["%s/%s" % (n, key)] for n in names]
    return torch.cat(items) if cat else torch.stack(items)


def close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def _cut_cases(name, names, dev):
    """-> (bag after the transform, {fixture key: attribute compared with torch.equal})"""
    data = bag(names, dev)
    if name == "sphere":
        return TR.SphereSampling(0.45, stack("sphere/centre", names), align_origin=True)(data), {"ids": "ids", "pos": "pos", "y": "y"}
    if name == "cylinder":
        return TR.CylinderSampling(0.45, stack("cylinder/centre", names), align_origin=True)(data), {"ids": "ids", "pos": "pos", "y": "y"}
    if name == "random_sphere":
        p = {"centre_index": stack("random_sphere/centre_index", names).reshape(-1)}
        return TR.RandomSphere(0.4, strategy="random", center=True).apply(data, p), {"ids": "ids", "pos": "pos"}
    if name == "sphere_crop":
        p = {"centre_index": stack("sphere_crop/centre_index", names).reshape(-1)}
        return TR.SphereCrop(radius=0.5).apply(data, p), {"ids": "ids"}
    if name == "cube_crop":
        p = {"matrix": stack("cube_crop/matrix", names), "centre": stack("cube_crop/centre", names)}
        return TR.CubeCrop(c=0.4, grid_size_center=0.05).apply(data, p), {"ids": "ids"}
    if name == "ellipsoid_crop":
        p = {"matrix": stack("ellipsoid_crop/matrix", names), "centre_index": stack("ellipsoid_crop/centre_index", names).reshape(-1)}
        return TR.EllipsoidCrop(a=0.5, b=0.7, c=0.3).apply(data, p), {"ids": "ids"}
    if name == "random_sphere_dropout":
        p = {"centre": stack("random_sphere_dropout/centre", names, cat=True)}
        return TR.RandomSphereDropout(num_sphere=3, radius=0.3, grid_size_center=0.05).apply(data, p), {"ids": "ids"}
    if name == "periodic":
        return TR.PeriodicSampling(period=0.4, prop=0.3).apply(data, {"u": stack("periodic/u", names)}), {"ids": "ids"}
    if name == "irregular":
        p = {"centre": stack("irregular/centre", names), "point_u": stack("irregular/point_u", names, cat=True)}
        return TR.IrregularSampling(d_half=0.6, p=2, grid_size_center=0.1).apply(data, p), {"ids": "ids"}
    raise KeyError(name)


CUTS = ["sphere", "cylinder", "random_sphere", "sphere_crop", "cube_crop", "ellipsoid_crop", "random_sphere_dropout",
        "periodic", "irregular"]
OTHERS = ["fixed_sphere_dropout", "grid_sphere", "grid_cylinder", "rotation", "scale", "symmetry", "translation", "noise",
          "shift", "coords_flip", "elastic"]
NAMES = CUTS + OTHERS


def check(name, dev):
    z = golden()
    if name in CUTS:
        for names in (("A",), ("B",), CLOUDS):
            out, keys = _cut_cases(name, names, dev)
            assert (getattr(out, "batch", None) is not None) == (len(names) > 1)
            for part, n in zip(per_cloud(out, names), names):
                for fkey, attr in keys.items():
                    assert torch.equal(part[attr], z["%s/%s/%s" % (n, name, fkey)]), (name, names, n, fkey)
                assert torch.equal(part["x"], z[n + "/x"][part["ids"]])  # every per-point key follows the cut
        return
    if name == "fixed_sphere_dropout":  # the centres differ per cloud (one is a point of the cloud): single clouds only
        for n in CLOUDS:
            out = TR.FixedSphereDropout(centers=z[n + "/fixed_sphere_dropout/centre"].tolist(), radius=0.35)(bag((n,), dev))
            assert torch.equal(out.ids.cpu(), z[n + "/fixed_sphere_dropout/ids"])
        return
    if name in ("grid_sphere", "grid_cylinder"):
        cls = TR.GridSphereSampling if name == "grid_sphere" else TR.GridCylinderSampling
        for names in (("A",), ("B",), CLOUDS):
            grid = cls(0.5, grid_size=0.8, center=True)
            out = grid(bag(names, dev))
            start = out.region_start.cpu()
            want_c = stack(name + "/centres", names, cat=True)
            got_c = grid.centres(bag(names, dev))[0].cpu()[:, :want_c.shape[1]]
            assert torch.equal(got_c, want_c), (name, names)
            k0 = 0
            for b, n in enumerate(names):
                ws = z["%s/%s/start" % (n, name)]
                K = ws.shape[0] - 1
                assert out.region_cloud.cpu()[k0:k0 + K].tolist() == [b] * K
                assert torch.equal(start[k0:k0 + K + 1] - start[k0], ws)
                rows = slice(int(start[k0]), int(start[k0 + K]))
                assert torch.equal(out.ids.cpu()[rows], z["%s/%s/ids" % (n, name)])
                assert torch.equal(out.pos.cpu()[rows], z["%s/%s/pos" % (n, name)])
                assert torch.equal(out.center_label.cpu()[k0:k0 + K], z["%s/%s/center_label" % (n, name)])
                assert torch.equal(out.batch.cpu()[rows], torch.repeat_interleave(torch.arange(k0, k0 + K), ws[1:] - ws[:-1]))
                k0 += K
            assert k0 == start.shape[0] - 1
            parts = cls.to_list(out)
            assert len(parts) == k0 and int(parts[-1].center_label) == int(out.center_label[-1])
        return
    for names in (("A",), ("B",), CLOUDS):
        data = bag(names, dev, with_coords=name in ("shift", "coords_flip"))
        if name == "rotation":
            out = TR.Random3AxisRotation(rot_x=20, rot_y=180, rot_z=5).apply(data, {"matrix": stack("rotation/matrix", names)})
            cmp = {"pos": "pos", "norm": "norm"}
        elif name == "scale":
            out = TR.RandomScaleAnisotropic(scales=[0.8, 1.25]).apply(data, {"scale": stack("scale/scale", names)})
            cmp = {"pos": "pos", "norm": "norm"}
        elif name == "symmetry":
            out = TR.RandomSymmetry(axis=[True, False, True]).apply(data, {"flip": stack("symmetry/flip", names)})
            cmp = {"pos": "pos"}
        elif name == "translation":
            out = TR.RandomTranslation(delta_max=[0.5, 1.0, 0.2], delta_min=[-0.5, 0.0, -0.2]).apply(
                data, {"trans": stack("translation/trans", names)})
            cmp = {"pos": "pos"}
        elif name == "noise":
            out = TR.RandomNoise(sigma=0.02, clip=0.03).apply(data, {"noise": stack("noise/noise", names, cat=True)})
            cmp = {"pos": "pos"}
        elif name == "shift":
            out = TR.ShiftVoxels().apply(data, {"shift": stack("shift/shift", names)})
            cmp = {"coords": "coords"}
        elif name == "coords_flip":
            out = TR.RandomCoordsFlip(ignored_axis=["z"], p=0.6).apply(data, {"flip": stack("coords_flip/flip", names)})
            cmp = {"coords": "coords"}
        elif name == "elastic":
            noise = [[z["%s/elastic/noise%d" % (n, lvl)] for n in names] for lvl in range(2)]
            out = TR.ElasticDistortion(granularity=[0.2, 0.8], magnitude=[0.4, 1.6]).apply(
                data, {"apply": torch.ones(len(names), dtype=torch.bool), "noise": noise})
            cmp = {"pos": "pos"}
        else:
            raise KeyError(name)
        for part, n in zip(per_cloud(out, names), names):
            for fkey, attr in cmp.items():
                want = z["%s/%s/%s" % (n, name, fkey)]
                if want.is_floating_point() and name != "elastic":
                    close(part[attr], want)
                else:
                    assert torch.equal(part[attr], want), (name, names, n, fkey)
