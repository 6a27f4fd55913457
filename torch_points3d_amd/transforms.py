"""The reference's sampling and augmentation transforms on ragged batches, on the device.

Mirrors (class names, constructor arguments, `__repr__`):
  * core/data_transform/transforms.py   SphereSampling, CylinderSampling, RandomSphere, GridSphereSampling,
                                        GridCylinderSampling, SphereCrop, CubeCrop, EllipsoidCrop, RandomSphereDropout,
                                        FixedSphereDropout, PeriodicSampling, IrregularSampling, RandomSymmetry,
                                        RandomNoise, ScalePos, RandomScaleAnisotropic, ShiftVoxels
  * core/data_transform/features.py     Random3AxisRotation, RandomTranslation
  * core/data_transform/sparse_transforms.py   RandomCoordsFlip
  * core/data_transform/grid_transform.py      ElasticDistortion
  * datasets/segmentation/s3dis.py:478-620     S3DISSphere / S3DISCylinder  ->  SceneSampler

The reference transforms one cloud at a time on the host (sklearn KDTree, scipy, per-sample tensor ops) and copies the
result to the GPU.  Here a transform takes an attribute bag (what grid_sampling.py accepts) that may hold a whole ragged
batch: with a `batch` attribute it acts per cloud, without one the bag is a single cloud.  Cuts go through
`torchpoints.region_cut` / `mask_compact` (csrc/transforms.hip), the warp through `torchpoints.elastic_distort`, rotations
through `torchpoints.segment_transform`; the rest is elementwise and stays a torch composition.  Every
per-point tensor of the bag follows a cut through index_select; `batch` is rewritten, `origin_id` follows like any key.
The same classes work on CPU tensors (a DataLoader worker): the operators then take their numpy restatement.

Every random class is split: `draw(nclouds, generator)` returns a small host record of parameters, `apply(data, params)`
applies it, `__call__` is `apply(data, draw(...))`.  A test, or a user replaying an experiment, feeds recorded draws to
`apply`.  Where the reference draws per point (RandomNoise, IrregularSampling, the elastic noise) the record holds a
seed and `apply` draws on the data's device with it, or takes the values themselves from the record.

Not served: FixedPoints / RandomDropout, RandomWalkDropout, DensityFilter, the `freq_class_based` strategy, the
chromatic and feature-bookkeeping transforms, the pair and multiscale wrappers.
"""
import copy

import numpy as np
import torch

from . import torchpoints as _tp
from .grid_sampling import _items, _num_nodes

__all__ = ["SphereSampling", "CylinderSampling", "RandomSphere", "GridSphereSampling", "GridCylinderSampling", "SphereCrop",
           "CubeCrop", "EllipsoidCrop", "RandomSphereDropout", "FixedSphereDropout", "PeriodicSampling", "IrregularSampling",
           "Random3AxisRotation", "RandomScaleAnisotropic", "RandomSymmetry", "RandomTranslation", "RandomNoise", "ScalePos",
           "ShiftVoxels", "RandomCoordsFlip", "ElasticDistortion", "SceneSampler"]


# ---------------------------------------------------------------------------------------------------------------------
# the bag
# ---------------------------------------------------------------------------------------------------------------------
def _is_gpu(t):
    return t.device.type == "cuda"


def cloud_table(data):
    """(seg (B + 1,) int64 on the data's device, B): the rows of every cloud; a bag without `batch` is one cloud"""
    N = _num_nodes(data)
    batch = getattr(data, "batch", None)
    dev = data.pos.device
    if batch is None:
        return torch.tensor([0, N], dtype=torch.int64, device=dev), 1
    if _is_gpu(batch):
        return _tp._cloud_rows(batch, None, N)
    b = batch.numpy().astype(np.int64)
    if b.shape[0] > 1 and (b[1:] < b[:-1]).any():
        raise ValueError("batch must be sorted")
    counts = np.bincount(b) if b.shape[0] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)), int(counts.shape[0])


def _batch_of(data, seg, B):
    batch = getattr(data, "batch", None)
    if batch is not None:
        return batch.long()
    return torch.zeros(_num_nodes(data), dtype=torch.int64, device=data.pos.device)


def take_rows(data, index, batch=None, pos=None, skip_keys=()):
    """A shallow copy of the bag whose per-point tensors hold the rows `index` (the reference's item[ind] /
    apply_mask); `batch` and `pos` replace the gathered ones when given."""
    N = _num_nodes(data)
    out = copy.copy(data)
    for key, item in _items(data):
        if torch.is_tensor(item) and item.dim() > 0 and item.shape[0] == N and key not in skip_keys:
            setattr(out, key, item.index_select(0, index))
    if pos is not None:
        out.pos = pos
    if batch is not None:
        out.batch = batch
    if "num_nodes" in vars(out) and out.num_nodes is not None:
        out.num_nodes = int(index.shape[0])
    return out


def _rand(shape, generator):
    return torch.rand(shape, generator=generator)  # host draws: the record is small


def _seed(generator):
    return int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator))


def _device_generator(seed, dev):
    return torch.Generator(device=dev).manual_seed(int(seed))


def _pick_rows(u, seg):
    """global row seg[b] + floor(u[b] * n_b) of every cloud (u (B,) in [0, 1) on the host); -1 for an empty cloud"""
    n = (seg[1:] - seg[:-1])
    u = torch.as_tensor(u, dtype=torch.float64).to(seg.device)
    local = torch.minimum((u * n.double()).long(), (n - 1).clamp(min=0))
    return torch.where(n > 0, seg[:-1] + local, torch.full_like(n, -1))


def _cloud_max(values, seg, batch, B):
    """(B, C) per-cloud maxima of values (N, C): segment_max on the device, scatter-amax on the host"""
    if _is_gpu(values) and values.is_floating_point():
        return _tp.segment_max(values.float(), seg)
    out = torch.zeros((B,) + tuple(values.shape[1:]), dtype=values.dtype, device=values.device)
    idx = batch.reshape((-1,) + (1,) * (values.dim() - 1)).expand_as(values)
    return out.scatter_reduce_(0, idx, values, "amax", include_self=False)


def _voxel_representatives(pos, batch, seg, B, size):
    """(rows (K,), per-cloud offsets (B + 1,)) of one point per occupied voxel of edge `size`, grouped by cloud -- the
    candidate centres the reference takes from GridSampling3D(size, mode="last").  The reference shuffles first, so its
    representative is a random member of the voxel; here it is the member with the highest index (voxel_cluster)."""
    if _is_gpu(pos):
        from .grid_sampling import voxel_cluster
        _, rows, _, _, counts, _ = voxel_cluster(pos, batch if B > 1 else None, size, return_counts=True)
        counts = counts if B > 1 else torch.tensor([rows.shape[0]])
        off = torch.zeros(B + 1, dtype=torch.int64)
        off[1:1 + counts.numel()] = torch.cumsum(counts, 0)
        off[1 + counts.numel():] = off[counts.numel()]
        return rows, off.to(pos.device, non_blocking=True)  # (the counts came with voxel_cluster's own host read)
    P = pos.numpy()
    # tensor / tensor: the true fp32 division, as on the device
    cells = np.round(P / np.float32(size)).astype(np.int64)
    key = np.concatenate([batch.numpy().astype(np.int64)[:, None], cells[:, ::-1]], 1)  # (batch, z, y, x) ascending
    _, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    K = int(inverse.max()) + 1 if inverse.shape[0] else 0
    rows = np.zeros(K, dtype=np.int64)
    rows[inverse] = np.arange(P.shape[0])  # the highest index of every voxel wins
    counts = np.bincount(batch.numpy().astype(np.int64)[rows], minlength=B) if K else np.zeros(B, dtype=np.int64)
    return torch.from_numpy(rows), torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def _voxel_means_host(pos, y, size):
    """GridSampling3D(size, mode="mean") of one CPU cloud: (mean positions (K, 3), majority labels (K,), ties to the
    lowest label), voxels ascending in (z, y, x) -- what `grid_sampling.GridSampling3D` gives on the device"""
    P = pos.numpy().astype(np.float32)
    cells = np.round(P / np.float32(size)).astype(np.int64)
    _, inverse = np.unique(cells[:, ::-1], axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    K = int(inverse.max()) + 1 if inverse.shape[0] else 0
    order = np.argsort(inverse, kind="stable")
    bounds = np.searchsorted(inverse[order], np.arange(K + 1))
    means = np.zeros((K, 3), dtype=np.float32)
    labels = np.zeros(K, dtype=np.int64)
    yn = None if y is None else y.numpy().astype(np.int64)
    for k in range(K):
        members = order[bounds[k]:bounds[k + 1]]
        acc = np.zeros(3, dtype=np.float32)
        for m in members:  # ascending point order, fp32 sums, as tp3d_cluster_mean_f32
            acc = acc + P[m]
        means[k] = acc / np.float32(len(members))
        if yn is not None:
            vals, cnt = np.unique(yn[members], return_counts=True)
            labels[k] = vals[np.argmax(cnt)]
    return torch.from_numpy(means), torch.from_numpy(labels)


# ---------------------------------------------------------------------------------------------------------------------
# cuts
# ---------------------------------------------------------------------------------------------------------------------
def _number(value):
    """a radius or grid size: a number, or the arithmetic expression a YAML file may give as a string ("2 * 0.04")"""
    return float(eval(value, {"__builtins__": {}})) if isinstance(value, str) else float(value)


def _centre_rows(centre):
    """(K, d) host array of one or several centres given as a sequence, an array or a tensor"""
    c = centre.detach().cpu().numpy() if torch.is_tensor(centre) else np.array(centre)
    return c.reshape(1, -1) if c.ndim == 1 else c


class _RegionSampling(object):
    """one region per centre: per cloud when the bag has a `batch` (centre b belongs to cloud b), else every centre cuts
    the one cloud; several regions come back as one collated batch"""

    _kind = "sphere"

    def _cut(self, data, centre, radius, align):
        seg, B = cloud_table(data)
        centre = centre.to(data.pos.device)
        scene = None
        if getattr(data, "batch", None) is not None:
            if centre.shape[0] != B:
                raise ValueError("%d centres for a batch of %d clouds" % (centre.shape[0], B))
            scene = torch.arange(B, dtype=torch.int64, device=data.pos.device)
        cut = _tp.region_cut(data.pos, centre, float(radius), kind=self._kind, seg=seg if scene is not None else None,
                             scene=scene, closed=True, align_origin=align)
        collated = scene is not None or centre.shape[0] > 1
        return take_rows(data, cut.index, batch=cut.batch if collated else None, pos=cut.pos.to(data.pos.dtype)), cut


class SphereSampling(_RegionSampling):
    """Samples points within a sphere (closed ball, as KDTree.query_radius); rows come back ascending."""

    def __init__(self, radius, sphere_centre, align_origin=True):
        self._radius = radius
        self._centre = _centre_rows(sphere_centre)
        self._align_origin = align_origin

    def __call__(self, data):
        return self._cut(data, torch.as_tensor(self._centre, dtype=torch.float32), self._radius, self._align_origin)[0]

    def __repr__(self):
        return "{}(radius={}, center={}, align_origin={})".format(self.__class__.__name__, self._radius, self._centre,
                                                                  self._align_origin)


class CylinderSampling(_RegionSampling):
    """Samples points within a vertical cylinder; the centre is (x, y) or (x, y, z), z ignored."""

    _kind = "cylinder"

    def __init__(self, radius, cylinder_centre, align_origin=True):
        self._radius = radius
        self._centre = _centre_rows(cylinder_centre)[:, :2]
        self._align_origin = align_origin

    def __call__(self, data):
        return self._cut(data, torch.as_tensor(self._centre, dtype=torch.float32), self._radius, self._align_origin)[0]

    def __repr__(self):
        return "{}(radius={}, center={}, align_origin={})".format(self.__class__.__name__, self._radius, self._centre,
                                                                  self._align_origin)


class RandomSphere(object):
    """A sphere around a random point of every cloud (strategy `random`)."""

    def __init__(self, radius, strategy="random", class_weight_method="sqrt", center=True):
        if strategy.lower() != "random":
            raise NotImplementedError("RandomSphere serves the `random` strategy only")
        self._radius = _number(radius)
        self._strategy = strategy
        self._class_weight_method = class_weight_method
        self._center = center

    def draw(self, nclouds, generator=None):
        return {"u": _rand((nclouds,), generator)}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        rows = params["centre_index"].to(seg.device) + seg[:-1] if "centre_index" in params else _pick_rows(params["u"], seg)
        centre = data.pos.float().index_select(0, rows.clamp(min=0))
        return _RegionSampling()._cut(data, centre, self._radius, self._center)[0]  # the centres stay on the device

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))

    def __repr__(self):
        return "{}(radius={}, center={}, sampling_strategy={})".format(self.__class__.__name__, self._radius, self._center,
                                                                       self._strategy)


def _nearest_row(pos, batch, centres, cbatch):
    """row of pos nearest to every centre, inside the centre's cloud (the reference's tree.query(k=1))"""
    if _is_gpu(pos):
        return _tp.knn(1, pos.float().contiguous(), centres.float().contiguous(), batch, cbatch)[0][:, 0]
    P, C = pos.numpy().astype(np.float64), centres.numpy().astype(np.float64)
    b, cb = batch.numpy(), cbatch.numpy()
    out = np.zeros(C.shape[0], dtype=np.int64)
    for k in range(C.shape[0]):
        rows = np.nonzero(b == cb[k])[0]
        d = P[rows] - C[k]
        out[k] = rows[np.argmin((d * d).sum(1))]
    return torch.from_numpy(out)


class _GridRegionSampling(object):
    _kind = "sphere"

    def __init__(self, radius, grid_size=None, delattr_kd_tree=True, center=True):
        self._radius = _number(radius)
        self._grid_size = _number(grid_size) if grid_size else self._radius
        self._delattr_kd_tree = delattr_kd_tree
        self._center = center

    def centres(self, data):
        """(centres (K, 3), the cloud of every centre (K,)): the voxel means of GridSampling3D(grid_size), cloud by cloud"""
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        if _is_gpu(data.pos):
            from .grid_sampling import GridSampling3D
            from .dense import Data
            low = GridSampling3D(self._grid_size)(Data(pos=data.pos.float(), batch=batch))
            c, cb = low.pos, low.batch
        else:
            parts = [_voxel_means_host(data.pos[seg[b]:seg[b + 1]].float(), None, self._grid_size)[0] for b in range(B)]
            c = torch.cat(parts) if parts else torch.zeros((0, 3))
            cb = torch.repeat_interleave(torch.arange(B), torch.tensor([p.shape[0] for p in parts], dtype=torch.int64))
        if self._kind == "cylinder":  # np.unique(grid.pos[:, :-1], axis=0): distinct (x, y), ascending, per cloud
            key = torch.unique(torch.cat([cb.to(c.dtype).unsqueeze(1), c[:, :2]], 1), dim=0)
            cb, c = key[:, 0].long(), torch.cat([key[:, 1:], torch.zeros_like(key[:, :1])], 1)
        return c, cb

    def __call__(self, data):
        """one collated batch of every grid region: `batch` = the region of each row, `center_label` (K,) = the label of
        the point nearest to the region's centre, `region_cloud` (K,) = the input cloud the region was cut from"""
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        c, cb = self.centres(data)
        pos_q = data.pos if self._kind == "sphere" else torch.cat([data.pos[:, :2], torch.zeros_like(data.pos[:, :1])], 1)
        near = _nearest_row(pos_q, batch, c, cb)
        cut = _tp.region_cut(data.pos, c, self._radius, kind=self._kind, seg=seg, scene=cb, closed=True,
                             align_origin=self._center)
        out = take_rows(data, cut.index, batch=cut.batch, pos=cut.pos.to(data.pos.dtype))
        if getattr(data, "y", None) is not None:
            out.center_label = data.y.index_select(0, near)
        out.region_cloud = cb
        out.region_start = cut.start
        return out

    @staticmethod
    def to_list(batch_data):
        """the reference's shape: one bag per region, each with its `center_label` (reads the offsets back once)"""
        start = batch_data.region_start.cpu().tolist()
        N = _num_nodes(batch_data)
        out = []
        for k in range(len(start) - 1):
            one = copy.copy(batch_data)
            for key, item in _items(batch_data):
                if torch.is_tensor(item) and item.dim() > 0 and item.shape[0] == N and key != "batch":
                    setattr(one, key, item[start[k]:start[k + 1]])
            one.batch = None
            one.region_cloud = one.region_start = None
            if getattr(batch_data, "center_label", None) is not None:
                one.center_label = batch_data.center_label[k:k + 1]
            out.append(one)
        return out

    def __repr__(self):
        return "{}(radius={}, center={})".format(self.__class__.__name__, self._radius, self._center)


class GridSphereSampling(_GridRegionSampling):
    """Fits every cloud to a grid and cuts a sphere around each grid centre, all in one region_cut."""


class GridCylinderSampling(_GridRegionSampling):
    """Fits every cloud to a grid and cuts a cylinder around each distinct (x, y) of the grid centres."""
    _kind = "cylinder"


class _PerCloudCrop(object):
    """keep, per cloud, the rows inside one region around a drawn point of the cloud"""

    def _crop(self, data, centre, param, kind, rot=None, skip_zero=False):
        seg, B = cloud_table(data)
        scene = torch.arange(B, dtype=torch.int64, device=data.pos.device)
        cut = _tp.region_cut(data.pos, centre, param, kind=kind, rot=rot, seg=seg, scene=scene, closed=False,
                             skip_zero=skip_zero, with_pos=False)
        return take_rows(data, cut.index, batch=cut.batch if getattr(data, "batch", None) is not None else None)

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))


def _drawn_centres(data, params, seg, B, grid_size=None):
    """the centre of every cloud: given (`centre`), a row of the cloud (`centre_index`, local), or the point u picks
    among the cloud's rows (grid_size None) or among its voxel representatives"""
    if "centre" in params:
        return torch.as_tensor(params["centre"], dtype=torch.float32).reshape(B, 3).to(data.pos.device)
    if "centre_index" in params:
        rows = torch.as_tensor(params["centre_index"]).to(seg.device) + seg[:-1]
    elif grid_size is None:
        rows = _pick_rows(params["u"], seg)
    else:
        reps, off = _voxel_representatives(data.pos.float(), _batch_of(data, seg, B), seg, B, grid_size)
        rows = reps.index_select(0, _pick_rows(params["u"], off).clamp(min=0)) if reps.numel() else reps.new_zeros(B)
    return data.pos.float().index_select(0, rows.clamp(min=0))


class SphereCrop(_PerCloudCrop):
    """Crop every cloud on a ball around one of its points.  The reference filters `dist > 0`, which loses the centre
    point itself (and every duplicate of it): kept."""

    def __init__(self, radius=50):
        self.radius = radius

    def draw(self, nclouds, generator=None):
        return {"u": _rand((nclouds,), generator)}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        return self._crop(data, _drawn_centres(data, params, seg, B), float(self.radius), "sphere", skip_zero=True)

    def __repr__(self):
        return "{}(radius={})".format(self.__class__.__name__, self.radius)


class CubeCrop(_PerCloudCrop):
    """Crop every cloud on a randomly rotated cube of half size c around one of its voxel representatives."""

    def __init__(self, c=1, rot_x=180, rot_y=180, rot_z=180, grid_size_center=0.01):
        self.c = c
        self.random_rotation = Random3AxisRotation(rot_x=rot_x, rot_y=rot_y, rot_z=rot_z)
        self._grid_size_center = grid_size_center

    def draw(self, nclouds, generator=None):
        return dict(self.random_rotation.draw(nclouds, generator), u=_rand((nclouds,), generator))

    def apply(self, data, params):
        seg, B = cloud_table(data)
        centre = _drawn_centres(data, params, seg, B, self._grid_size_center)
        return self._crop(data, centre, float(self.c), "box", rot=params["matrix"])

    def __repr__(self):
        return "{}(c={}, rotation={})".format(self.__class__.__name__, self.c, self.random_rotation)


class EllipsoidCrop(_PerCloudCrop):
    """Crop every cloud on a randomly rotated ellipsoid of half axes (a, b, c) around one of its points."""

    def __init__(self, a=1, b=1, c=1, rot_x=180, rot_y=180, rot_z=180):
        self._a2, self._b2, self._c2 = a ** 2, b ** 2, c ** 2
        self._axes = (float(a), float(b), float(c))
        self.random_rotation = Random3AxisRotation(rot_x=rot_x, rot_y=rot_y, rot_z=rot_z)

    def draw(self, nclouds, generator=None):
        return dict(self.random_rotation.draw(nclouds, generator), u=_rand((nclouds,), generator))

    def apply(self, data, params):
        seg, B = cloud_table(data)
        centre = _drawn_centres(data, params, seg, B)
        return self._crop(data, centre, torch.tensor(self._axes), "ellipsoid", rot=params["matrix"])

    def __repr__(self):
        return "{}(a={}, b={}, c={}, rotation={})".format(self.__class__.__name__, np.sqrt(self._a2), np.sqrt(self._b2),
                                                         np.sqrt(self._c2), self.random_rotation)


class _Dropout(object):
    def _drop(self, data, centre, scene, radius, skip_zero):
        seg, B = cloud_table(data)
        cut = _tp.region_cut(data.pos, centre, float(radius), kind="sphere", seg=seg, scene=scene, closed=False,
                             skip_zero=skip_zero, mode="outside_all")
        return take_rows(data, cut.index)


class RandomSphereDropout(_Dropout):
    """Drop the points inside num_sphere balls around voxel representatives of every cloud (open balls, the centre
    point included, as the reference's `dist >= 0`)."""

    def __init__(self, num_sphere=10, radius=5, grid_size_center=0.01):
        self.num_sphere = num_sphere
        self.radius = radius
        self._grid_size_center = grid_size_center

    def draw(self, nclouds, generator=None):
        return {"u": _rand((nclouds, self.num_sphere), generator)}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        dev = data.pos.device
        scene = torch.arange(B, dtype=torch.int64, device=dev).repeat_interleave(self.num_sphere)
        if "centre" in params:
            centre = torch.as_tensor(params["centre"], dtype=torch.float32).reshape(-1, 3).to(dev)
        else:
            reps, off = _voxel_representatives(data.pos.float(), _batch_of(data, seg, B), seg, B, self._grid_size_center)
            n = (off[1:] - off[:-1]).repeat_interleave(self.num_sphere)
            u = torch.as_tensor(params["u"], dtype=torch.float64).reshape(-1).to(dev)
            pick = off[:-1].repeat_interleave(self.num_sphere) + torch.minimum((u * n.double()).long(), (n - 1).clamp(min=0))
            centre = data.pos.float().index_select(0, reps.index_select(0, pick.clamp(max=max(reps.numel() - 1, 0))))
        return self._drop(data, centre, scene, self.radius, skip_zero=False)

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))

    def __repr__(self):
        return "{}(num_sphere={}, radius={})".format(self.__class__.__name__, self.num_sphere, self.radius)


class FixedSphereDropout(_Dropout):
    """Drop the points inside balls of fixed centres, in every cloud (or around the rows listed in data[name_ind]).
    The reference's `dist > 0` keeps a point that coincides with a centre: kept."""

    def __init__(self, centers=[[0, 0, 0]], name_ind=None, radius=1):
        self.centers = torch.tensor(centers)
        self.radius = radius
        self.name_ind = name_ind

    def __call__(self, data):
        seg, B = cloud_table(data)
        dev = data.pos.device
        if self.name_ind is None:
            K = self.centers.shape[0]
            centre = self.centers.float().repeat(B, 1).to(dev)
            scene = torch.arange(B, dtype=torch.int64, device=dev).repeat_interleave(K)
        else:
            rows = getattr(data, self.name_ind).long().reshape(-1)
            centre = data.pos.float().index_select(0, rows)
            scene = torch.searchsorted(seg, rows, right=True) - 1
        return self._drop(data, centre, scene, self.radius, skip_zero=True)

    def __repr__(self):
        return "{}(centers={}, radius={})".format(self.__class__.__name__, self.centers, self.radius)


def _mask_rows(data, mask, seg, skip_keys):
    cut = _tp.mask_compact(mask, seg)
    return take_rows(data, cut.index, skip_keys=skip_keys)


class PeriodicSampling(object):
    """Keep the points at a periodic distance from a random centre of every cloud's bounding box.  The mask is a torch
    composition; `mask_compact` applies it."""

    def __init__(self, period=0.1, prop=0.1, box_multiplier=1, skip_keys=[]):
        # a point is kept while its distance to the centre, taken modulo `period`, lies within prop * period / 2 of a
        # multiple of the period: cos(2 pi d / period) above cos(pi prop)
        self.pulse = 2 * np.pi / period
        self.thresh = np.cos(np.pi * prop)
        self.box_multiplier = box_multiplier
        self.skip_keys = skip_keys

    def draw(self, nclouds, generator=None):
        return {"u": _rand((nclouds, 3), generator)}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        pos = data.pos.float()
        max_p = _cloud_max(pos, seg, batch, B)
        min_p = -_cloud_max(-pos, seg, batch, B)
        u = torch.as_tensor(params["u"], dtype=torch.float32).to(pos.device)
        center = self.box_multiplier * u * (max_p - min_p) + min_p
        dist = (pos - center.index_select(0, batch)).pow(2).sum(1).sqrt()
        return _mask_rows(data, torch.cos(dist * self.pulse) > self.thresh, seg, self.skip_keys)

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))

    def __repr__(self):
        return "{}(pulse={}, thresh={}, box_mullti={}, skip_keys={})".format(self.__class__.__name__, self.pulse, self.thresh,
                                                                            self.box_multiplier, self.skip_keys)


class IrregularSampling(object):
    """A soft crop: the further from a drawn centre, the less likely a point is kept."""

    def __init__(self, d_half=2.5, p=2, grid_size_center=0.1, skip_keys=[]):
        self.d_half = d_half
        self.p = p
        self.skip_keys = skip_keys
        self._grid_size_center = grid_size_center

    def draw(self, nclouds, generator=None):
        return {"u": _rand((nclouds,), generator), "seed": _seed(generator)}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        pos = data.pos.float()
        center = _drawn_centres(data, params, seg, B, self._grid_size_center)
        # the keep probability halves with every d_half ** p of the p-th power distance to the centre
        power_dist = (pos - center.index_select(0, batch)).abs().pow(self.p).sum(1)
        thresh = torch.exp2(-power_dist / float(self.d_half ** self.p))
        if "point_u" in params:
            point_u = torch.as_tensor(params["point_u"], dtype=torch.float32).to(pos.device)
        else:
            point_u = torch.rand(pos.shape[0], generator=_device_generator(params["seed"], pos.device), device=pos.device)
        return _mask_rows(data, point_u < thresh, seg, self.skip_keys)

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))

    def __repr__(self):
        return "{}(d_half={}, p={}, skip_keys={})".format(self.__class__.__name__, self.d_half, self.p, self.skip_keys)


# ---------------------------------------------------------------------------------------------------------------------
# pose (elementwise torch compositions, and segment_transform for the rotation)
# ---------------------------------------------------------------------------------------------------------------------
def axis_rotations(angles):
    """(..., 3) angles in radians about x, y, z -> (..., 3, 3, 3): for every axis a the rotation
    cos(t) I + sin(t) [e_a]x + (1 - cos(t)) e_a e_a^T (Rodrigues' form about a unit axis)"""
    angles = torch.as_tensor(angles, dtype=torch.float32)
    eye = torch.eye(3)
    cross = torch.zeros(3, 3, 3)  # cross[a] = the cross-product matrix of e_a
    for a, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
        cross[a, j, i], cross[a, i, j] = 1.0, -1.0
    outer = eye.unsqueeze(2) * eye.unsqueeze(1)  # outer[a] = e_a e_a^T
    c, s = torch.cos(angles)[..., None, None], torch.sin(angles)[..., None, None]
    return c * eye + s * cross + (1 - c) * outer


def rotation_from_axis_angles(angles, order=(0, 1, 2)):
    """the product of the three axis rotations, applied in the order given: R = A[order[2]] A[order[1]] A[order[0]]
    (the reference composes its x, y, z matrices after shuffling them; the order is an explicit argument here)"""
    A = axis_rotations(angles)
    return A[..., order[2], :, :] @ A[..., order[1], :, :] @ A[..., order[0], :, :]


def _rotate(x, M, seg, batch):
    """x[i] @ M[b(i)].T per cloud: segment_transform at k = 3 on the device, a batched product on the host"""
    x = x.float()
    Mt = M.transpose(1, 2).contiguous().to(x.device)
    if _is_gpu(x):
        return _tp.segment_transform(x.contiguous(), Mt, seg=seg)
    return torch.bmm(x.unsqueeze(1), Mt.index_select(0, batch)).squeeze(1)


class Random3AxisRotation(object):
    """Rotate every cloud by its own random Euler angles (degrees), composed in a random axis order; `norm` follows."""

    def __init__(self, apply_rotation=True, rot_x=None, rot_y=None, rot_z=None):
        self._apply_rotation = apply_rotation
        limits = (rot_x, rot_y, rot_z)
        if apply_rotation and all(v is None for v in limits):
            raise ValueError("a rotation needs a limit (degrees) for at least one of rot_x, rot_y, rot_z")
        # |limit| per axis, 0 for an axis that was not given; the three names appear in __repr__
        self._rot_x, self._rot_y, self._rot_z = (abs(v) if v else 0 for v in limits)
        self._degree_angles = [self._rot_x, self._rot_y, self._rot_z]

    def draw(self, nclouds, generator=None):
        """{"matrix": (nclouds, 3, 3)}: per cloud an angle uniform in [-limit, limit] degrees about every axis (an axis
        with limit 0 stays at angle 0) and a uniformly random order in which the three axis rotations are applied"""
        limits = torch.tensor([float(v) for v in self._degree_angles], dtype=torch.float64)
        angles = (2.0 * _rand((nclouds, 3), generator).double() - 1.0) * limits * (np.pi / 180.0)
        orders = torch.argsort(_rand((nclouds, 3), generator), dim=1)  # a random permutation per cloud
        A = axis_rotations(angles.float())
        pick = lambda k: A[torch.arange(nclouds), orders[:, k]]  # noqa: E731
        return {"matrix": pick(2) @ pick(1) @ pick(0)}

    def apply(self, data, params):
        if not self._apply_rotation:
            return data
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        M = torch.as_tensor(params["matrix"], dtype=torch.float32).reshape(B, 3, 3)
        out = copy.copy(data)
        out.pos = _rotate(data.pos, M, seg, batch)
        if getattr(data, "norm", None) is not None:
            out.norm = _rotate(data.norm, M, seg, batch)
        return out

    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator)) if self._apply_rotation else data

    def __repr__(self):
        return "{}(apply_rotation={}, rot_x={}, rot_y={}, rot_z={})".format(self.__class__.__name__, self._apply_rotation,
                                                                             self._rot_x, self._rot_y, self._rot_z)


class _Elementwise(object):
    def __call__(self, data, generator=None):
        return self.apply(data, self.draw(cloud_table(data)[1], generator))


class RandomScaleAnisotropic(_Elementwise):
    """Scale every cloud by its own (s1, s2, s3) from [scales[0], scales[1]]; `norm` is divided and renormalised."""

    def __init__(self, scales=None, anisotropic=True):
        assert len(scales) == 2 and scales[0] <= scales[1]
        self.scales = scales

    def draw(self, nclouds, generator=None):
        return {"scale": self.scales[0] + _rand((nclouds, 3), generator) * (self.scales[1] - self.scales[0])}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        scale = torch.as_tensor(params["scale"], dtype=torch.float32).reshape(B, 3).to(data.pos.device)
        scale = scale.index_select(0, _batch_of(data, seg, B))
        out = copy.copy(data)
        out.pos = data.pos * scale
        if getattr(data, "norm", None) is not None:
            out.norm = torch.nn.functional.normalize(data.norm / scale, dim=1)
        return out

    def __repr__(self):
        return "{}({})".format(self.__class__.__name__, self.scales)


class RandomSymmetry(_Elementwise):
    """Mirror every cloud about its own maximum along the chosen axes, each with probability one half."""

    def __init__(self, axis=[False, False, False]):
        self.axis = axis

    def draw(self, nclouds, generator=None):
        u = _rand((nclouds, 3), generator)
        return {"flip": (u < 0.5) & torch.tensor([bool(a) for a in self.axis])}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        flip = torch.as_tensor(params["flip"]).reshape(B, 3).to(data.pos.device)
        c_max = _cloud_max(data.pos, seg, batch, B).to(data.pos.dtype)
        out = copy.copy(data)
        out.pos = torch.where(flip.index_select(0, batch), c_max.index_select(0, batch) - data.pos, data.pos)
        return out

    def __repr__(self):
        return "Random symmetry of axes: x={}, y={}, z={}".format(*self.axis)


class RandomTranslation(_Elementwise):
    """Translate every cloud by its own vector from [delta_min, delta_max]."""

    def __init__(self, delta_max=[1.0, 1.0, 1.0], delta_min=[-1.0, -1.0, -1.0]):
        self.delta_max = torch.tensor(delta_max)
        self.delta_min = torch.tensor(delta_min)

    def draw(self, nclouds, generator=None):
        return {"trans": _rand((nclouds, 3), generator) * (self.delta_max - self.delta_min) + self.delta_min}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        trans = torch.as_tensor(params["trans"], dtype=torch.float32).reshape(B, 3).to(data.pos.device)
        out = copy.copy(data)
        out.pos = data.pos + trans.index_select(0, _batch_of(data, seg, B))
        return out

    def __repr__(self):
        return "{}(delta_min={}, delta_max={})".format(self.__class__.__name__, self.delta_min, self.delta_max)


class RandomNoise(_Elementwise):
    """Isotropic gaussian jitter, clipped; the per-point normals are drawn on the data's device from the record's seed."""

    def __init__(self, sigma=0.01, clip=0.05):
        self.sigma = sigma
        self.clip = clip

    def draw(self, nclouds, generator=None):
        return {"seed": _seed(generator)}

    def apply(self, data, params):
        pos = data.pos
        if "noise" in params:
            normal = torch.as_tensor(params["noise"], dtype=pos.dtype).to(pos.device)
        else:
            normal = torch.randn(pos.shape, generator=_device_generator(params["seed"], pos.device), device=pos.device,
                                 dtype=pos.dtype)
        out = copy.copy(data)
        out.pos = pos + (self.sigma * normal).clamp(-self.clip, self.clip)
        return out

    def __repr__(self):
        return "{}(sigma={}, clip={})".format(self.__class__.__name__, self.sigma, self.clip)


class ScalePos(object):
    def __init__(self, scale=None):
        self.scale = scale

    def __call__(self, data):
        out = copy.copy(data)
        out.pos = data.pos * self.scale
        return out

    def __repr__(self):
        return "{}(scale={})".format(self.__class__.__name__, self.scale)


class ShiftVoxels(_Elementwise):
    """Shift the integer coordinates of every cloud by its own random offset in [0, 100)^3."""

    def __init__(self, apply_shift=True):
        self._apply_shift = apply_shift

    def draw(self, nclouds, generator=None):
        return {"shift": (_rand((nclouds, 3), generator) * 100).int()}

    def apply(self, data, params):
        if not self._apply_shift:
            return data
        if getattr(data, "coords", None) is None:
            raise ValueError("ShiftVoxels needs `coords`: run GridSampling3D(quantize_coords=True) first")
        if data.coords.dtype != torch.int32:
            raise ValueError("`coords` must be int32 voxel coordinates, got %s" % data.coords.dtype)
        seg, B = cloud_table(data)
        shift = torch.as_tensor(params["shift"], dtype=torch.int32).reshape(B, 3).to(data.coords.device)
        out = copy.copy(data)
        out.coords = data.coords.clone()
        out.coords[:, :3] += shift.index_select(0, _batch_of(data, seg, B))
        return out

    def __repr__(self):
        return "{}(apply_shift={})".format(self.__class__.__name__, self._apply_shift)


class RandomCoordsFlip(_Elementwise):
    """Flip the sparse coordinates of every cloud about its own maximum along the non-ignored axes, each with
    probability p."""

    def __init__(self, ignored_axis, is_temporal=False, p=0.95):
        if not 0 <= p <= 1:
            raise ValueError("p is a probability")
        self._is_temporal, self._p = is_temporal, p
        self._D = 3 + int(bool(is_temporal))  # a temporal cloud carries a fourth coordinate
        kept = {"xyz".index(name) for name in ignored_axis}
        self._horz_axes = {a for a in range(self._D) if a not in kept}  # the axes that may flip (named in __repr__)

    def draw(self, nclouds, generator=None):
        may_flip = torch.tensor([a in self._horz_axes for a in range(self._D)])
        return {"flip": (_rand((nclouds, self._D), generator) < self._p) & may_flip}

    def apply(self, data, params):
        seg, B = cloud_table(data)
        batch = _batch_of(data, seg, B)
        coords = data.coords
        flip = torch.as_tensor(params["flip"]).reshape(B, self._D).to(coords.device)
        c_max = _cloud_max(coords[:, :self._D], seg, batch, B)
        out = copy.copy(data)
        out.coords = coords.clone()
        out.coords[:, :self._D] = torch.where(flip.index_select(0, batch), c_max.index_select(0, batch) - coords[:, :self._D],
                                              coords[:, :self._D])
        return out

    def __repr__(self):
        return "{}(flip_axis={}, prob={}, is_temporal={})".format(self.__class__.__name__, self._horz_axes, self._p,
                                                                  self._is_temporal)


class ElasticDistortion(_Elementwise):
    """Elastic distortion of every cloud: smoothed gaussian noise on a grid of `granularity`, interpolated at the points
    and scaled by `magnitude`, one level after the other (`torchpoints.elastic_distort`).  A cloud is distorted with
    probability 0.95."""

    def __init__(self, apply_distorsion=True, granularity=[0.2, 0.8], magnitude=[0.4, 1.6]):
        assert len(magnitude) == len(granularity)
        self._apply_distorsion = apply_distorsion
        self._granularity = granularity
        self._magnitude = magnitude

    def draw(self, nclouds, generator=None):
        return {"apply": _rand((nclouds,), generator) < 0.95, "seed": _seed(generator)}

    def apply(self, data, params):
        """params: `apply` (B,) bool; `noise`: one entry per level (what elastic_distort takes), or `seed`"""
        if not self._apply_distorsion:
            return data
        seg, B = cloud_table(data)
        flag = torch.as_tensor(params["apply"]).reshape(B).to(data.pos.device).index_select(0, _batch_of(data, seg, B))
        gen = None if "noise" in params else _device_generator(params["seed"], data.pos.device)
        pos = data.pos.float()
        for i in range(len(self._granularity)):
            new = _tp.elastic_distort(pos, seg, self._granularity[i], self._magnitude[i],
                                      noise=params["noise"][i] if "noise" in params else None, generator=gen)
            pos = torch.where(flag.unsqueeze(1), new, pos)
        out = copy.copy(data)
        out.pos = pos
        return out

    def __repr__(self):
        return "{}(apply_distorsion={}, granularity={}, magnitude={})".format(self.__class__.__name__, self._apply_distorsion,
                                                                              self._granularity, self._magnitude)


# ---------------------------------------------------------------------------------------------------------------------
class SceneSampler(object):
    """S3DISSphere / S3DISCylinder with the areas resident: `datas` (the dataset's `_datas`: bags with pos and y) are
    concatenated once into one tensor per key with a scene table, and a batch of B samples is ONE region_cut.

      centres   (K, 5) = x, y, z, area, label: the voxel means and majority labels of GridSampling3D(radius / 10) per area
      labels, label_weights   the classes present and sqrt(mean count / count), normalised (the reference's
                              `_label_counts`)
      sample(B, generator)    draws B (label, centre) pairs by the reference's rule -- a label by weight, then centre
                              int(u * (n - 1)) of that label's centres -- and returns one collated batch (pos not
                              centred, as the reference's align_origin=False) with `batch`, `origin_id` (row in the
                              resident tensors) and `centre` / `centre_label` per sample
      test_batches(max_clouds)  the fixed grid of regions (GridSphereSampling(radius, radius, center=False)), at most
                              max_clouds regions per batch

    sample_per_epoch > 0 builds the centre table (as the reference does); <= 0 serves test_batches."""

    def __init__(self, datas, radius=2, kind="sphere", sample_per_epoch=100, device=None):
        if kind not in ("sphere", "cylinder"):
            raise ValueError("kind must be 'sphere' or 'cylinder'")
        datas = list(datas) if isinstance(datas, (list, tuple)) else [datas]
        self._radius, self._kind, self._sample_per_epoch = float(radius), kind, sample_per_epoch
        dev = torch.device(device) if device is not None else datas[0].pos.device
        N0 = [_num_nodes(d) for d in datas]
        self.seg = torch.tensor(np.concatenate([[0], np.cumsum(N0)]), dtype=torch.int64, device=dev)
        keys = [k for k, v in _items(datas[0]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N0[0]]
        from .dense import Data
        self.data = Data(**{k: torch.cat([getattr(d, k) for d in datas]).to(dev) for k in keys})
        self.data.batch = torch.repeat_interleave(torch.arange(len(datas)), torch.tensor(N0)).to(dev)
        self.data.origin_id = torch.arange(int(self.seg[-1]), device=dev)
        if sample_per_epoch > 0:
            self._build_centres(len(datas))

    def _build_centres(self, S):
        size = self._radius / 10.0
        data, seg = self.data, self.seg
        if _is_gpu(data.pos):
            from .dense import Data
            from .grid_sampling import GridSampling3D
            low = GridSampling3D(size)(Data(pos=data.pos.float(), y=data.y, batch=data.batch))
            centres = torch.cat([low.pos, low.batch.float().unsqueeze(1), low.y.float().unsqueeze(1)], 1)
        else:
            parts = []
            for s in range(S):
                m, l = _voxel_means_host(data.pos[seg[s]:seg[s + 1]].float(), data.y[seg[s]:seg[s + 1]], size)
                parts.append(torch.cat([m, torch.full((m.shape[0], 1), float(s)), l.float().unsqueeze(1)], 1))
            centres = torch.cat(parts)
        self.centres = centres
        host = centres[:, 4].cpu().numpy()
        uni, uni_counts = np.unique(host, return_counts=True)
        w = np.sqrt(uni_counts.mean() / uni_counts)
        self.labels, self.label_weights = uni, w / np.sum(w)
        # the centres of every label, in table order: sample() indexes them on the host
        self._by_label = {float(l): np.nonzero(host == l)[0] for l in uni}

    def __len__(self):
        return self._sample_per_epoch if self._sample_per_epoch > 0 else -1

    def draw(self, B, generator=None):
        """{"label": (B,), "row": (B,) rows of the centre table}"""
        cdf = torch.from_numpy(np.cumsum(self.label_weights))
        u = _rand((B, 2), generator).double()
        which = torch.searchsorted(cdf, u[:, 0].clamp(max=float(cdf[-1]) * (1 - 1e-12)), right=True).clamp(max=len(self.labels) - 1)
        rows = []
        for b in range(B):
            valid = self._by_label[float(self.labels[int(which[b])])]
            rows.append(int(valid[int(float(u[b, 1]) * (valid.shape[0] - 1))]))
        return {"label": torch.from_numpy(self.labels[which.numpy()]), "row": torch.tensor(rows, dtype=torch.int64)}

    def apply(self, params, capacity=None):
        rows = torch.as_tensor(params["row"]).to(self.centres.device, non_blocking=True)
        c = self.centres.index_select(0, rows)
        cut = _tp.region_cut(self.data.pos, c[:, :3].contiguous(), self._radius, kind=self._kind, seg=self.seg,
                             scene=c[:, 3].long(), closed=True, align_origin=False, capacity=capacity)
        out = take_rows(self.data, cut.index, batch=cut.batch, pos=cut.pos)
        out.centre, out.centre_label, out.cut = c[:, :3], c[:, 4].long(), cut
        return out

    def sample(self, B, generator=None, capacity=None):
        """one collated batch of B random regions.  With `capacity` the call reads nothing back: the per-point tensors
        have `capacity` rows of which the first cut.status[0] are meaningful (cut.status[1]: they did not fit)."""
        return self.apply(self.draw(B, generator), capacity=capacity)

    def test_batches(self, max_clouds=16):
        grid = (GridSphereSampling if self._kind == "sphere" else GridCylinderSampling)(self._radius, self._radius, center=False)
        c, cb = grid.centres(self.data)
        pos_q = self.data.pos if self._kind == "sphere" else torch.cat([self.data.pos[:, :2], torch.zeros_like(self.data.pos[:, :1])], 1)
        near = _nearest_row(pos_q, self.data.batch, c, cb)
        for lo in range(0, c.shape[0], max_clouds):
            cc, cs = c[lo:lo + max_clouds].contiguous(), cb[lo:lo + max_clouds].contiguous()
            cut = _tp.region_cut(self.data.pos, cc, self._radius, kind=self._kind, seg=self.seg, scene=cs, closed=True)
            out = take_rows(self.data, cut.index, batch=cut.batch, pos=cut.pos)
            out.center_label = self.data.y.index_select(0, near[lo:lo + max_clouds])
            out.centre, out.cut = cc, cut
            yield out

    def __repr__(self):
        return "{}(scenes={}, radius={}, kind={}, sample_per_epoch={})".format(
            self.__class__.__name__, self.seg.numel() - 1, self._radius, self._kind, self._sample_per_epoch)
