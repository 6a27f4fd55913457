"""TSDF fusion of depth frames into 3DMatch fragments (reference torch_points3d/datasets/registration/fusion.py and
utils.py: TSDFVolume, get_view_frustum, get_3D_bound, rgbd2fragment_fine, rgbd2fragment_rough, extract_pcd, rgbd2pcd).

The numpy float64 functions of this file ARE the definition: they restate the reference's CPU path (the one it runs
without pycuda) operation for operation, csrc/tsdf.hip implements the same rules on the device
(torchpoints.tsdf_integrate / tsdf_surface / depth_unproject) and must equal them bit for bit, and CPU tensors are
served by the numpy forms.

The rules ("TSDF fusion", lists how the reference's pycuda kernel deviates from them):
  voxel position  p_a = fp32(origin_a + fp32(fp32(voxel_size) * fp32(i_a))): two fp32 roundings, no fma -- what the
                  reference's vox2world evaluates under plain numpy (numba's typing would round once from double, at
                  most one ulp of the coordinate away);
  camera point    M = numpy.linalg.inv(cam_pose) in float64 on the host; c_r = ((M_r0 p_x + M_r1 p_y) + M_r2 p_z) + M_r3
                  in double; a voxel with not (c_z > 0) is skipped before any division;
  pixel           px = rint(c_x * double(fp32(fx)) / c_z + double(fp32(cx))), half to even, py likewise; the range test
                  0 <= px < W, 0 <= py < H is made in double before the cast;
  update          d = double(depth[py, px]) needs d > 0; diff = d - c_z needs diff >= -trunc; dist = min(1, diff / trunc);
                  w_new = fp32(double(w_old) + obs_weight);
                  t_new = fp32((double(fp32(w_old * t_old)) + obs_weight * dist) / double(w_new));
  surface cloud   the voxels with |t| < fp32(tsdf_thresh) and w > fp32(weight_thresh) (fp32 compares, as numpy compares
                  a float32 array with a Python number) in ascending voxel index, as index * voxel_size + double(origin);
  unprojection    Z = raw / 1000, kept for (Z < 6) & (Z > 0) in ascending pixel index; X = ((x + 0.5) - K02) * Z / K00,
                  Y likewise; world = ((X r_a0 + Y r_a1) + Z r_a2) + t_a.

Not served: the marching-cubes mesh (get_mesh), and compute_overlap_and_matches / tracked_matches of utils.py.
"""
import numpy as np
import torch

from . import torchpoints as tp

TRUNC_VOXELS = 5          # truncation margin in voxels
DEPTH_SCALE = 1000.0      # raw depth units per metre (3DMatch: millimetres)
UNPROJECT_MAX_DEPTH = 6.0  # extract_pcd keeps Z < 6
_SLAB_VOXELS = 1 << 21    # the numpy path walks the volume in x slabs of about this many voxels


class Fragment(object):
    """attribute bag (pos, optionally color), like the ones transforms.py works on"""

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def keys(self):
        return [k for k in self.__dict__ if not k.startswith("_")]

    def __repr__(self):
        return "Fragment(%s)" % ", ".join("%s=%s" % (k, tuple(getattr(self, k).shape)) for k in self.keys)


# ------------------------------------------------------------------------------------------------------------------ volume
def volume_geometry(vol_bnds, voxel_size):
    """(bounds (3, 2) float64 with the upper side moved onto the grid, dim (3,) ints, origin (3,) float32)"""
    b = np.array(vol_bnds, dtype=np.float64)
    if b.shape != (3, 2):
        raise ValueError("vol_bnds must be (3, 2)")
    vs = float(voxel_size)
    dim = np.ceil((b[:, 1] - b[:, 0]) / vs).astype(int)
    if (dim < 0).any():
        raise ValueError("vol_bnds: an upper bound lies below its lower bound")
    b[:, 1] = b[:, 0] + dim * vs
    return b, dim, b[:, 0].astype(np.float32)


def voxel_axis(origin_a, voxel_size, n, start=0):
    """(n,) float32 positions of the voxels start .. start + n - 1 of one axis: two fp32 roundings"""
    i = np.arange(start, start + n).astype(np.float32)
    return np.float32(origin_a) + np.float32(voxel_size) * i


def depth_metres_numpy(raw, depth_scale=DEPTH_SCALE, depth_thresh=None):
    """float64 metres of raw depth: double(raw) / depth_scale, zero above depth_thresh (rgbd2fragment_fine)"""
    d = np.asarray(raw).astype(np.float64) / float(depth_scale)
    if depth_thresh is not None:
        d[d > float(depth_thresh)] = 0.0
    return d


def integrate_consts(cam_intr, cam_poses, obs_weight, F):
    """(F, 17) float64 per frame: the rows 0 .. 2 of inv(cam_pose), double(fp32(fx, fy, cx, cy)), the weight"""
    K = np.asarray(cam_intr, dtype=np.float64)
    K = np.broadcast_to(K, (F, 3, 3)) if K.ndim == 2 else K
    P = np.asarray(cam_poses, dtype=np.float64).reshape(-1, 4, 4)
    w = np.broadcast_to(np.asarray(obs_weight, dtype=np.float64), (F,))
    if K.shape != (F, 3, 3) or P.shape != (F, 4, 4):
        raise ValueError("cam_intr must be (3, 3) or (F, 3, 3) and cam_poses (F, 4, 4) for %d frames" % F)
    out = np.empty((F, 17))
    for f in range(F):
        out[f, :12] = np.linalg.inv(P[f])[:3].reshape(12)
        k32 = K[f].astype(np.float32)
        out[f, 12:16] = (k32[0, 0], k32[1, 1], k32[0, 2], k32[1, 2])
        out[f, 16] = w[f]
    return out


def integrate_numpy(tsdf, weight, origin, voxel_size, depth, consts, trunc=None):
    """One frame into tsdf, weight (X, Y, Z) float32, in place.  depth (H, W) float64 metres, consts (17,) of
    integrate_consts.  Returns the number of voxels updated."""
    X, Y, Z = tsdf.shape
    H, W = depth.shape
    vs = float(voxel_size)
    trunc = TRUNC_VOXELS * vs if trunc is None else float(trunc)
    M = consts[:12].reshape(3, 4)
    fx, fy, cx, cy, obs = (float(v) for v in consts[12:17])
    py = voxel_axis(origin[1], vs, Y).astype(np.float64)[None, :, None]
    pz = voxel_axis(origin[2], vs, Z).astype(np.float64)[None, None, :]
    step = max(1, _SLAB_VOXELS // max(1, Y * Z))
    touched = 0
    with np.errstate(all="ignore"):
        for x0 in range(0, X, step):
            x1 = min(X, x0 + step)
            px = voxel_axis(origin[0], vs, x1 - x0, x0).astype(np.float64)[:, None, None]
            c = [((M[r, 0] * px + M[r, 1] * py) + M[r, 2] * pz) + M[r, 3] for r in range(3)]
            ok = c[2] > 0.0
            cz = np.where(ok, c[2], 1.0)  # skipped voxels never divide
            u = np.rint(c[0] * fx / cz + cx)
            v = np.rint(c[1] * fy / cz + cy)
            ok &= (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(H))
            ui = np.where(ok, u, 0.0).astype(np.int64)
            vi = np.where(ok, v, 0.0).astype(np.int64)
            d = np.where(ok, depth[vi, ui], 0.0)
            diff = d - c[2]
            ok &= (d > 0.0) & (diff >= -trunc)
            dist = np.minimum(1.0, diff / trunc)
            t_old, w_old = tsdf[x0:x1], weight[x0:x1]
            w_new = (w_old.astype(np.float64) + obs).astype(np.float32)
            prod = w_old * t_old  # fp32 x fp32, rounded to fp32
            t_new = ((prod.astype(np.float64) + obs * dist) / w_new.astype(np.float64)).astype(np.float32)
            tsdf[x0:x1] = np.where(ok, t_new, t_old)
            weight[x0:x1] = np.where(ok, w_new, w_old)
            touched += int(ok.sum())
    return touched


def surface_numpy(tsdf, weight, origin, voxel_size, tsdf_thresh, weight_thresh):
    """(pos (T, 3) float64, index (T,) int64 flat voxel ids), ascending"""
    X, Y, Z = tsdf.shape
    mask = (np.abs(tsdf) < np.float32(tsdf_thresh)) & (weight > np.float32(weight_thresh))
    index = np.nonzero(mask.reshape(-1))[0].astype(np.int64)
    ijk = np.stack([index // (Y * Z), (index // Z) % Y, index % Z], 1) if len(index) else np.zeros((0, 3), np.int64)
    pos = ijk.astype(np.float64) * float(voxel_size) + np.asarray(origin, dtype=np.float32).astype(np.float64)
    return pos, index


def unproject_consts(cam_intr, cam_poses, F):
    """(F, 16) float64 per frame: the rows 0 .. 2 of the pose, K00, K11, K02, K12"""
    K = np.asarray(cam_intr, dtype=np.float64)
    K = np.broadcast_to(K, (F, 3, 3)) if K.ndim == 2 else K
    P = np.broadcast_to(np.eye(4), (F, 4, 4)) if cam_poses is None else np.asarray(cam_poses, dtype=np.float64).reshape(-1, 4, 4)
    if K.shape != (F, 3, 3) or P.shape != (F, 4, 4):
        raise ValueError("cam_intr must be (3, 3) or (F, 3, 3) and cam_poses (F, 4, 4) for %d frames" % F)
    out = np.empty((F, 16))
    out[:, :12] = P[:, :3].reshape(F, 12)
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    return out


def unproject_numpy(raw, consts, depth_scale=DEPTH_SCALE, max_depth=UNPROJECT_MAX_DEPTH):
    """(start (F + 1,) int64, pos (T, 3) float64 world rows, pixel (T,) int64 = frame * H * W + y * W + x) of the raw
    depth frames (F, H, W): extract_pcd followed by rgbd2pcd's pose, frame after frame"""
    raw = np.asarray(raw)
    F, H, W = raw.shape
    start = np.zeros(F + 1, np.int64)
    rows, pixels = [], []
    for f in range(F):
        Zall = (raw[f].astype(np.float64) / float(depth_scale)).ravel()
        keep = np.nonzero((Zall < float(max_depth)) & (Zall > 0.0))[0].astype(np.int64)
        Zk = Zall[keep]
        x, y = (keep % W).astype(np.float64), (keep // W).astype(np.float64)
        c = consts[f]
        Xw = ((x + 0.5) - c[14]) * Zk / c[12]
        Yw = ((y + 0.5) - c[15]) * Zk / c[13]
        T = c[:12].reshape(3, 4)
        rows.append(np.stack([((Xw * T[a, 0] + Yw * T[a, 1]) + Zk * T[a, 2]) + T[a, 3] for a in range(3)], 1))
        pixels.append(keep + f * H * W)
        start[f + 1] = start[f] + len(keep)
    pos = np.concatenate(rows) if F else np.zeros((0, 3))
    pixel = np.concatenate(pixels) if F else np.zeros(0, np.int64)
    return start, pos.reshape(-1, 3), pixel


# ------------------------------------------------------------------------------------------------------------------ bounds
def get_view_frustum(depth_im, cam_intr, cam_pose, max_depth=None):
    """(3, 5) float64 corners of the camera's view frustum in the world: the apex and the four image corners at the
    frame's largest depth (`max_depth`, or the maximum of depth_im)"""
    im_h, im_w = depth_im.shape[-2], depth_im.shape[-1]
    if max_depth is None:
        max_depth = float(torch.amax(depth_im)) if torch.is_tensor(depth_im) else np.max(depth_im)
    K = np.asarray(cam_intr, dtype=np.float64)
    T = np.asarray(cam_pose, dtype=np.float64)
    zs = np.array([0, max_depth, max_depth, max_depth, max_depth])
    p = np.array([(np.array([0, 0, 0, im_w, im_w]) - K[0, 2]) * zs / K[0, 0],
                  (np.array([0, 0, im_h, 0, im_h]) - K[1, 2]) * zs / K[1, 1],
                  zs])
    return np.stack([((T[r, 0] * p[0] + T[r, 1] * p[1]) + T[r, 2] * p[2]) + T[r, 3] for r in range(3)])


def _raw_stack(depths):
    """depth frames as one (F, H, W) array or tensor; (is a tensor, is raw integer depth)"""
    if isinstance(depths, (list, tuple)):
        depths = torch.stack(list(depths)) if torch.is_tensor(depths[0]) else np.stack([np.asarray(d) for d in depths])
    if not torch.is_tensor(depths):
        depths = np.asarray(depths)
    if depths.ndim == 2:
        depths = depths[None]
    if depths.ndim != 3:
        raise ValueError("depth frames must be (H, W) or (F, H, W)")
    if torch.is_tensor(depths):
        return depths, True, not depths.dtype.is_floating_point
    return depths, False, depths.dtype.kind in "iu"


def _as_int32(t):
    """integer depth tensor -> int32 values (uint16 has few operators of its own)"""
    if t.dtype == torch.uint16:
        return t.view(torch.int16).to(torch.int32) & 0xFFFF
    return t.to(torch.int32)


def true_divide(t, scale):
    """t / scale in float64 with an IEEE division: torch divides a device tensor by a Python number by multiplying with
    its reciprocal, which is one rounding more than double(raw) / depth_scale"""
    t = t.to(torch.float64)
    return t / torch.full((1,), float(scale), dtype=torch.float64, device=t.device)


def frame_max_depth(depths, depth_thresh, depth_scale=DEPTH_SCALE):
    """(F,) float64 on the host: per frame the largest raw / depth_scale that is not above depth_thresh (0 when none);
    floating frames are metres already.  Device frames are reduced by torch.amax: F numbers are read back."""
    depths, is_tensor, raw = _raw_stack(depths)
    if not is_tensor:
        d = depth_metres_numpy(depths, depth_scale if raw else 1.0, depth_thresh)
        return d.reshape(d.shape[0], -1).max(1) if d.shape[0] else np.zeros(0)
    out = []
    for f0 in range(0, depths.shape[0], 8):  # a few frames at a time: the double copy stays small
        r = depths[f0:f0 + 8]
        d = true_divide(_as_int32(r), depth_scale) if raw else r.to(torch.float64)
        d = torch.where(d > float(depth_thresh), torch.zeros_like(d), d)
        out.append(torch.amax(d.reshape(d.shape[0], -1), 1))
    return torch.cat(out).cpu().numpy() if out else np.zeros(0)


def get_3D_bound(depths, intrinsic, poses, depth_thresh, limit_size=600, voxel_size=0.01):
    """(3, 2) float64 bounds of the volume of one fragment: the 0.1 / 0.9 quantiles over the frames of the frusta's
    extents, trimmed symmetrically on every axis longer than limit_size voxels"""
    depths, _, _ = _raw_stack(depths)
    F = depths.shape[0]
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(intrinsic, dtype=np.float64)
    zmax = frame_max_depth(depths, depth_thresh)
    list_min, list_max = np.zeros((3, F)), np.zeros((3, F))
    for i in range(F):
        pts = get_view_frustum(depths[i], K if K.ndim == 2 else K[i], poses[i], max_depth=zmax[i])
        list_min[:, i] = np.amin(pts, axis=1)
        list_max[:, i] = np.amax(pts, axis=1)
    vol_bnds = np.zeros((3, 2))
    vol_bnds[:, 0] = np.quantile(list_min, 0.1, axis=1)
    vol_bnds[:, 1] = np.quantile(list_max, 0.9, axis=1)
    vol_dim = (vol_bnds[:, 1] - vol_bnds[:, 0]) / voxel_size
    for i in range(3):
        if vol_dim[i] > limit_size:
            delta = voxel_size * (vol_dim[i] - limit_size) * 0.5
            vol_bnds[i][0] += delta
            vol_bnds[i][1] -= delta
    return vol_bnds


# --------------------------------------------------------------------------------------------------------------- the class
class TSDFVolume(object):
    """The reference's TSDFVolume with its method names.  device=None keeps the volume in numpy on the host (the
    definition); a torch device keeps tsdf and weight there and integrates with csrc/tsdf.hip."""

    def __init__(self, vol_bnds, voxel_size, device=None):
        self._vol_bnds, self._vol_dim, self._vol_origin = volume_geometry(vol_bnds, voxel_size)
        self._voxel_size = float(voxel_size)
        self._trunc_margin = TRUNC_VOXELS * self._voxel_size
        self.device = torch.device("cpu") if device is None else torch.device(device)
        shape = tuple(int(d) for d in self._vol_dim)
        self._tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self._weight = torch.zeros(shape, dtype=torch.float32, device=self.device)

    def integrate(self, depth_im, cam_intr, cam_pose, obs_weight=1., depth_scale=DEPTH_SCALE, depth_thresh=None):
        """one frame (H, W): raw integer depth (divided by depth_scale, zeroed above depth_thresh) or floating metres"""
        d = depth_im[None] if torch.is_tensor(depth_im) else np.asarray(depth_im)[None]
        return self.integrate_frames(d, cam_intr, np.asarray(cam_pose, dtype=np.float64)[None], obs_weight, depth_scale,
                                     depth_thresh)

    def integrate_frames(self, depths, cam_intr, cam_poses, obs_weight=1., depth_scale=DEPTH_SCALE, depth_thresh=None):
        """frames (F, H, W) in order; cam_intr (3, 3) or (F, 3, 3), cam_poses (F, 4, 4), obs_weight a number or (F,).
        On the device every voxel is read and written once per tp.tsdf_max_frames() frames."""
        depths, is_tensor, _ = _raw_stack(depths)
        if not is_tensor:
            if depths.dtype == np.uint16 and self.device.type == "cuda":
                depths = torch.from_numpy(np.ascontiguousarray(depths).view(np.int16).copy()).view(torch.uint16)
            else:
                depths = torch.from_numpy(np.ascontiguousarray(depths if depths.dtype != np.uint16 else depths.astype(np.int32)))
        tp.tsdf_integrate(self._tsdf, self._weight, self._vol_origin, self._voxel_size, depths.to(self.device), cam_intr,
                          cam_poses, obs_weight, depth_scale=depth_scale, depth_thresh=depth_thresh, trunc=self._trunc_margin)

    def get_volume(self):
        """(tsdf, weight): numpy arrays of a host volume, device tensors of a device volume (no copy either way)"""
        if self.device.type == "cuda":
            return self._tsdf, self._weight
        return self._tsdf.numpy(), self._weight.numpy()

    def get_point_cloud(self, tsdf_thresh, weight_thresh, capacity=None, return_index=False):
        """(T, 3) float64 surface points in ascending voxel index (numpy for a host volume, a device tensor otherwise)"""
        res = tp.tsdf_surface(self._tsdf, self._weight, self._vol_origin, self._voxel_size, tsdf_thresh, weight_thresh,
                              capacity=capacity)
        if self.device.type != "cuda":
            return (res.pos.numpy(), res.index.numpy()) if return_index else res.pos.numpy()
        return (res.pos, res.index) if return_index else res.pos

    def get_mesh(self):
        raise NotImplementedError("get_mesh needs marching cubes (skimage.measure.marching_cubes_lewiner in the reference),"
                                  " which this project does not provide; use get_point_cloud")


# ---------------------------------------------------------------------------------------------------------------- fragments
def fragment_windows(num_frames, num_frame_per_fragment):
    """[(begin, end)] the frame windows rgbd2fragment_fine takes its bounds from: one per num_frame_per_fragment frames,
    the last one shorter when the frames run out (the reference opens a volume for it; a fragment is written only from a
    full window)"""
    per = int(num_frame_per_fragment)
    if per < 1:
        raise ValueError("num_frame_per_fragment must be positive")
    return [(b, min(b + per, num_frames)) for b in range(0, num_frames, per)]


def rgbd2fragment_fine(depths, intrinsic, poses, num_frame_per_fragment=5, voxel_size=0.01, depth_thresh=6, limit_size=600,
                       pre_transform=None, device=None):
    """The fragments of a sequence of raw depth frames (F, H, W) with poses (F, 4, 4): every num_frame_per_fragment
    frames are fused into one TSDF volume whose surface cloud get_point_cloud(0.35, 0.0) is the fragment.  The bounds of
    a fragment come from its own frames (the reference's windows: a last window that is not longer than
    num_frame_per_fragment runs to the end of the sequence); trailing frames that do not fill a fragment give none.
    Takes arrays, not file paths.  device=None: the device of `depths` (numpy: the host)."""
    depths, is_tensor, raw = _raw_stack(depths)
    if not raw:
        raise ValueError("rgbd2fragment_fine takes raw integer depth (millimetres)")
    if device is None and is_tensor and depths.device.type == "cuda":
        device = depths.device
    n = depths.shape[0]
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(intrinsic, dtype=np.float64)
    per = int(num_frame_per_fragment)
    out = []
    for begin, end in fragment_windows(n, per):
        if end - begin < per:
            break  # the reference opens a volume for the short last window and never writes a fragment from it
        sel = slice(begin, end)
        bnds = get_3D_bound(depths[sel], K if K.ndim == 2 else K[sel], poses[sel], depth_thresh, limit_size=limit_size,
                            voxel_size=voxel_size)
        vol = TSDFVolume(bnds, voxel_size, device=device)
        vol.integrate_frames(depths[sel], K if K.ndim == 2 else K[sel], poses[sel], 1.0, depth_thresh=depth_thresh)
        pos = vol.get_point_cloud(0.35, 0.0)
        data = Fragment(pos=pos if torch.is_tensor(pos) else torch.from_numpy(pos.copy()))
        out.append(pre_transform(data) if pre_transform is not None else data)
    return out


def rgbd2fragment_rough(depths, intrinsic, poses, colors=None, num_frame_per_fragment=5, pre_transform=None):
    """The fragments as plain unions of the unprojected frames (extract_pcd + the pose), num_frame_per_fragment frames
    each, with the colour rows (F, H, W, 3) gathered alongside when given"""
    depths, is_tensor, raw = _raw_stack(depths)
    if not raw:
        raise ValueError("rgbd2fragment_rough takes raw integer depth (millimetres)")
    n, per = depths.shape[0], int(num_frame_per_fragment)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(intrinsic, dtype=np.float64)
    out = []
    for begin in range(0, n - per + 1, per):
        sel = slice(begin, begin + per)
        d = depths[sel] if is_tensor else torch.from_numpy(np.ascontiguousarray(
            depths[sel] if depths.dtype != np.uint16 else depths[sel].astype(np.int32)))
        res = tp.depth_unproject(d, K if K.ndim == 2 else K[sel], poses[sel])
        data = Fragment(pos=res.pos)
        if colors is not None:
            c = colors[sel] if torch.is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(np.asarray(colors)[sel]))
            data.color = c.reshape(-1, c.shape[-1]).to(res.pixel.device)[res.pixel]
        out.append(pre_transform(data) if pre_transform is not None else data)
    return out
