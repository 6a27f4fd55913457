"""The scene the PointGroup tests share, the host reference of its clusters and the reference formulas restated.

The scene lives on a lattice of step H = 1/64 with a jitter of at most H/64 per axis, radius = 1.5 H: lattice distances
H and sqrt(2) H join, sqrt(3) H does not, and every pair stays at least 2 % away from the radius, so the clusters cannot
depend on fp32 rounding or FMA contraction.  The generator asserts that margin and that no point has more than NSAMPLE
neighbours (float64, scipy's cKDTree): with both, the capped host walk and the connected components coincide.
"""
import functools

import numpy as np
import torch

H = 1.0 / 64
RADIUS = 1.5 * H
NSAMPLE = 32
MIN_CLUSTER_SIZE = 10
IGNORE = [0]
SNAKE_ROW, SNAKE_ROWS = 96, 30  # 30 rows of 96 voxels + 30 one-voxel connectors = 2910 voxels


def _box(lo, size):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], lo[a] + size[a]) for a in range(3)], indexing="ij"), -1)
    return g.reshape(-1, 3)


def _snake(origin):
    """a one-voxel-wide boustrophedon: long union-find paths across many workgroups"""
    out = []
    for r in range(SNAKE_ROWS):
        xs = np.arange(SNAKE_ROW) if r % 2 == 0 else np.arange(SNAKE_ROW)[::-1]
        for x in xs:
            out.append((x, 2 * r, 0))
        out.append((xs[-1], 2 * r + 1, 0))  # the connector to the next row
    return np.asarray(out) + np.asarray(origin)


def _specials():
    """[(voxels, label)]: the same in both clouds (same coordinates and label in two clouds must not merge)"""
    m = MIN_CLUSTER_SIZE
    return [
        (_snake((0, 0, 64)), 1),
        (_box((70, 0, 0), (3, 3, 3)), 1), (_box((73, 0, 0), (3, 3, 3)), 2),       # face contact, two labels: apart
        (_box((70, 10, 0), (2, 2, 2)), 3), (_box((72, 12, 0), (2, 2, 2)), 3),     # edge contact: one cluster of 16
        (_box((70, 20, 0), (2, 2, 3)), 3), (_box((72, 22, 3), (2, 2, 3)), 3),     # corner contact: two clusters of 12
        (_box((70, 30, 0), (m - 1, 1, 1)), 2),                                     # one point short: dropped
        (_box((70, 34, 0), (m, 1, 1)), 2),                                         # exactly min_cluster_size: kept
    ]


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    """dict(pos (N,3) f32, labels (N), batch (N) sorted): two clouds, CPU tensors"""
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(seed)
    specials = _specials()
    special_jitter = [rng.uniform(-H / 64, H / 64, size=v.shape) for v, _ in specials]
    pos, labels, batch = [], [], []
    for cloud in range(2):
        taken = {}
        chunks = []
        for _ in range(40):  # random boxes of 1..8 voxels per side, labels 0..3 (0 is ignored); a voxel holds one point
            size = rng.randint(1, 9, size=3)
            lo = np.asarray([rng.randint(0, 57 - size[a]) for a in range(3)])
            lab = int(rng.randint(0, 4))
            vox = [tuple(v) for v in _box(lo, size) if tuple(v) not in taken]
            for v in vox:
                taken[v] = lab
            if vox:
                v = np.asarray(vox)
                chunks.append((v * H + rng.uniform(-H / 64, H / 64, size=v.shape), np.full(len(v), lab)))
        for (v, lab), jit in zip(specials, special_jitter):
            chunks.append((v * H + jit, np.full(len(v), lab)))
        p = np.concatenate([c[0] for c in chunks]).astype(np.float32)
        lab = np.concatenate([c[1] for c in chunks])
        perm = rng.permutation(len(p))  # shuffled inside the cloud
        pos.append(p[perm])
        labels.append(lab[perm])
        batch.append(np.full(len(p), cloud))
        # the generator's own guarantees, in float64
        tree = cKDTree(pos[-1].astype(np.float64))
        pairs = tree.query_pairs(1.02 * RADIUS, output_type="ndarray")
        d = np.linalg.norm(pos[-1][pairs[:, 0]].astype(np.float64) - pos[-1][pairs[:, 1]].astype(np.float64), axis=1)
        assert d.max() < 0.98 * RADIUS, "a pair sits within 2 %% of the radius: %g" % (d.max() / RADIUS)
        most = max(len(r) for r in tree.query_ball_point(pos[-1].astype(np.float64), RADIUS))
        assert most <= NSAMPLE, "a point has %d neighbours" % most
    return dict(pos=torch.from_numpy(np.concatenate(pos)), labels=torch.from_numpy(np.concatenate(labels)).long(),
                batch=torch.from_numpy(np.concatenate(batch)).long())


def as_sorted_lists(clusters):
    return [sorted(c.tolist()) for c in clusters]


@functools.lru_cache(maxsize=None)
def scene_reference(seed=0):
    """torch_points_kernels.region_grow on the CPU copies of the scene, as sorted index lists in list order"""
    import torch_points_kernels as tpk
    s = scene(seed)
    return as_sorted_lists(tpk.region_grow(s["pos"], s["labels"], s["batch"], ignore_labels=IGNORE, radius=RADIUS,
                                           nsample=NSAMPLE, min_cluster_size=MIN_CLUSTER_SIZE))


def components_reference(pos, labels, batch, ignore, radius, min_cluster_size):
    """uncapped connected components in float64 (cKDTree pairs + scipy.sparse.csgraph), in the order
    (label, lowest member), members ascending"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p = pos.numpy().astype(np.float64)
    lab, bat = labels.numpy(), batch.numpy()
    pairs = cKDTree(p).query_pairs(radius, output_type="ndarray")
    ok = (lab[pairs[:, 0]] == lab[pairs[:, 1]]) & (bat[pairs[:, 0]] == bat[pairs[:, 1]])
    pairs = pairs[ok]
    n = len(p)
    _, comp = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    out = {}
    for i in range(n):
        if lab[i] not in ignore:
            out.setdefault((int(lab[i]), int(comp[i])), []).append(i)
    groups = [m for m in out.values() if len(m) >= min_cluster_size]
    return sorted(groups, key=lambda m: (int(lab[m[0]]), m[0]))


# ---- the reference formulas, restated (structures.py:6-49, panoptic_losses.py) ----------------------------------------
def reference_non_max_suppression(ious, scores, threshold):
    """written apart from the code under test: a plain double loop over a set of suppressed clusters"""
    order = sorted(range(len(scores)), key=lambda i: float(scores[i]), reverse=True)
    suppressed, pick = set(), []
    for rank, i in enumerate(order):
        if i in suppressed:
            continue
        pick.append(i)
        for j in order[rank + 1:]:
            if float(ious[i, j]) > threshold:
                suppressed.add(j)
    return pick


def reference_cross_ious(clusters, n_points):
    """the dense mask with mm"""
    masks = torch.zeros(len(clusters), n_points)
    for i, c in enumerate(clusters):
        masks[i, c.cpu()] = 1
    inter = torch.mm(masks, masks.t())
    num = masks.sum(1)
    return inter / (num.unsqueeze(-1) + num.unsqueeze(0) - inter)


def reference_get_instances(clusters, scores, n_points, nms_threshold=0.3, min_cluster_points=100, min_score=0.2):
    if not clusters:
        return []
    ious = reference_cross_ious(clusters, n_points)
    pick = reference_non_max_suppression(ious.numpy(), scores.cpu().numpy(), nms_threshold)
    return [i for i in pick if len(clusters) > min_cluster_points and scores[i] > min_score]
