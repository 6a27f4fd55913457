"""The scene the PointGroup tests share, the host reference of its clusters and the reference formulas restated.

The scene lives on a lattice of step H = 1/64 with a jitter of at most H/64 per axis, radius = 1.5 H: lattice distances
H and sqrt(2) H join, sqrt(3) H does not, and every pair stays at least 2 % away from the radius, so the clusters cannot
depend on fp32 rounding or FMA contraction.  The generator asserts that margin and that no point has more than NSAMPLE
neighbours (float64, scipy's cKDTree): with both, the capped host walk and the connected components coincide.

The edge generators at the end of the file (field limits of the sort key, cell seams, adversarial index orders) give
the same two guarantees through check_margins.
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
    return _scene(seed, (0, 0, 0), 0.02)


def _scene(seed, shift, margin):
    """the scene with its voxel coordinates moved by `shift` voxels before the jitter and the fp32 cast"""
    from scipy.spatial import cKDTree
    shift = np.asarray(shift, dtype=np.int64)
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
                chunks.append(((v + shift) * H + rng.uniform(-H / 64, H / 64, size=v.shape), np.full(len(v), lab)))
        for (v, lab), jit in zip(specials, special_jitter):
            chunks.append(((v + shift) * H + jit, np.full(len(v), lab)))
        p = np.concatenate([c[0] for c in chunks]).astype(np.float32)
        lab = np.concatenate([c[1] for c in chunks])
        perm = rng.permutation(len(p))  # shuffled inside the cloud
        pos.append(p[perm])
        labels.append(lab[perm])
        batch.append(np.full(len(p), cloud))
        # the generator's own guarantees, in float64
        tree = cKDTree(pos[-1].astype(np.float64))
        pairs = tree.query_pairs((1 + margin) * RADIUS, output_type="ndarray")
        d = np.linalg.norm(pos[-1][pairs[:, 0]].astype(np.float64) - pos[-1][pairs[:, 1]].astype(np.float64), axis=1)
        assert d.max() < (1 - margin) * RADIUS, "a pair sits within %g %% of the radius: %g" % (100 * margin, d.max() / RADIUS)
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


# ---- the edge generators (tests/test_gpu_region_grow_edges.py; held to their own guarantees in test_pointgroup_cpu.py) ----
# Every generator returns dict(pos (N,3) f32, labels (N,), batch (N,) sorted) of CPU tensors, plus what its test needs
# (`want`: the expectation its construction dictates, `radius`, `cells`), and has asserted through check_margins, in
# float64 on the fp32 positions, that no pair of a cloud lies within 2 % of the radius and that no point has more
# neighbours than the nsample its test uses.
def check_margins(pos, batch, radius, nsample, margin=0.02):
    """asserts the two guarantees; nsample=None leaves the neighbour count alone (uncapped cases)"""
    from scipy.spatial import cKDTree
    p, bat = np.asarray(pos, dtype=np.float64), np.asarray(batch)
    assert np.all(bat[1:] >= bat[:-1]), "batch is not sorted"
    for cloud in np.unique(bat):
        q = p[bat == cloud]
        tree = cKDTree(q)
        pairs = tree.query_pairs((1 + margin) * radius, output_type="ndarray")
        d = np.linalg.norm(q[pairs[:, 0]] - q[pairs[:, 1]], axis=1)
        near = d[d >= (1 - margin) * radius]
        assert len(near) == 0, "a pair sits within %g %% of the radius: %r" % (100 * margin, (near[:4] / radius).tolist())
        if nsample is not None:
            most = max(len(r) for r in tree.query_ball_point(q, radius))
            assert most <= nsample, "a point has %d neighbours" % most


def _pack(pos, labels, batch, **more):
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    out = dict(pos=torch.from_numpy(pos), labels=torch.from_numpy(np.asarray(labels, dtype=np.int64)),
               batch=torch.from_numpy(np.asarray(batch, dtype=np.int64)))
    out.update(more)
    return out


def cell_edge(radius):
    """the cell edge as csrc/region_grow.hip forms it in fp32: radius * 1.01f"""
    return np.float32(radius) * np.float32(1.01)


def cells_fp32(pos, radius):
    """the integer cell of every coordinate as the kernel forms it: floorf(p * (1.0f / (radius * 1.01f)))"""
    inv = np.float32(1.0) / cell_edge(radius)
    return np.floor(np.asarray(pos, dtype=np.float32) * inv).astype(np.int64)


SHIFTS = {"straddle": (-40, -20, -70), "far": (-(1 << 21), 1 << 20, 0)}


@functools.lru_cache(maxsize=None)
def scene_shifted(which):
    """scene() moved by SHIFTS[which] voxels (applied before the jitter and the fp32 cast): the same points under the
    same indices, so the clusters are scene_reference()'s.  "straddle" puts 0 inside the span of x and y and the whole of z
    (voxels 0..64) below 0.  "far" puts
    x near -32768 and y near +16384 (cells near -1.4e6 and +0.7e6 with the span unchanged); the fp32 step there is
    H / 8 and H / 8, the jitter of at most H / 64 rounds away and x and y are the exact lattice, while z keeps its jitter.
    The worst joined pair is then (1, 0, 1) voxels with dz = H (1 + 1/32): 0.958 radii, the worst pair apart (1, 1, 1)
    with dz = H (1 - 1/32): 1.143 radii; pairs inside a z-plane sit at 0.943 and beyond.  Asserted as a 4 % margin."""
    s = _scene(0, SHIFTS[which], 0.04 if which == "far" else 0.02)
    p = s["pos"].numpy()
    if which == "straddle":
        assert all(p[:, a].min() < 0 < p[:, a].max() for a in range(2)) and p[:, 2].max() < 0
    else:
        assert np.array_equal(p[:, :2] * 64, np.round(p[:, :2] * 64)), "x and y are not the exact lattice"
        c = cells_fp32(p, RADIUS)
        assert c[:, 0].max() < -(1 << 20) and c[:, 1].min() > (1 << 19) and (c.max(0) - c.min(0)).max() < 120
    return s


def scene_with_far_point(x):
    """scene() and one more point of label 1 at the end of cloud 1, at (x, 0, 0): 1e6 is beyond 2^24 cells"""
    s = scene()
    pos = torch.cat([s["pos"], torch.tensor([[x, 0.0, 0.0]], dtype=torch.float32)])
    return dict(pos=pos, labels=torch.cat([s["labels"], torch.tensor([1])]), batch=torch.cat([s["batch"], torch.tensor([1])]))


DIRS26 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def _corner_pairs():
    """(52, 2, 3) float64: pair i < 26 sits around a cell corner at corner -+ eps * DIRS26[i], 0.9 radii apart, pair
    26 + i the same at 1.1 radii; mid-cell on the axes where the direction is 0; pairs ten cells apart"""
    cell = float(cell_edge(RADIUS))
    out = np.empty((52, 2, 3))
    for k in range(52):
        d = np.asarray(DIRS26[k % 26], dtype=np.float64)
        eps = (0.45 if k < 26 else 0.55) * RADIUS / np.linalg.norm(d)
        corner = np.asarray([10 * (k % 26) + 5, 5 + 10 * (k // 26), 5], dtype=np.float64) * cell
        mid = np.where(d == 0, 0.5 * cell, 0.0)
        out[k, 0] = corner + mid - eps * d
        out[k, 1] = corner + mid + eps * d
    return out


@functools.lru_cache(maxsize=None)
def pairs26(swap=False):
    """Every one of the 26 neighbour cells as the only link of a pair: points 2i, 2i + 1 (i < 26) are joined across
    direction DIRS26[i], points 52 + 2i, 53 + 2i are not.  swap: the two points of every pair change places, so that
    either end is the lower index.  want = [[2i, 2i + 1]] at min_cluster_size 2.  Asserts, in fp32 as the kernel forms
    them, that the cells of every pair differ by exactly the direction (or its negative under swap)."""
    pairs = _corner_pairs()
    if swap:
        pairs = pairs[:, ::-1]
    pos = pairs.reshape(-1, 3).astype(np.float32)
    check_margins(pos, np.zeros(len(pos)), RADIUS, NSAMPLE)
    cells = cells_fp32(pos, RADIUS).reshape(52, 2, 3)
    sign = -1 if swap else 1
    assert np.array_equal(cells[:, 1] - cells[:, 0], sign * np.asarray(DIRS26 + DIRS26)), "a pair is not across its direction"
    d = np.linalg.norm(pos[1::2].astype(np.float64) - pos[0::2].astype(np.float64), axis=1) / RADIUS
    assert np.all(np.abs(d[:26] - 0.9) < 1e-3) and np.all(np.abs(d[26:] - 1.1) < 1e-3)
    n = len(pos)
    return _pack(pos, np.ones(n), np.zeros(n), want=[[2 * i, 2 * i + 1] for i in range(26)], radius=RADIUS)


FIELD_LABELS, FIELD_CLOUDS = (0, 1, 4094), (0, 7, 1023)


@functools.lru_cache(maxsize=None)
def pairs26_fields(extra=None):
    """The pairs of pairs26 spread over the labels 0, 1, 4094 (nothing ignored) and the clouds 0, 7, 1023 (sorted, with
    gaps): pair k has cloud FIELD_CLOUDS[k % 3] and label FIELD_LABELS[(k // 3) % 3], the pairs then ordered by cloud, so
    that the 26 joined pairs cover all nine (label, cloud) combinations.  extra: None, or one more point (two for
    "ignored") far from the pairs at the end of the last cloud -- "label4095", "label-1", "cloud1024" (each beyond a key
    field), "ignored" (labels -1 and 5000, to be passed as ignore_labels)."""
    pairs = _corner_pairs()
    order = sorted(range(52), key=lambda k: (k % 3, k))
    pos = pairs[order].reshape(-1, 3)
    labels = np.repeat([FIELD_LABELS[(k // 3) % 3] for k in order], 2)
    batch = np.repeat([FIELD_CLOUDS[k % 3] for k in order], 2)
    joined = [[2 * j, 2 * j + 1] for j, k in enumerate(order) if k < 26]
    assert set((int(labels[c[0]]), int(batch[c[0]])) for c in joined) == set((l, c) for l in FIELD_LABELS for c in FIELD_CLOUDS)
    far = np.asarray([[1.0, 1.0, 1.0], [1.0, 1.0, 1.5]])
    add = {None: ([], []), "label4095": ([4095], [1023]), "label-1": ([-1], [1023]), "cloud1024": ([1], [1024]),
           "ignored": ([-1, 5000], [1023, 1023])}[extra]
    pos = np.concatenate([pos, far[:len(add[0])]]).astype(np.float32)
    labels, batch = np.concatenate([labels, add[0]]), np.concatenate([batch, add[1]])
    check_margins(pos, batch, RADIUS, NSAMPLE)
    want = sorted(joined, key=lambda c: (int(labels[c[0]]), c[0]))
    return _pack(pos, labels, batch, want=want, radius=RADIUS, ignore=(-1, 5000) if extra == "ignored" else ())


CELL_MAX = (1 << 14) - 3  # RG_CELL_MAX: the largest cell coordinate relative to the box that the key holds


@functools.lru_cache(maxsize=None)
def span_limit(axis, k):
    """Two clusters `k` cells apart along `axis`.  A: three points 0.3 radii apart along the next axis, in cell 0 of
    `axis` and around the middle of cell 1 of the two other axes.  B: the same three points in cell k of `axis`, at
    (k + 0.5) cells, and around them one point in each of the eight cells at +-1 on the two other axes (cells 0 and 2),
    at most 0.9 radii from a point of B: the rows dy, dz = +-1 are in play at the top of the field.  Points 0..2 are A,
    3..13 are B.  Asserts in fp32, as the kernel forms them, that the cells are the intended ones: the box then spans
    exactly k + 1 cells along `axis` (k = CELL_MAX fits the key, CELL_MAX + 1 does not)."""
    cell = float(cell_edge(RADIUS))
    o1, o2 = (axis + 1) % 3, (axis + 2) % 3

    def three(at):
        p = np.full((3, 3), 1.5 * cell)
        p[:, axis] = at
        p[:, o1] += np.asarray([-0.3, 0.0, 0.3]) * RADIUS
        return p

    around, around_cells = [], []
    for d1 in (-1, 0, 1):
        for d2 in (-1, 0, 1):
            if (d1, d2) != (0, 0):
                p = np.empty(3)
                p[axis], p[o1], p[o2] = (k + 0.5) * cell, (1.5 + 0.6 * d1) * cell, (1.5 + 0.6 * d2) * cell
                around.append(p)
                around_cells.append((1 + d1, 1 + d2))
    pos = np.concatenate([three(0.5 * cell), three((k + 0.5) * cell), np.asarray(around)]).astype(np.float32)
    n = len(pos)
    check_margins(pos, np.zeros(n), RADIUS, NSAMPLE)
    cells = cells_fp32(pos, RADIUS)
    assert cells[:3, axis].tolist() == [0] * 3 and cells[3:, axis].tolist() == [k] * 11, "not the intended cells along the axis"
    assert np.all(cells[:6, o1] == 1) and np.all(cells[:6, o2] == 1)
    assert [tuple(c) for c in cells[6:][:, [o1, o2]].tolist()] == around_cells, "not the intended neighbour cells"
    assert cells.min(0).tolist() == [0, 0, 0] and cells[:, axis].max() == k
    return _pack(pos, np.ones(n), np.zeros(n), want=[[0, 1, 2], list(range(3, 14))], radius=RADIUS, cells=cells)


def pile3(count):
    """Three piles of `count` identical points in three x-adjacent cells of one row (cells 0, 1, 2), neighbouring piles
    0.6 radii apart -- three cells cannot be met with less than 0.505 radii between neighbours -- and the outer two 1.2
    radii apart: the three runs are consecutive in the sorted keys, a point of the middle pile scans all 3 * count slots
    and joins them.  Between two far-away singles; the piles are interleaved in index order.  want: one cluster."""
    cell = float(cell_edge(RADIUS))
    x = 1.5 * cell + 0.6 * RADIUS * (np.arange(3 * count) % 3 - 1)
    pos = np.full((3 * count + 2, 3), 0.5 * cell)
    pos[1:-1, 0] = x
    pos[0], pos[-1] = -1.0, 1.0
    pos = pos.astype(np.float32)
    n = len(pos)
    check_margins(pos, np.zeros(n), RADIUS, None)
    assert cells_fp32(pos[1:-1], RADIUS).tolist() == [[c, 0, 0] for c in (np.arange(3 * count) % 3).tolist()]
    return _pack(pos, np.ones(n), np.zeros(n), want=[list(range(1, n - 1))], radius=RADIUS)


STRICT_RADIUS = 0.25


def strict_pairs():
    """radius 0.25: points 0, 1 exactly on the radius (d2 == r2 == 0.0625 in fp32: apart), points 2, 3 one ulp inside it
    (joined).  Exact by construction, so no margin applies."""
    inside = float(np.nextafter(np.float32(0.25), np.float32(0)))
    pos = np.asarray([[0, 0, 0], [0.25, 0, 0], [0, 3, 0], [inside, 3, 0]], dtype=np.float32)
    d2 = ((pos[1::2] - pos[0::2]) ** 2).sum(1, dtype=np.float32)
    assert d2[0] == np.float32(0.25) * np.float32(0.25) and d2[1] < np.float32(0.0625) and pos[3, 0] < pos[1, 0]
    return _pack(pos, np.ones(4), np.zeros(4), want=[[0], [1], [2, 3]], radius=STRICT_RADIUS)


def line_of_singles(runs):
    """`runs` points three cells apart on a line: at min_cluster_size 1 every point is a cluster, in index order"""
    cell = float(cell_edge(RADIUS))
    pos = np.full((runs, 3), 0.5 * cell)
    pos[:, 0] = (3 * np.arange(runs) + 0.5) * cell
    check_margins(pos.astype(np.float32), np.zeros(runs), RADIUS, NSAMPLE)
    return _pack(pos, np.ones(runs), np.zeros(runs), want=[[i] for i in range(runs)], radius=RADIUS)


@functools.lru_cache(maxsize=None)
def alternating_runs(runs=2049, ignored=0):
    """`runs` groups three cells apart on a line, in index order: a pair (0.5 radii apart) at the even positions, a single
    at the odd ones.  At min_cluster_size 2 the kept runs are the even ones and the compaction crosses every chunk end
    of the run scan.  ignored: that many points of label 0 (to be ignored) interleaved in index order, on a line of
    their own five cells away: they form the trailing run of left-out points.  want: the pairs."""
    cell = float(cell_edge(RADIUS))
    every = (runs // ignored) if ignored else 0
    pos, labels, want = [], [], []
    left = ignored
    for j in range(runs):
        if left and j % every == 0:
            pos.append(((3 * j + 0.5) * cell, 5.5 * cell, 0.5 * cell))
            labels.append(0)
            left -= 1
        x = (3 * j + 0.5) * cell
        if j % 2 == 0:
            want.append([len(pos), len(pos) + 1])
            pos += [(x, 0.5 * cell, 0.5 * cell), (x + 0.5 * RADIUS, 0.5 * cell, 0.5 * cell)]
            labels += [1, 1]
        else:
            pos.append((x, 0.5 * cell, 0.5 * cell))
            labels.append(1)
    assert left == 0 and len(want) == (runs + 1) // 2
    pos = np.asarray(pos, dtype=np.float32)
    check_margins(pos, np.zeros(len(pos)), RADIUS, NSAMPLE)
    return _pack(pos, labels, np.zeros(len(pos)), want=want, radius=RADIUS)


def _bit_reverse(v, bits):
    out = np.zeros_like(v)
    for b in range(bits):
        out |= ((v >> b) & 1) << (bits - 1 - b)
    return out


@functools.lru_cache(maxsize=None)
def snake_chain(order):
    """One cloud holding the snake alone (2 910 points, one cluster), its indices numbered along the path: "ascending",
    "descending", or "bitrev" -- ranked by the reversed bits of a 12-bit counter of the position on the path, so that
    index neighbours are far apart on the path at every scale.  The longest parent walks of the union-find."""
    vox = _snake((0, 0, 0))
    n = len(vox)
    rng = np.random.RandomState(5)
    path = (vox * H + rng.uniform(-H / 64, H / 64, size=vox.shape)).astype(np.float32)
    rank = np.arange(n)
    index = {"ascending": rank, "descending": n - 1 - rank,
             "bitrev": np.argsort(np.argsort(_bit_reverse(rank, 12), kind="stable"), kind="stable")}[order]
    assert sorted(index.tolist()) == list(range(n))
    pos = np.empty_like(path)
    pos[index] = path  # the point at position k of the path gets index index[k]
    check_margins(pos, np.zeros(n), RADIUS, NSAMPLE)
    return _pack(pos, np.ones(n), np.zeros(n), want=[list(range(n))], radius=RADIUS, index=index)


@functools.lru_cache(maxsize=None)
def scene_permuted(seed):
    """scene() under another permutation inside each cloud: point i of the result is point perm[i] of scene()"""
    s = scene()
    rng = np.random.RandomState(100 + seed)
    batch = s["batch"].numpy()
    perm = np.concatenate([np.flatnonzero(batch == c)[rng.permutation(int((batch == c).sum()))] for c in np.unique(batch)])
    assert np.array_equal(batch[perm], batch)
    return dict(pos=s["pos"][perm].contiguous(), labels=s["labels"][perm].contiguous(), batch=s["batch"], perm=perm)


def map_back(clusters, s):
    """clusters of scene_permuted's indices as clusters of scene()'s, members ascending, in (label, lowest member) order"""
    labels = scene()["labels"]
    back = [sorted(s["perm"][np.asarray(c, dtype=np.int64)].tolist()) for c in clusters]
    return sorted(back, key=lambda c: (int(labels[c[0]]), c[0]))
