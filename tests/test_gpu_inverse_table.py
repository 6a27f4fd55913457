"""The inverted index tables themselves (csrc/inverse_table.hip), exactly: every other test sees them through a gradient.

`tp3d_rows_scatter_invert` writes, for every destination bin, the slots that name it in ascending slot order; the table
sits in the workspace at the offsets `tp3d_scatter_plan` reports (start, order, wsorted).  The expected table is numpy's
stable argsort and bincount per cloud; these are integers, so every comparison is exact.  Every case carries bins of 24,
25, 64, 65, 1024, 1025 and 3000 slots as far as its L allows: the seams of the one-thread insertion sort (<= 24), the
wave sorts of 64 .. 1024 slots and the rule for bins of more than 1024 slots.  Each case names the inverter it is meant
to reach and fails if the library routes it elsewhere."""
import ctypes

import numpy as np
import pytest
import torch

from torch_points3d_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEAM_BINS = (24, 25, 64, 65, 1024, 1025, 3000)

# (B, L, nbins, div, weights, out-of-range entries, route)
CASES = [
    (3, 700, 50, 1, False, False, "lds1"),      # in LDS, one workgroup per cloud
    (2, 8192, 512, 1, False, False, "lds4"),    # in LDS, four workgroups per cloud
    (2, 600, 40000, 1, False, False, "hbm"),    # per cloud, tables in HBM (do not fit LDS, L < 2 nbins)
    (1, 16384, 300, 1, False, False, "flat"),   # flat, B == 1
    (2, 76800, 300, 1, False, False, "flat"),   # flat, tables do not fit LDS; the 3000-slot bin goes through merge_tmp
    (2, 2100, 128, 3, True, False, "lds1"),     # div = 3 with weights: the three_interpolate shape
    (3, 700, 50, 1, False, True, "lds1"),       # entries -1 and nbins: clamped to [0, nbins - 1]
]


def planned_sizes(L):
    """The seam sizes a cloud of L slots has room for (taken in order while they fit)."""
    sizes, used = [], 0
    for s in SEAM_BINS:
        if used + s <= L:
            sizes.append(s)
            used += s
    return sizes


def make_idx(B, L, nbins, out_of_range, seed):
    """idx (B, L) int64 and, per cloud, {bin: planned size}.  The first and the last bin always carry a seam size (the
    out-of-range entries clamp onto them); the slots the seams leave go to the other bins at random; slot positions are
    a random permutation, so every bin's slots are spread over the whole cloud."""
    rs = np.random.RandomState(seed)
    idx = np.empty((B, L), np.int64)
    plans = []
    for b in range(B):
        sizes = planned_sizes(L)
        inner = rs.permutation(np.arange(1, nbins - 1))
        bins = [0, nbins - 1] + list(inner[:len(sizes) - 2])
        plan = dict(zip(bins, sizes))
        vals = np.concatenate([np.full(s, k, np.int64) for k, s in plan.items()])
        rest = inner[len(sizes) - 2:]
        vals = np.concatenate([vals, rest[rs.randint(0, len(rest), L - len(vals))]])
        vals = vals[rs.permutation(L)]
        if out_of_range:  # half of the first bin's slots name -1, half of the last bin's name nbins
            lo, hi = np.flatnonzero(vals == 0), np.flatnonzero(vals == nbins - 1)
            vals[lo[::2]] = -1
            vals[hi[::2]] = nbins
        idx[b] = vals
        plans.append(plan)
    return idx, plans


def expected_table(idx, nbins, div, weight, flat):
    """start, order (, wsorted) as the library lays them out: per cloud (B, nbins + 1) / (B, L) with cloud-local slot
    ids, or flat over the batch, B * nbins + 1 starts and batch-wide slot ids."""
    B, L = idx.shape
    clipped = np.clip(idx, 0, nbins - 1)
    perm = np.stack([np.argsort(clipped[b], kind="stable") for b in range(B)])
    counts = np.stack([np.bincount(clipped[b], minlength=nbins) for b in range(B)])
    start = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(counts, axis=1)], axis=1)
    wsorted = None if weight is None else np.take_along_axis(weight, perm, axis=1)
    if flat:
        off = np.arange(B, dtype=np.int64)[:, None] * L
        start = np.concatenate([(start[:, :nbins] + off).reshape(-1), [B * L]])
        perm = perm + off
    return start.astype(np.int32), (perm // div).astype(np.int32), wsorted, counts


def expected_route(B, L, nbins):
    """csr_fits_lds, scatter_goes_flat and the workgroups-per-cloud rule of csr_transpose (csrc/inverse_table.hip)."""
    fits = L <= 65536 and ((4 * nbins + 15) // 16) * 16 + 2 * L <= 147456
    if L >= 2 * nbins and ((B == 1 and L >= 16384) or not fits):
        return "flat"
    if not fits:
        return "hbm"
    parts = 1
    while parts < 4 and B * parts * 2 <= 256 and nbins >= parts * 2 * 64 and L >= 8192:
        parts *= 2
    return "lds%d" % parts


@pytest.mark.parametrize("B,L,nbins,div,weighted,out_of_range,route", CASES)
def test_inverted_table_is_the_stable_argsort(B, L, nbins, div, weighted, out_of_range, route):
    idx, plans = make_idx(B, L, nbins, out_of_range, seed=B * L + nbins)
    weight = np.random.RandomState(7).rand(B, L).astype(np.float32) if weighted else None

    plan = (ctypes.c_int64 * 9)()
    assert _lib.load().tp3d_scatter_plan(B, L, nbins, int(weighted), ctypes.addressof(plan)) == 0
    flat = bool(plan[6])
    assert expected_route(B, L, nbins) == route and flat == (route == "flat"), (expected_route(B, L, nbins), flat)

    start, order, wsorted, counts = expected_table(idx, nbins, div, weight, flat)
    for b in range(B):  # the table asked for is the one planned: every seam size that fits, on its bin
        assert planned_sizes(L) == list(plans[b].values()) and len(plans[b]) >= 4
        assert all(counts[b, k] == s for k, s in plans[b].items()), (b, plans[b])
    if out_of_range:
        assert (idx == -1).sum() == 12 * B and (idx == nbins).sum() == 13 * B

    dev = torch.device(DEV)
    ws, nbytes = _lib.scatter_workspace(B, L, nbins, weighted, dev)
    assert nbytes == plan[5]
    ws.fill_(0xA5)
    t_idx = torch.from_numpy(idx).to(dev)
    t_w = None if weight is None else torch.from_numpy(weight).to(dev)
    with _lib.on_device(dev):
        _lib.call("tp3d_rows_scatter_invert", _lib.ptr(t_idx), _lib.ptr(t_w), B, L, div, nbins, _lib.ptr(ws), nbytes,
                  _lib.stream_ptr(dev))

    def view(off, n, dtype):
        return ws[off:off + 4 * n].view(dtype).cpu().numpy()

    got_start = view(plan[0], start.size, torch.int32)
    got_order = view(plan[1], B * L, torch.int32)
    assert np.array_equal(got_start, start.reshape(-1))
    assert np.array_equal(got_order, order.reshape(-1))
    if weighted:
        assert np.array_equal(view(plan[3], B * L, torch.float32), wsorted.reshape(-1))
    else:
        assert plan[3] == -1
