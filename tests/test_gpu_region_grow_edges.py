"""Region growing (csrc/region_grow.hip, torchpoints.region_grow_csr) at the limits of its sort key's fields, at the cell
seams and under adversarial orders -- where test_gpu_region_grow.py checks the middle of the domain.

Clusters are index sets, so every comparison is exact.  The references are that file's: torch_points_kernels.region_grow
on CPU copies (`host`), the float64 connected components (pointgroup_util.components_reference), and, in addition, the
literal list wherever the construction dictates it (`want` of the generator).  Every generator of pointgroup_util keeps
all pairs 2 % away from the radius and the neighbour counts within the nsample in use (asserted there, and held to the
references on the CPU by test_pointgroup_cpu.py), so the capped walk and the uncapped components coincide and the call
must take the device route."""
import numpy as np
import pytest
import torch

import pointgroup_util as pgu
from test_gpu_region_grow import DEV, check_csr, grow, host, pile
from torch_points3d_amd import torchpoints as tp

pytestmark = pytest.mark.gpu
FIELDS = ("members", "starts", "member_cluster", "label", "cloud")


def components(s, ignore=pgu.IGNORE, radius=pgu.RADIUS, min_cluster_size=pgu.MIN_CLUSTER_SIZE):
    return pgu.components_reference(s["pos"], s["labels"], s["batch"], list(ignore), radius, min_cluster_size)


def flagged(s, text, **kw):
    """an input beyond a key field: cap=None refuses it and names the flag, the reference's cap sends it to the host"""
    with pytest.raises(ValueError, match=text):
        grow(s, cap=None, **kw)
    a = grow(s, **kw)
    assert a.route == "host"
    check_csr(a, s, host(s, **kw))


# ---- 1. shifted scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(pgu.SHIFTS))
def test_shifted_scene(which):
    s = pgu.scene_shifted(which)
    a = grow(s)
    assert a.route == "device"
    want = host(s)
    assert want == pgu.scene_reference()  # a translation changes no membership
    check_csr(a, s, want)


# ---- 2. the coordinate flag -----------------------------------------------------------------------------------------
def test_coordinate_flag():
    flagged(pgu.scene_with_far_point(1e6), "coordinate")
    for x in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="coordinate"):
            grow(pgu.scene_with_far_point(x), cap=None)


# ---- 3. label and cloud limits --------------------------------------------------------------------------------------
def test_label_and_cloud_limits():
    s = pgu.pairs26_fields()
    a = grow(s, ignore_labels=(), min_cluster_size=2)
    assert a.route == "device"
    want = host(s, ignore_labels=(), min_cluster_size=2)  # (the CPU path takes cloud ids with gaps)
    assert want == s["want"] and want == components(s, (), min_cluster_size=2)
    check_csr(a, s, want)
    assert sorted(set(zip(a.label.tolist(), a.cloud.tolist()))) == [(l, c) for l in pgu.FIELD_LABELS for c in pgu.FIELD_CLOUDS]
    keys = [(int(s["labels"][c[0]]), c[0]) for c in want]
    assert keys == sorted(keys)


@pytest.mark.parametrize("extra,text", [("label4095", "label"), ("label-1", "label"), ("cloud1024", "cloud id")])
def test_one_point_beyond_a_key_field(extra, text):
    flagged(pgu.pairs26_fields(extra), text, ignore_labels=(), min_cluster_size=2)


def test_ignored_labels_raise_no_flag():
    s = pgu.pairs26_fields("ignored")  # labels -1 and 5000 are present and both ignored
    for cap in ("reference", None):
        a = grow(s, ignore_labels=s["ignore"], min_cluster_size=2, cap=cap)
        assert a.route == "device"
        want = host(s, ignore_labels=s["ignore"], min_cluster_size=2)
        assert want == s["want"]
        check_csr(a, s, want)
    a = grow(s, ignore_labels=torch.tensor([5000, 0, -1]), min_cluster_size=2, cap=None)  # several entries, as a tensor
    assert a.route == "device"
    check_csr(a, s, components(s, (5000, 0, -1), min_cluster_size=2))


# ---- 4. the span limit, per axis ------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_span_limit(axis):
    s = pgu.span_limit(axis, pgu.CELL_MAX)  # asserts the intended cells in fp32
    cells = s["cells"]
    assert cells[:, axis].min() == 0 and cells[:, axis].max() == pgu.CELL_MAX == 16381
    a = grow(s, min_cluster_size=3)
    assert a.route == "device"
    want = host(s, min_cluster_size=3)
    assert want == s["want"]
    check_csr(a, s, want)
    over = pgu.span_limit(axis, pgu.CELL_MAX + 1)
    assert over["cells"][:, axis].max() == 16382
    flagged(over, "cells along an axis", min_cluster_size=3)


# ---- 5. each of the 26 neighbour cells as the only link of a pair ----------------------------------------------------
@pytest.mark.parametrize("swap", [False, True])
def test_twenty_six_neighbour_cells(swap):
    s = pgu.pairs26(swap)  # asserts that the cells of every pair differ by exactly its direction
    a = grow(s, min_cluster_size=2)
    assert a.route == "device"
    want = host(s, min_cluster_size=2)
    assert want == [[2 * i, 2 * i + 1] for i in range(26)] and want == components(s, min_cluster_size=2)
    check_csr(a, s, want)


# ---- 6. x-runs longer than one wave ---------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [63, 64, 65, 128, 129])
def test_long_x_runs(count):
    s = pile(count)
    a = grow(s, nsample=300)
    assert a.route == "device"
    want = host(s, nsample=300)
    assert want == [list(range(1, count + 1))]
    check_csr(a, s, want)
    # three consecutive runs of `count`: the middle cell's points scan all of them
    s = pgu.pile3(count)
    a = grow(s, cap=None)
    assert a.route == "device"
    want = components(s)
    assert want == s["want"]
    check_csr(a, s, want)
    if 3 * count <= 300:  # ... and under the reference's cap where the neighbourhoods fit it
        a = grow(s, nsample=300)
        assert a.route == "device"
        assert host(s, nsample=300) == want
        check_csr(a, s, want)
    else:
        assert grow(s, nsample=300).route == "host"


# ---- 7. strict membership -------------------------------------------------------------------------------------------
def test_strict_membership():
    s = pgu.strict_pairs()
    kw = dict(radius=pgu.STRICT_RADIUS, min_cluster_size=1)
    a = grow(s, **kw)
    assert a.route == "device"
    want = host(s, **kw)
    assert want == [[0], [1], [2, 3]]
    check_csr(a, s, want)


# ---- 8. the run scan at its chunk seams -----------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [1, 1023, 1024, 1025, 2049])
def test_scan_seams_singles(runs):
    s = pgu.line_of_singles(runs)
    a = grow(s, min_cluster_size=1)
    assert a.route == "device" and len(a) == runs
    assert torch.equal(a.starts.cpu(), torch.arange(runs + 1)) and torch.equal(a.members.cpu(), torch.arange(runs))
    want = components(s, min_cluster_size=1)
    assert want == [[i] for i in range(runs)]
    check_csr(a, s, want)


@pytest.mark.parametrize("ignored", [0, 100])
def test_scan_seams_alternating(ignored):
    s = pgu.alternating_runs(2049, ignored)
    assert int((s["labels"] == 0).sum()) == ignored
    a = grow(s, min_cluster_size=2)
    assert a.route == "device"
    want = components(s, min_cluster_size=2)
    assert want == s["want"] and len(want) == 1025 and want == host(s, min_cluster_size=2)
    check_csr(a, s, want)


# ---- 9. index orders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "bitrev"])
def test_chain_index_orders(order):
    s = pgu.snake_chain(order)
    a = grow(s)
    assert a.route == "device"
    want = host(s)
    assert want == [list(range(2910))] and want == components(s)
    check_csr(a, s, want)
    b = grow(s)
    for name in FIELDS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scene_under_further_permutations(seed):
    s = pgu.scene_permuted(seed)
    a = grow(s)
    assert a.route == "device"
    got = [c.tolist() for c in a.to_list()]
    assert all(c == sorted(c) for c in got)
    keys = [(int(s["labels"][c[0]]), c[0]) for c in got]
    assert keys == sorted(keys)
    assert pgu.map_back(got, s) == pgu.scene_reference()


# ---- 10. stale workspace and argument forms ---------------------------------------------------------------------------
def test_small_call_on_a_stale_workspace():
    big, small = pgu.scene(), pgu.strict_pairs()
    a = grow(big)
    b = grow(small, radius=pgu.STRICT_RADIUS, min_cluster_size=1)
    c = grow(big)
    assert b.route == "device"
    check_csr(b, small, [[0], [1], [2, 3]])
    check_csr(a, big, pgu.scene_reference())
    for name in FIELDS:
        assert torch.equal(getattr(a, name), getattr(c, name)), name


def test_argument_forms():
    s = pgu.scene()
    n = s["pos"].shape[0]
    buf = torch.full((n, 4), float("nan"))
    buf[:, :3] = s["pos"]
    pos = buf.to(DEV)[:, :3]
    assert not pos.is_contiguous()
    kw = dict(ignore_labels=pgu.IGNORE, radius=pgu.RADIUS, nsample=pgu.NSAMPLE, min_cluster_size=pgu.MIN_CLUSTER_SIZE)
    a = tp.region_grow_csr(pos, s["labels"].int().to(DEV), s["batch"].int().to(DEV), **kw)
    b = grow(s)
    assert a.route == b.route == "device"
    for name in FIELDS:
        assert getattr(a, name).dtype == torch.int64 and torch.equal(getattr(a, name), getattr(b, name)), name
    check_csr(a, s, pgu.scene_reference())
