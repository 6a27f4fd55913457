"""The detection kernels of csrc/detection.hip on the device (torchpoints.box_nms / box3d_iou / box_best_gt / ap_match) and
what torch_points3d_amd.votenet builds on them (get_boxes, BoxSet, DetectionEvaluator).

References, none of them the code under test: the known answers of the reference's test/test_boxstuff.py; the stored
outputs of the reference's own nms_samecls, box3d_iou, eval_detection and get_boxes (tests/golden/votenet_boxes.npz); the
numpy / float64 restatement tests/votenet_ref.py.  Shapes: the smallest at which a kernel changes path -- P around the
wave (63, 64, 65), around the workgroup (256, 257, 300), around the 64 KiB of LDS a launch gets without asking (1771, 1772)
and the largest served (4096); pair counts below, at and above a workgroup.

Bars.  NMS and the matching flags: torch.equal (the NMS arithmetic is the reference's fp32 sequence bit for bit).  IoU:
both sides compute in float64 on the same inputs and differ by roundings only; the largest distance of the kernel to the
restatement on the cases below was measured as IOU_MEASURED (0: every operation is one IEEE rounding in the same
order on both sides), and the test allows 16x that, never more than 1e-12; the reference's hull area is within 1e-12.  AP within
1e-10 of the reference's."""
import pytest
import torch

import votenet_cases as vc
from torch_points3d_amd import detection_cpu
from torch_points3d_amd import votenet as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IOU_MEASURED = 0.0  # largest |kernel - restatement| over the cases of check_iou_fixture on an MI355X: bit-equal
IOU_BAR = 1e-12 if IOU_MEASURED is None else min(16 * IOU_MEASURED, 1e-12)


# ---------------------------------------------------------------------------------------------------- NMS
def test_nms_known_answers_ties_chain_and_zero_volume():
    vc.check_nms_known_answers(DEV)
    vc.check_nms_tie_chain_and_degenerate(DEV)


@pytest.mark.parametrize("B,P", vc.NMS_SHAPES)
def test_nms_fixture(B, P):
    """B = 1 and 3; P = 1, 2, 63, 64, 65, 256, 257, 300; one class, every box its own class, three classes; thresholds 0.25
    and 0.1; against the reference's stored picks and the restatement; a second call is bit-equal"""
    vc.check_nms_fixture(DEV, B, P)


@pytest.mark.parametrize("B,P", [(2, 1771), (1, 1772), (2, 4096)])
def test_nms_large_scenes(B, P):
    """the scene no longer fits the LDS a launch gets by default (P >= 1772), up to the largest P served.  The oracle is
    the vectorised numpy form (detection_cpu.box_nms), which tests/test_votenet_cpu.py holds to the reference's picks."""
    g = torch.Generator().manual_seed(P)
    lo = torch.rand(B, P, 3, generator=g) * 6.0
    boxes = torch.cat([lo, lo + 0.3 + torch.rand(B, P, 3, generator=g)], -1)
    scores = torch.rand(B, P, generator=g)
    scores[:, 5] = scores[:, 900]  # a tie
    cls = torch.randint(0, 2, (B, P), generator=g)
    want = torch.from_numpy(detection_cpu.box_nms(boxes.numpy(), scores.numpy(), cls.numpy(), 0.25))
    got = V.box_nms(boxes.to(DEV), scores.to(DEV), cls.to(DEV), 0.25)
    assert 0.05 * B * P < int(want.sum()) < 0.95 * B * P
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, V.box_nms(boxes.to(DEV), scores.to(DEV), cls.to(DEV), 0.25))


def test_nms_refuses_more_boxes_than_it_serves(hip):
    P = hip.BOX_NMS_MAX_BOXES + 1
    with pytest.raises(ValueError):
        hip.box_nms(torch.zeros(1, P, 6, device=DEV), torch.zeros(1, P, device=DEV), torch.zeros(1, P, dtype=torch.int64, device=DEV))
    empty = hip.box_nms(torch.zeros(2, 0, 6, device=DEV), torch.zeros(2, 0, device=DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    assert tuple(empty.shape) == (2, 0) and empty.dtype == torch.bool


# ---------------------------------------------------------------------------------------------------- IoU
def test_box_geometry_known_answers():
    vc.check_corner_and_volume_known_answers(DEV)
    vc.check_intersection_area_known_answers(DEV)


def test_iou_against_reference_values_and_the_float64_restatement():
    """(n, m) = (1, 1), (3, 5), (64, 65), (130, 7); headings arbitrary, 0 and quarter turns; identical, disjoint,
    face-sharing, nested and z-separated boxes"""
    from golden_util import report
    worst = vc.check_iou_fixture(DEV, IOU_BAR)
    report("detection", "box3d_iou_max_distance_to_restatement", worst)


def test_iou_empty_and_repeat(hip):
    g = vc.boxes_gold()
    c, c2 = g["iou/64x65/c1"].to(DEV), g["iou/64x65/c2"].to(DEV)
    assert tuple(hip.box3d_iou(c[:0], c).shape) == (0, 64) and tuple(hip.box3d_iou(c, c[:0]).shape) == (64, 0)
    assert torch.equal(hip.box3d_iou(c, c2), hip.box3d_iou(c, c2))
    # axis-aligned boxes against themselves: 1 up to the roundings of three edge lengths and their products (1e-15).  (A
    # ROTATED box against itself is outside the reference's domain: rounding splits collinear edges, its clip divides by
    # zero and its hull raises; the kernel returns NaN there.)
    flat = g["iou/3x5/c2"].to(DEV)
    assert float((torch.diagonal(hip.box3d_iou(flat, flat)) - 1.0).abs().max()) <= 1e-15
    with pytest.raises(ValueError):
        hip.box3d_iou(c.reshape(-1, 4, 6), c)


# ---------------------------------------------------------------------------------------------------- matching, AP
def test_matching_small_cases():
    """a group without ground truth, a group without detections, two detections on one box, equal scores, the exact
    quarter overlap (strict comparison), no detection at all"""
    vc.check_matching_small_cases(DEV)


def test_matching_and_ap_against_the_reference_s_eval_detection():
    vc.check_matching_fixture(DEV)
    vc.check_eval_detection_known_answer(DEV)


def test_best_gt_agrees_with_the_iou_matrix(hip):
    g = vc.boxes_gold()
    keys = ("det_corners", "det_class", "det_scene", "gt_corners", "gt_class", "gt_scene_start")
    dc, dcl, dsn, gc, gcl, start = [g["match/" + k].to(DEV) for k in keys]
    ovmax, jmax = hip.box_best_gt(dc, dcl, dsn, gc, gcl, start)
    iou = hip.box3d_iou(dc, gc)
    gt_scene = torch.repeat_interleave(torch.arange(3, device=DEV), start[1:] - start[:-1])
    ok = (dcl[:, None] == gcl[None]) & (dsn[:, None] == gt_scene[None])
    masked = torch.where(ok, iou, torch.full_like(iou, -1.0))
    pos = ovmax > 0  # (among boxes that do not overlap at all the first candidate wins; argmax need not agree)
    assert torch.equal(ovmax, masked.max(1)[0]) and torch.equal(jmax[pos], masked.argmax(1)[pos]) and int(pos.sum()) > 40


# ---------------------------------------------------------------------------------------------------- get_boxes
def test_get_boxes_known_answer_and_fixture():
    """B = 2, P = 16, a non-zero heading; with and without NMS and duplicate_boxes; corners 1e-5, scores 1e-6, order and
    classes exact against the reference's own list"""
    vc.check_get_boxes_known_answer(DEV)
    vc.check_get_boxes_fixture(DEV)


@pytest.mark.parametrize("dup", [False, True])
def test_get_boxes_reads_nothing_back_before_to_list(dup):
    """get_boxes under stream capture: any host read (an .item(), a boolean-mask index, a copy to the host) would end the
    capture with an error.  The replayed graph fills the same BoxSet, which is then read with to_list()."""
    g = vc.boxes_gold()
    res, ds = vc.results_from_gold(DEV)
    res.get_boxes(ds, apply_nms=True, duplicate_boxes=dup)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bs = res.get_boxes(ds, apply_nms=True, duplicate_boxes=dup)
        start = bs.scene_start
    graph.replay()
    torch.cuda.synchronize()
    vc.compare_box_list(bs.to_list(), g, True, dup)
    assert torch.equal(start.cpu(), g["boxes/out/nms1_dup%d/scene_start" % dup])

