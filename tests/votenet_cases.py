"""Checks shared by tests/test_votenet_cpu.py (CPU tensors: the numpy path of torch_points3d_amd.votenet) and
tests/test_gpu_detection.py / test_gpu_votenet.py (device tensors: csrc/detection.hip).  Every function takes the device.

References: the known answers of the reference's test/test_boxstuff.py, the stored outputs of the reference's own
functions (tests/golden/votenet_boxes.npz, votenet.npz; tests/golden/make_golden_votenet.py) and the float64 / numpy
restatement tests/votenet_ref.py, which the generator checked against the reference on the same inputs."""
import numpy as np
import torch

import votenet_ref as vr
from conftest import load_golden
from torch_points3d_amd import votenet as V
from torch_points3d_amd.dense import Data

NMS_SHAPES = [(1, 1), (1, 2), (3, 63), (1, 64), (3, 65), (1, 256), (3, 257), (1, 300)]
IOU_SHAPES = [(1, 1), (3, 5), (64, 65), (130, 7)]
AP_THRESHOLDS = [0.25, 0.5]
_cache = {}


def boxes_gold():
    if "boxes" not in _cache:
        _cache["boxes"] = load_golden("votenet_boxes")
    return _cache["boxes"]


def net_gold():
    if "net" not in _cache:
        _cache["net"] = load_golden("votenet")
    return _cache["net"]


def param_box(size, heading, centre, dev="cpu"):
    return V.box_corners_from_param(torch.tensor(size, dtype=torch.float32, device=dev), heading,
                                    torch.tensor(centre, dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------------------ known answers
def check_corner_and_volume_known_answers(dev):
    box = param_box([1, 2, 3], np.pi / 2, [1, 1, 1], dev)
    want = 1 + torch.tensor([[1.0, -0.5, -1.5], [1.0, 0.5, -1.5], [-1.0, 0.5, -1.5], [-1.0, -0.5, -1.5],
                             [1.0, -0.5, 1.5], [1.0, 0.5, 1.5], [-1.0, 0.5, 1.5], [-1.0, -0.5, 1.5]])
    torch.testing.assert_close(box.cpu(), want, rtol=1e-5, atol=1e-6)
    vol = V.box3d_vol(param_box([1, 2, 3], np.pi / 2, [0, 0, 0], dev))
    assert abs(float(vol) - 6.0) < 1e-6


def _prism(rect, dev):
    """a box of height 1 over a counter-clockwise rectangle given by its four (x, y) corners"""
    r = torch.tensor(rect, dtype=torch.float32)
    return torch.cat([torch.cat([r, torch.zeros(4, 1)], 1), torch.cat([r, torch.ones(4, 1)], 1)]).to(dev)


def check_intersection_area_known_answers(dev):
    """the three cases of test_intersection_area, read off the IoU of prisms of height 1: area = iou (v1 + v2) / (1 + iou)"""
    cases = [(param_box([1, 1, 1], 0, [0, 0, 0.5], dev), param_box([1, 1, 1], np.pi / 2, [0, 0, 0.5], dev), 1.0),
             (param_box([2, 2, 1], 0, [1, 1, 0.5], dev), param_box([2, 2, 1], 0, [0, 0, 0.5], dev), 1.0),
             (_prism([(0, 0), (1, 0), (1, 1), (0, 1)], dev), _prism([(0, 0), (1, 1), (0, 2), (-1, 1)], dev), 0.5)]
    for a, b, want in cases:
        iou = float(V.box3d_iou(a[None], b[None]))
        v = float(V.box3d_vol(a)) + float(V.box3d_vol(b))
        assert abs(iou * v / (1 + iou) - want) < 1e-5, (iou, want)
    one, small = param_box([2, 2, 3], 0, [1, 1, 0], dev), param_box([1, 1, 1], 0, [0.5, 0.5, 0.5], dev)
    assert abs(float(V.box3d_iou(one[None], small[None])) - 1.0 / 12) < 1e-12  # test_box3diou


def check_nms_known_answers(dev):
    boxes = torch.tensor([[[0, 0, 0, 1, 1, 1], [0, 0, 0, 0.5, 0.5, 0.5]]], dtype=torch.float32, device=dev)
    cls = torch.zeros(1, 2, dtype=torch.int64, device=dev)
    score = torch.tensor([[0.0, 1.0]], device=dev)
    assert V.box_nms(boxes, score, cls, 0.25).cpu().tolist() == [[True, True]]    # picks [1, 0]
    assert V.box_nms(boxes, score, cls, 0.1).cpu().tolist() == [[False, True]]    # picks [1]
    # TestVotenetResults.test_nms: every proposal is the same unit box
    hull = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.float32, device=dev).expand(2, 4, 6).contiguous()
    objectness = torch.tensor([[0, 1, 0.5, 0], [1, 0.8, 0, 0]], device=dev)
    classes = torch.tensor([[0, 0, 0, 0], [2, 1, 1, 1]], device=dev)
    keep = V.box_nms(hull, objectness, classes, 0.25)
    assert keep.cpu().tolist() == [[False, True, False, False], [True, True, False, False]]


def check_nms_tie_chain_and_degenerate(dev):
    unit = [0, 0, 0, 1, 1, 1]
    # equal scores on identical boxes: the higher index survives
    boxes = torch.tensor([[unit, unit, unit]], dtype=torch.float32, device=dev)
    keep = V.box_nms(boxes, torch.full((1, 3), 0.5, device=dev), torch.zeros(1, 3, dtype=torch.int64, device=dev), 0.25)
    assert keep.cpu().tolist() == [[False, False, True]]
    # a chain: A suppresses B; the dead B must not suppress C, which A does not reach
    chain = torch.tensor([[[0, 0, 0, 1, 1, 1], [0.5, 0, 0, 1.5, 1, 1], [1.0, 0, 0, 2.0, 1, 1]]], dtype=torch.float32, device=dev)
    keep = V.box_nms(chain, torch.tensor([[0.9, 0.8, 0.7]], device=dev), torch.zeros(1, 3, dtype=torch.int64, device=dev), 0.25)
    assert keep.cpu().tolist() == [[True, False, True]]
    # two boxes without volume: 0 / 0 is NaN, which compares false -- both stay
    flat = torch.tensor([[[0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0]]], dtype=torch.float32, device=dev)
    keep = V.box_nms(flat, torch.tensor([[0.9, 0.8]], device=dev), torch.zeros(1, 2, dtype=torch.int64, device=dev), 0.25)
    assert keep.cpu().tolist() == [[True, True]]


def check_nms_fixture(dev, B, P):
    g = boxes_gold()
    tag = "nms/%dx%d/" % (B, P)
    boxes, scores, mixed = g[tag + "boxes"], g[tag + "scores"], g[tag + "classes"]
    modes = {"one": torch.zeros(B, P, dtype=torch.int64), "own": torch.arange(P).repeat(B, 1), "mixed": mixed}
    for thr in (0.25, 0.1):
        for mode, cls in modes.items():
            want = g[tag + "keep/%s/%g" % (mode, thr)]
            got = V.box_nms(boxes.to(dev), scores.to(dev), cls.to(dev), thr)
            assert got.dtype == torch.bool and torch.equal(got.cpu(), want), (B, P, mode, thr)
            again = V.box_nms(boxes.to(dev), scores.to(dev), cls.to(dev), thr)
            assert torch.equal(got, again)
            if mode == "mixed":
                assert np.array_equal(vr.nms_mask(boxes.numpy(), cls.numpy(), scores.numpy(), thr), want.numpy())


def iou_cases():
    g = boxes_gold()
    out = [("%dx%d" % s, g["iou/%dx%d/c1" % s], g["iou/%dx%d/c2" % s], g["iou/%dx%d/ref" % s]) for s in IOU_SHAPES]
    s1, s2 = g["iou/special/c1"], g["iou/special/c2"]
    return out, (s1, s2, g["iou/special/ref"])


def check_iou_fixture(dev, bar):
    """every case against the float64 restatement within `bar` and against the reference's stored values (whose hull
    area differs from the shoelace sum by a few roundings: 1e-12); returns the largest distance to the restatement"""
    cases, (s1, s2, sref) = iou_cases()
    worst = 0.0
    for name, c1, c2, ref in cases:
        got = V.box3d_iou(c1.to(dev), c2.to(dev))
        assert got.dtype == torch.float64 and tuple(got.shape) == (c1.shape[0], c2.shape[0])
        got = got.cpu().numpy()
        want = vr.box3d_iou_matrix(c1.numpy(), c2.numpy())
        d = float(np.abs(got - want).max())
        print("box3d_iou %s: largest distance to the restatement %.3e, to the reference %.3e" % (
            name, d, float(np.abs(got - ref).max())))
        worst = max(worst, d)
        assert np.abs(got - ref).max() <= 1e-12
    got = V.box3d_iou(s1.to(dev), s2.to(dev)).cpu().numpy()
    diag = np.diagonal(got)
    want = np.array([vr.box3d_iou(a, b) for a, b in zip(s1.numpy(), s2.numpy())])
    worst = max(worst, float(np.abs(diag - want).max()))
    assert diag[0] == 1.0 and diag[1] == 0.0 and diag[2] == 0.0 and diag[4] == 0.0  # identical, disjoint, face, z apart
    assert abs(diag[3] - 1.0 / 27) < 1e-7 and abs(diag[6] - 1.0 / 12) < 1e-7 and np.abs(diag - sref).max() <= 1e-12
    print("box3d_iou: largest distance to the restatement over all cases %.3e (bar %.3e)" % (worst, bar))
    assert worst <= bar
    return worst


def _match_inputs(dev):
    g = boxes_gold()
    keys = ("det_corners", "det_score", "det_class", "det_scene", "gt_corners", "gt_class", "gt_scene_start")
    return g, [g["match/" + k].to(dev) for k in keys]


def _sets(dev, det_c, det_s, det_cls, det_scene, gt_c, gt_cls, gt_scene, S):
    t = lambda v, dt: torch.as_tensor(np.asarray(v), dtype=dt).to(dev)  # noqa: E731
    det = V.BoxSet(t(det_c, torch.float32).reshape(-1, 8, 3), t(det_cls, torch.int64), t(det_scene, torch.int64),
                   torch.ones(len(det_cls), dtype=torch.bool, device=dev), S, t(det_s, torch.float32))
    gt = V.BoxSet(t(gt_c, torch.float32).reshape(-1, 8, 3), t(gt_cls, torch.int64), t(gt_scene, torch.int64),
                  torch.ones(len(gt_cls), dtype=torch.bool, device=dev), S)
    return det, gt


def check_matching_small_cases(dev):
    unit = param_box([1, 1, 1], 0, [0.5, 0.5, 0.5]).numpy()
    far = param_box([1, 1, 1], 0, [9, 9, 9]).numpy()
    # scene 0: two detections on one box (the second is a false positive); scene 1: ground truth without detections;
    # scene 2: detections without ground truth; scene 0 also holds a detection of a class without ground truth
    det, gt = _sets(dev, [unit, unit, unit, far, unit], [0.9, 0.8, 0.7, 0.6, 0.5], [0, 0, 1, 0, 0], [0, 0, 0, 2, 2],
                    [unit, unit], [0, 0], [0, 1], 3)
    tp, ovmax, jmax = V.ap_match(det, gt, AP_THRESHOLDS)
    assert tp.cpu().tolist() == [[True, True], [False, False], [False, False], [False, False], [False, False]]
    assert jmax.cpu().tolist() == [0, 0, -1, -1, -1]
    assert ovmax.cpu().tolist()[:2] == [1.0, 1.0] and bool(torch.isinf(ovmax[2:]).all()) and bool((ovmax[2:] < 0).all())
    # equal scores keep input order: the first of two equal detections takes the box
    det, gt = _sets(dev, [unit, unit], [0.5, 0.5], [0, 0], [0, 0], [unit], [0], [0], 1)
    assert V.ap_match(det, gt, [0.25])[0].cpu().tolist() == [[True], [False]]
    # the exact case: IoU 0.25 is not above 0.25
    g = boxes_gold()
    assert "match/exact/a" in g, "the generator dropped the exact case"
    det, gt = _sets(dev, [g["match/exact/a"].numpy()], [0.9], [0], [0], [g["match/exact/b"].numpy()], [0], [0], 1)
    tp, ovmax, _ = V.ap_match(det, gt, [0.25, 0.2])
    assert float(ovmax[0]) == 0.25 and tp.cpu().tolist() == [[False, True]]
    # no detection at all
    ev = V.DetectionEvaluator()
    empty, gt = _sets(dev, np.zeros((0, 8, 3)), [], [], [], [unit], [0], [0], 1)
    ev.add(empty, gt)
    rec, prec, ap = ev.finalise([0.25])
    assert rec[0.25][0] == 0 and prec[0.25][0] == 0 and ap[0.25][0] == 0


def check_matching_fixture(dev):
    g, (dc, ds, dcl, dsn, gc, gcl, start) = _match_inputs(dev)
    S = start.shape[0] - 1
    gt_scene = torch.repeat_interleave(torch.arange(S, device=start.device), start[1:] - start[:-1])
    det, gt = _sets(dev, dc.cpu(), ds.cpu(), dcl.cpu(), dsn.cpu(), gc.cpu(), gcl.cpu(), gt_scene.cpu(), S)
    ev = V.DetectionEvaluator()
    ev.add(det, gt)
    _, _, tp, ovmax, jmax = ev.match(AP_THRESHOLDS)
    assert torch.equal(tp.cpu(), g["match/tp"]) and torch.equal(jmax.cpu(), g["match/jmax"])
    assert np.abs(ovmax.cpu().numpy() - g["match/ovmax"]).max() <= 1e-12
    rec, prec, ap = ev.finalise(AP_THRESHOLDS)
    for thr in AP_THRESHOLDS:
        for c in range(3):
            assert np.array_equal(rec[thr][c], g["match/ref/%g/rec/%d" % (thr, c)])
            assert np.array_equal(prec[thr][c], g["match/ref/%g/prec/%d" % (thr, c)])
            assert abs(ap[thr][c] - float(g["match/ref/%g/ap/%d" % (thr, c)][0])) <= 1e-10
    # split over two add() calls (scenes 0-1, then scene 2): the same curves
    ev2 = V.DetectionEvaluator()
    for lo, hi in ((0, 2), (2, 3)):
        d = (dsn.cpu() >= lo) & (dsn.cpu() < hi)
        q = (gt_scene.cpu() >= lo) & (gt_scene.cpu() < hi)
        a, b = _sets(dev, dc.cpu()[d], ds.cpu()[d], dcl.cpu()[d], dsn.cpu()[d] - lo, gc.cpu()[q], gcl.cpu()[q],
                     gt_scene.cpu()[q] - lo, hi - lo)
        ev2.add(a, b)
    ap2 = ev2.finalise(AP_THRESHOLDS)[2]
    assert all(ap2[t][c] == ap[t][c] for t in AP_THRESHOLDS for c in range(3))


def check_eval_detection_known_answer(dev):
    box = param_box([1, 1, 1], 0, [0.5, 0.5, 0.5])
    gt = {"0": [V.BoxData("class1", box), V.BoxData("class2", box)], "1": [V.BoxData("class1", box)]}
    pred = {"0": [V.BoxData("class1", box, score=0.5), V.BoxData("class2", box, score=0.5)],
            "1": [V.BoxData("class2", box, score=1)]}
    rec, prec, ap = V.eval_detection(pred, gt, device=dev)
    np.testing.assert_allclose(rec["class2"], np.asarray([0, 1]))
    np.testing.assert_allclose(prec["class2"], np.asarray([0, 0.5]))
    assert abs(ap["class2"] - 0.5) < 1e-12


# ------------------------------------------------------------------------------------------------ get_boxes
class BoxDataset(object):
    def __init__(self, mean_size_arr):
        self.mean_size_arr = mean_size_arr


def results_from_gold(dev):
    g = boxes_gold()
    res = V.VoteNetResults(**{k[len("boxes/in/"):]: v.to(dev) for k, v in g.items() if k.startswith("boxes/in/")})
    res.has_class = True
    return res, BoxDataset(g["boxes/mean_size_arr"].to(dev))


def compare_box_list(got, g, nms, dup):
    tag = "boxes/out/nms%d_dup%d/" % (nms, dup)
    start = g[tag + "scene_start"].tolist()
    assert [len(s) for s in got] == [b - a for a, b in zip(start[:-1], start[1:])], (nms, dup)
    k = 0
    for scene in got:
        for box in scene:
            assert int(box.classname) == int(g[tag + "classname"][k])
            assert np.abs(box.corners3d - g[tag + "corners"][k].numpy()).max() <= 1e-5
            assert abs(box.score - float(g[tag + "score"][k])) <= 1e-6
            k += 1


def check_get_boxes_fixture(dev):
    g = boxes_gold()
    res, ds = results_from_gold(dev)
    for nms in (False, True):
        for dup in (False, True):
            bs = res.get_boxes(ds, apply_nms=nms, duplicate_boxes=dup)
            assert isinstance(bs, V.BoxSet) and bs.num_scenes == 2
            compare_box_list(bs.to_list(), g, nms, dup)
            tag = "boxes/out/nms%d_dup%d/" % (nms, dup)
            assert torch.equal(bs.scene_start.cpu(), g[tag + "scene_start"])
            assert tuple(bs.corners.shape) == (len(g[tag + "score"]), 8, 3) and bs.classname.dtype == torch.int64


def check_get_boxes_known_answer(dev):
    """TestVotenetResults.test_getboxes: unit boxes at the origin, score 0.5, every proposal kept"""
    B, P = 2, 4
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    res = V.VoteNetResults(center=z(B, P, 3), heading_scores=z(B, P, 1), heading_residuals=z(B, P, 1), size_scores=z(B, P, 1),
                           size_residuals=z(B, P, 2, 3), objectness_scores=torch.ones(B, P, 2, device=dev),
                           sem_cls_scores=torch.ones(B, P, 1, device=dev))

    class Mock(object):
        mean_size_arr = [[1, 1, 1], [0, 0, 0]]

        def class2angle(self, classname, residual):
            return 0

    boxes = res.get_boxes(Mock()).to_list()
    assert len(boxes) == B and len(boxes[0]) == P
    want = np.asarray([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [0.5, 0.5, -0.5], [-0.5, 0.5, -0.5],
                       [-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, 0.5], [-0.5, 0.5, 0.5]])
    np.testing.assert_allclose(boxes[0][0].corners3d, want)
    assert abs(boxes[0][0].score - 0.5) < 1e-7


# ------------------------------------------------------------------------------------------------ the network
MEAN_SIZE = [[0.4, 0.4, 0.4], [0.6, 0.3, 0.5], [0.3, 0.7, 0.4], [0.5, 0.5, 0.8]]
STAGE_KEYS = ("objectness_scores", "heading_scores", "heading_residuals_normalized", "size_scores",
              "size_residuals_normalized", "sem_cls_scores", "center")
LOSS_KEYS = ("vote_loss", "objectness_loss", "center_loss", "heading_cls_loss", "heading_reg_loss", "size_cls_loss",
             "size_reg_loss", "sem_cls_loss", "box_loss", "loss")


def reduced_config():
    return V.votenet_config("VoteNetPaper", 1, 4, MEAN_SIZE, in_feat=8, num_features=32, num_proposal=16, num_seeds=64,
                            npoint=(128, 64, 32, 16), nsamples=((16,), (8,), (8,), (8,)), agg_nsample=16)


def build_net(g, dev, kernels=None, fused=True):
    net = V.VoteNet(reduced_config(), feat=1, num_classes=4, mean_size_arr=MEAN_SIZE, kernels=kernels, fused=fused)
    net.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")}, strict=True)  # the reference's keys
    return net.to(dev).train()


def labels_of(g, dev):
    lab = {k[len("label/"):]: v.to(dev) for k, v in g.items() if k.startswith("label/")}
    lab["pos"] = g["pos"].to(dev)
    return lab


def bound(fp32, fp64, floor=1e-5):
    own = float((fp32.double().cpu() - torch.as_tensor(fp64)).abs().max())
    return max(floor, 2.0 * own)


def close(got, g, key, what=None):
    want = g[key]
    torch.testing.assert_close(got.detach().cpu(), want, rtol=1e-5, atol=bound(want, g["f64/" + key]),
                               msg=lambda m: "%s: %s" % (what or key, m))


def check_stages_teacher_forced(g, net, dev, report=None):
    """every stage on the FIXTURE's inputs for that stage: rtol 1e-5, atol 1e-5 or twice the reference pass's own
    distance to its float64 evaluation"""
    bb = net.backbone_model
    x0 = g["x"].to(dev).transpose(1, 2)
    fused = getattr(bb, "fused", False) and x0.is_cuda and bb._kernels_are_hip
    cur = Data(pos=g["pos"].to(dev), x=x0 if fused else x0.contiguous())
    skips = [cur]
    for i in range(4):
        out = bb.down_modules[i](cur)
        assert torch.equal(out.pos.cpu(), g["down%d_pos" % i])
        close(out.x, g, "down%d_x" % i)
        if i == 0:
            assert torch.equal(out.sampling_id_0.cpu(), g["sampling_id_0"])
        cur = Data(pos=g["down%d_pos" % i].to(dev), x=g["down%d_x" % i].to(dev))
        if i < 3:
            skips.append(cur)
    for i in range(2):
        out = bb.up_modules[i]((cur, skips.pop()))
        close(out.x, g, "up%d_x" % i)
        cur = Data(pos=out.pos, x=g["up%d_x" % i].to(dev))
    assert torch.equal(cur.pos.cpu(), g["down1_pos"])
    votes = net.voting_module(Data(pos=cur.pos, x=cur.x))
    close(votes.pos, g, "vote_pos")
    close(votes.x, g, "vote_x")
    votes = Data(pos=g["vote_pos"].to(dev), x=g["vote_x"].to(dev), seed_pos=cur.pos,
                 seed_inds=g["sampling_id_0"][:, :64].to(dev))
    res = net.proposal_cls_module(votes)
    assert torch.equal(res.sampled_votes.cpu(), g["sampled_votes"])
    for k in STAGE_KEYS:
        close(res[k], g, k)


def check_chained_pass(g, net, dev, report=None):
    """the whole training pass: distance to the stored float64 pass <= 4x max and 2x RMS of the reference pass's own (floor
    1e-5 / 2.5e-6); assignments exact; every loss term against float64; gradients by relative L2 <= max(1e-4, 4x the
    reference's own fp32-to-fp64 distance stored in the fixture); BatchNorm buffers; eval mode 1e-5 * scale"""
    data = Data(pos=g["pos"].to(dev), x=g["x"].to(dev))
    res = net(data, labels=labels_of(g, dev))
    assert torch.equal(res.seed_inds.cpu(), g["sampling_id_0"][:, :64])
    assert torch.equal(res.sampled_votes.cpu(), g["sampled_votes"]) or \
        float((res.sampled_votes.cpu() - g["sampled_votes"]).abs().max()) < 1e-5
    for k in ("objectness_label", "object_assignment"):
        assert torch.equal(res[k].cpu(), g[k]), k
    assert torch.equal(res.objectness_mask.cpu(), g["objectness_mask"])
    for k in STAGE_KEYS:
        d = res[k].detach().double().cpu() - torch.as_tensor(g["f64/" + k])
        own = g[k].double() - torch.as_tensor(g["f64/" + k])
        got_max, got_rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
        own_max, own_rms = float(own.abs().max()), float(own.pow(2).mean().sqrt())
        if report:
            report("votenet_chained", k, dict(max=got_max, rms=got_rms, ref_max=own_max, ref_rms=own_rms))
        print("chained %s vs float64: max %.3e (reference pass %.3e), rms %.3e (reference pass %.3e)" % (
            k, got_max, own_max, got_rms, own_rms))
        assert got_max <= max(1e-5, 4 * own_max) and got_rms <= max(2.5e-6, 2 * own_rms), (k, got_max, own_max, got_rms, own_rms)
    for k in LOSS_KEYS:
        want64 = float(g["f64/loss/" + k])
        own = abs(float(g["loss/" + k]) - want64)
        got = float(net.losses[k])
        tol = max(1e-5 * max(1.0, abs(want64)), 4 * own)
        if report:
            report("votenet_loss", k, dict(got=got, f64=want64, ref_fp32_distance=own))
        print("loss %s: %.7f (float64 %.7f, reference fp32 off by %.2e, bar %.2e)" % (k, got, want64, own, tol))
        assert abs(got - want64) <= tol, (k, got, want64, tol)
    net.losses["loss"].backward()
    checked = 0
    for name, p in net.named_parameters():
        want = g.get("f64/pgrad/" + name)
        if want is None or "grel/" + name not in g:
            continue  # no gradient (mean_size_arr), or analytically zero (a bias in front of a train-mode BatchNorm)
        want = torch.as_tensor(want)
        tol = max(1e-4, 4.0 * float(g["grel/" + name][0]))
        rel = float((p.grad.double().cpu() - want).norm() / (want.norm() + 1e-300))
        if report:
            report("votenet_grad", name, dict(rel_l2=rel, bar=tol))
        assert rel <= tol, (name, rel, tol)
        checked += 1
    assert checked > 60, checked
    sd = net.state_dict()
    after = {k[len("after/"):]: v for k, v in g.items() if k.startswith("after/")}
    assert len(after) > 40
    for name, v in after.items():
        if name.endswith("num_batches_tracked"):
            assert int(sd[name]) == int(v), name
        else:
            torch.testing.assert_close(sd[name].cpu(), v, rtol=1e-4, atol=1e-5, msg=name)
    net.eval()
    with torch.no_grad():
        ev = net(Data(pos=g["pos"].to(dev), x=g["x"].to(dev)))
    for k in STAGE_KEYS:
        want = g["eval/" + k]
        torch.testing.assert_close(ev[k].cpu(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())), msg=k)
