"""Plain numpy / Python restatement of the reference's box post-processing, the oracle of the detection tests:
  nms_samecls        utils/box_utils.py:28-85      (fp32, explicit stable order)
  box3d_iou          utils/box_utils.py:88-182     (float64; the hull area replaced by the shoelace sum of the clip)
  eval_det_cls       metrics/box_detection/ap.py:35-118 (grouped by scene and class, explicit stable order)
  voc_ap             metrics/box_detection/ap.py:10-32
  get_boxes          modules/VoteNet/votenet_results.py:155-255 (the host loop, box by box)
tests/golden/make_golden_votenet.py asserts that these agree with the reference's own functions on the fixture inputs.
Loops are written out on purpose: nothing here is shared with the code under test."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ NMS
def nms_order(scores):
    """descending score, among equal scores the higher index first: a stable ascending sort read from the back"""
    return np.argsort(np.asarray(scores, dtype=F32), kind="stable")[::-1]


def nms_samecls(boxes, classes, scores, overlap_threshold=0.25):
    """the picks of the reference, in picking order (fp32 arithmetic, threshold rounded to fp32)"""
    boxes = np.asarray(boxes, dtype=F32)
    classes = np.asarray(classes)
    thr = F32(overlap_threshold)
    x1, y1, z1, x2, y2, z2 = [boxes[:, k] for k in range(6)]
    area = (x2 - x1) * (y2 - y1) * (z2 - z1)
    order = list(nms_order(scores))
    alive = [True] * len(order)
    pick = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, i in enumerate(order):
            if not alive[a]:
                continue
            pick.append(int(i))
            for b in range(a + 1, len(order)):
                if not alive[b]:
                    continue
                j = order[b]
                l = np.maximum(F32(0), np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j]))
                w = np.maximum(F32(0), np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j]))
                h = np.maximum(F32(0), np.minimum(z2[i], z2[j]) - np.maximum(z1[i], z1[j]))
                inter = l * w * h
                o = inter / (area[i] + area[j] - inter)
                o = o * F32(classes[i] == classes[j])
                assert o.dtype == F32
                if o > thr:
                    alive[b] = False
    return pick


def nms_mask(boxes, classes, scores, overlap_threshold=0.25):
    """(B, P) bool keep mask of nms_samecls scene by scene"""
    boxes = np.asarray(boxes)
    mask = np.zeros(boxes.shape[:2], dtype=bool)
    for b in range(boxes.shape[0]):
        mask[b, nms_samecls(boxes[b], np.asarray(classes)[b], np.asarray(scores)[b], overlap_threshold)] = True
    return mask


# ------------------------------------------------------------------------------------------------ rotated IoU
def polygon_clip(subject, clip):
    """utils/box_utils.py:135-182 verbatim in structure: strict inside test, the same computeIntersection"""
    out = [(float(p[0]), float(p[1])) for p in subject]
    cp1 = (float(clip[-1][0]), float(clip[-1][1]))
    most = len(out)
    for cv in clip:
        cp2 = (float(cv[0]), float(cv[1]))

        def inside(p):
            return (cp2[0] - cp1[0]) * (p[1] - cp1[1]) > (cp2[1] - cp1[1]) * (p[0] - cp1[0])

        def intersection(s, e):
            dc = (cp1[0] - cp2[0], cp1[1] - cp2[1])
            dp = (s[0] - e[0], s[1] - e[1])
            n1 = cp1[0] * cp2[1] - cp1[1] * cp2[0]
            n2 = s[0] * e[1] - s[1] * e[0]
            n3 = 1.0 / (dc[0] * dp[1] - dc[1] * dp[0])
            return ((n1 * dp[0] - n2 * dc[0]) * n3, (n1 * dp[1] - n2 * dc[1]) * n3)

        inp, out = out, []
        s = inp[-1]
        for e in inp:
            if inside(e):
                if not inside(s):
                    out.append(intersection(s, e))
                out.append(e)
            elif inside(s):
                out.append(intersection(s, e))
            s = e
        cp1 = cp2
        most = max(most, len(out))
        if not out:
            return None, most
    return out, most


def shoelace(poly):
    s = 0.0
    n = len(poly)
    for k in range(n):
        p, q = poly[k], poly[(k + 1) % n]
        s = s + (p[0] * q[1] - q[0] * p[1])
    return 0.5 * abs(s)


def intersection_area(rect1, rect2):
    poly, _ = polygon_clip(rect1, rect2)
    return 0.0 if poly is None else shoelace(poly)


def box3d_vol(c):
    c = np.asarray(c, dtype=np.float64)

    def edge(i, j):
        d = c[i] - c[j]
        return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))

    return edge(0, 1) * edge(1, 2) * edge(0, 4)


def box3d_iou(c1, c2):
    """float64 on the (promoted) corners"""
    c1 = np.asarray(c1).astype(np.float64)
    c2 = np.asarray(c2).astype(np.float64)
    area = intersection_area([(c1[i, 0], c1[i, 1]) for i in range(4)], [(c2[i, 0], c2[i, 1]) for i in range(4)])
    zmin = max(c1[0, 2], c2[0, 2])
    zmax = min(c1[4, 2], c2[4, 2])
    inter = area * max(0.0, zmax - zmin)
    v1, v2 = box3d_vol(c1), box3d_vol(c2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(inter) / np.float64((v1 + v2) - inter))


def box3d_iou_matrix(c1, c2):
    out = np.zeros((len(c1), len(c2)), dtype=np.float64)
    for i in range(len(c1)):
        for j in range(len(c2)):
            out[i, j] = box3d_iou(c1[i], c2[j])
    return out


# ------------------------------------------------------------------------------------------------ AP matching
def ap_match(det_corners, det_score, det_class, det_scene, gt_corners, gt_class, gt_scene_start, thresholds):
    """(tp (D, T) bool, ovmax (D,), jmax (D,)): eval_det_cls's loop for every (scene, class) group; jmax is a row of
    gt_corners (-1 without a candidate); equal scores keep input order"""
    D = len(det_corners)
    T = len(thresholds)
    tp = np.zeros((D, T), dtype=bool)
    ovmax = np.full((D,), -np.inf)
    jmax = np.full((D,), -1, dtype=np.int64)
    S = len(gt_scene_start) - 1
    for d in range(D):
        s = int(det_scene[d])
        if not 0 <= s < S:
            continue
        for j in range(int(gt_scene_start[s]), int(gt_scene_start[s + 1])):
            if gt_class[j] != det_class[d]:
                continue
            iou = box3d_iou(det_corners[d], gt_corners[j])
            if iou > ovmax[d]:
                ovmax[d], jmax[d] = iou, j
    order = np.argsort(-np.asarray(det_score, dtype=np.float64), kind="stable")
    for t, thr in enumerate(thresholds):
        taken = set()
        for d in order:  # the global order restricted to a group is the group's order
            key = (int(det_scene[d]), int(det_class[d]), int(jmax[d]))
            if jmax[d] >= 0 and ovmax[d] > thr and key not in taken:
                taken.add(key)
                tp[d, t] = True
    return tp, ovmax, jmax


def voc_ap(rec, prec):
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def class_curves(tp, det_score, det_class, gt_class):
    """{class: (rec, prec, ap)} from the flags of one threshold, as eval_det_cls ends and eval_detection collects: classes
    of the ground truth; a class without detections gets 0, 0, 0"""
    out = {}
    det_class = np.asarray(det_class)
    gt_class = np.asarray(gt_class)
    score = np.asarray(det_score, dtype=np.float64)
    for c in sorted(set(gt_class.tolist()) | set(det_class.tolist())):
        sel = np.where(det_class == c)[0]
        npos = int((gt_class == c).sum())
        if len(sel) == 0:
            out[c] = (0, 0, 0)
            continue
        sel = sel[np.argsort(-score[sel], kind="stable")]
        t = np.cumsum(tp[sel].astype(np.float64))
        f = np.cumsum((~tp[sel]).astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            rec = t / float(npos)
        prec = t / np.maximum(t + f, np.finfo(np.float64).eps)
        out[c] = (rec, prec, voc_ap(rec, prec))
    return out


# ------------------------------------------------------------------------------------------------ get_boxes, the host loop
def box_corners_from_param(size, heading, center):
    """utils/box_utils.py:8-25 in fp32"""
    c, s = F32(np.cos(F32(heading))), F32(np.sin(F32(heading)))
    l, w, h = [F32(v) for v in size]
    x = np.array([-l / 2, l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2], dtype=F32)
    y = np.array([-w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2, w / 2], dtype=F32)
    z = np.array([-h / 2, -h / 2, -h / 2, -h / 2, h / 2, h / 2, h / 2, h / 2], dtype=F32)
    out = np.stack([c * x - s * y + F32(center[0]), s * x + c * y + F32(center[1]), z + F32(center[2])], 1)
    return out.astype(F32)


def _softmax(v):
    e = np.exp(v - v.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def get_boxes(res, mean_size_arr, class2angle=None, num_heading_bin=1, apply_nms=False, objectness_threshold=0.05,
              duplicate_boxes=False, has_class=True):
    """VoteNetResults.get_boxes as the reference walks it: one box at a time on the host.  `res` maps the field names to
    numpy arrays.  Returns per scene a list of (classname, corners (8, 3), score)."""
    hs, hr = res["heading_scores"], res["heading_residuals"]
    ss, sr = res["size_scores"], res["size_residuals"]
    B, P = hs.shape[:2]
    corners = np.zeros((B, P, 8, 3), dtype=F32)
    for i in range(B):
        for j in range(P):
            hc = int(np.argmax(hs[i, j]))
            sc = int(np.argmax(ss[i, j]))
            if class2angle is not None:
                angle = class2angle(hc, hr[i, j, hc])
            else:
                angle = F32(hc) * F32(2 * np.pi / num_heading_bin) + hr[i, j, hc]
            size = np.asarray(mean_size_arr, dtype=F32)[sc] + sr[i, j, sc]
            corners[i, j] = box_corners_from_param(size, angle, res["center"][i, j])
    obj = _softmax(res["objectness_scores"].astype(F32))[:, :, 1]
    sem = res["sem_cls_scores"]
    cls = np.argmax(sem, -1)
    proba = _softmax(sem.astype(F32))
    if apply_nms:
        boxes = np.concatenate([corners.min(2), corners.max(2)], -1)
        mask = nms_mask(boxes, cls, obj, 0.25)
    else:
        mask = np.ones((B, P), dtype=bool)
    out = []
    for i in range(B):
        scene = []
        for j in range(P):
            if not mask[i, j] or not obj[i, j] > objectness_threshold:
                continue
            if duplicate_boxes and has_class:
                for c in range(proba.shape[-1]):
                    scene.append((c, corners[i, j], float(obj[i, j] * proba[i, j, c])))
            else:
                scene.append((int(cls[i, j]), corners[i, j], float(obj[i, j])))
        out.append(scene)
    return out
