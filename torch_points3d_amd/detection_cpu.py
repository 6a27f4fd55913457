"""Host (numpy) form of the detection operators of csrc/detection.hip, for CPU tensors: the data-loader and offline
evaluation side, where no device is at hand.  Same definitions as the kernels (include/tp3d_hip.h, "Detection"): the fp32
overlap of nms_samecls with its explicit visiting order, the float64 Sutherland-Hodgman clip with the shoelace area,
the grouped greedy matching of eval_det_cls.  torch_points3d_amd.votenet dispatches here when its inputs are not on a
device; the HIP path never does."""
import numpy as np

_F32 = np.float32


def box_nms(boxes, scores, classes, overlap_threshold=0.25):
    """boxes (B, P, 6) fp32, scores (B, P), classes (B, P) -> keep (B, P) bool"""
    boxes = np.ascontiguousarray(boxes, dtype=_F32)
    scores = np.asarray(scores, dtype=_F32)
    classes = np.asarray(classes)
    B, P = boxes.shape[:2]
    keep = np.zeros((B, P), dtype=bool)
    thr = _F32(overlap_threshold)
    for b in range(B):
        bx = boxes[b]
        lo, hi = bx[:, :3], bx[:, 3:]
        ext = hi - lo
        area = ext[:, 0] * ext[:, 1] * ext[:, 2]
        order = np.argsort(scores[b], kind="stable")[::-1]
        alive = np.ones(P, dtype=bool)  # by slot of the order
        with np.errstate(invalid="ignore", divide="ignore"):
            for a in range(P):
                if not alive[a]:
                    continue
                i = order[a]
                rest = order[a + 1:]
                d = np.maximum(_F32(0), np.minimum(hi[i], hi[rest]) - np.maximum(lo[i], lo[rest]))
                inter = d[:, 0] * d[:, 1] * d[:, 2]
                o = inter / (area[i] + area[rest] - inter)
                o = o * (classes[b, i] == classes[b, rest]).astype(_F32)
                alive[a + 1:] &= ~(o > thr)
        keep[b, order[alive]] = True
    return keep


def _clip_area(r1, r2):
    """area of the counter-clockwise rectangle r1 (4 (x, y) pairs) inside the convex rectangle r2"""
    poly = [(float(x), float(y)) for x, y in r1]
    c1x, c1y = float(r2[3][0]), float(r2[3][1])
    for k in range(4):
        c2x, c2y = float(r2[k][0]), float(r2[k][1])
        ex, ey = c2x - c1x, c2y - c1y
        src, poly = poly, []
        sx, sy = src[-1]
        s_in = ex * (sy - c1y) > ey * (sx - c1x)
        for px, py in src:
            p_in = ex * (py - c1y) > ey * (px - c1x)
            if p_in != s_in:
                dcx, dcy = c1x - c2x, c1y - c2y
                dpx, dpy = sx - px, sy - py
                n1 = c1x * c2y - c1y * c2x
                n2 = sx * py - sy * px
                n3 = 1.0 / (dcx * dpy - dcy * dpx)
                poly.append(((n1 * dpx - n2 * dcx) * n3, (n1 * dpy - n2 * dcy) * n3))
            if p_in:
                poly.append((px, py))
            sx, sy, s_in = px, py, p_in
        c1x, c1y = c2x, c2y
        if not poly:
            return 0.0
    twice = 0.0
    for k in range(len(poly)):
        px, py = poly[k]
        qx, qy = poly[(k + 1) % len(poly)]
        twice = twice + (px * qy - qx * py)
    return 0.5 * abs(twice)


def _edge(c, i, j):
    d = c[i] - c[j]
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def _volume(c):
    return _edge(c, 0, 1) * _edge(c, 1, 2) * _edge(c, 0, 4)


def _iou(c1, c2, v1, v2):
    area = _clip_area(c1[:4, :2], c2[:4, :2])
    height = max(0.0, min(c1[4, 2], c2[4, 2]) - max(c1[0, 2], c2[0, 2]))
    inter = area * height
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(inter) / np.float64((v1 + v2) - inter))


def box3d_iou(corners1, corners2):
    """corners1 (n, 8, 3), corners2 (m, 8, 3) -> (n, m) float64"""
    c1 = np.asarray(corners1, dtype=_F32).astype(np.float64)
    c2 = np.asarray(corners2, dtype=_F32).astype(np.float64)
    v1 = [_volume(c) for c in c1]
    v2 = [_volume(c) for c in c2]
    out = np.zeros((len(c1), len(c2)), dtype=np.float64)
    for i in range(len(c1)):
        for j in range(len(c2)):
            out[i, j] = _iou(c1[i], c2[j], v1[i], v2[j])
    return out


def ap_match(det_corners, det_score, det_class, det_scene, gt_corners, gt_class, gt_scene_start, thresholds=(0.25, 0.5)):
    """(tp (D, T) bool, ovmax (D,) float64, jmax (D,) int64), as torchpoints.ap_match"""
    det = np.asarray(det_corners, dtype=_F32).astype(np.float64)
    gt = np.asarray(gt_corners, dtype=_F32).astype(np.float64)
    det_class, det_scene, gt_class = np.asarray(det_class), np.asarray(det_scene), np.asarray(gt_class)
    start = np.asarray(gt_scene_start)
    D, T = len(det), len(thresholds)
    vg = [_volume(c) for c in gt]
    ovmax = np.full(D, -np.inf)
    jmax = np.full(D, -1, dtype=np.int64)
    for d in range(D):
        s = int(det_scene[d])
        if s < 0 or s + 1 >= len(start):
            continue
        vd = _volume(det[d])
        for j in range(int(start[s]), int(start[s + 1])):
            if gt_class[j] == det_class[d]:
                iou = _iou(det[d], gt[j], vd, vg[j])
                if iou > ovmax[d]:
                    ovmax[d], jmax[d] = iou, j
    tp = np.zeros((D, T), dtype=bool)
    order = np.argsort(-np.asarray(det_score, dtype=np.float64), kind="stable")
    for t, thr in enumerate(thresholds):
        taken = np.zeros(max(len(gt), 1), dtype=bool)  # a box belongs to one (scene, class) group
        for d in order:
            j = jmax[d]
            if j >= 0 and ovmax[d] > thr and not taken[j]:
                taken[j] = True
                tp[d, t] = True
    return tp, ovmax, jmax
