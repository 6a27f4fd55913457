// Object-detection post-processing of VoteNet (include/tp3d_hip.h, "Detection"):
//   tp3d_box_nms_f32      nms_samecls of every scene in one launch       [utils/box_utils.py:28-85]
//   tp3d_box3d_iou_f64    box3d_iou of every (box, box) pair              [utils/box_utils.py:88-182]
//   tp3d_box_best_gt_f64  the best ground-truth box of every detection    [metrics/box_detection/ap.py:85-97]
//   tp3d_ap_match         the greedy true-positive assignment per group   [metrics/box_detection/ap.py:100-107]
// Plain loads and stores, LDS flags, no atomics: every output is a function of the inputs alone.  The translation unit
// is built with -ffp-contract=off; the fp32 overlap of the NMS and the float64 clip are evaluated in the reference's
// order of operations, one rounding per operation.
#include "tp3d_common.h"

namespace tp3d {
namespace {

constexpr int kNmsThreads = 256;
constexpr int kPairThreads = 256;

// The library is built with -fno-honor-nans, so a NaN is recognised by its bits, never by a comparison.
__device__ __forceinline__ bool is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool is_nan_bits(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// ------------------------------------------------------------------------------------------------ NMS
// One workgroup per scene.  The scene's boxes are staged in LDS in visiting order (slot s = box order[s]); the sweep
// walks the slots, and every live slot suppresses the later live slots of its class in parallel.  A dead slot costs
// one LDS read and no barrier.  LDS per slot: 6 + 1 floats, the class (int64) and one flag byte.
__global__ void __launch_bounds__(kNmsThreads)
box_nms_kernel(const float *__restrict__ boxes, const int64_t *__restrict__ classes, const int64_t *__restrict__ order, int P,
               float thr, uint8_t *__restrict__ keep)
{
    extern __shared__ __align__(16) unsigned char nms_lds[];
    int64_t *cls = reinterpret_cast<int64_t *>(nms_lds);  // P
    float *bx = reinterpret_cast<float *>(cls + P);       // 6 * P, component-major
    float *area = bx + 6 * (size_t)P;                     // P
    uint8_t *alive = reinterpret_cast<uint8_t *>(area + P);

    const int64_t base = (int64_t)blockIdx.x * P;
    for (int s = threadIdx.x; s < P; s += kNmsThreads) {
        int64_t src = order[base + s];
        const bool ok = src >= 0 && src < P;  // a slot with an index outside the scene never suppresses and is not kept
        if (!ok) src = 0;
        const float *b = boxes + (base + src) * 6;
        const float x1 = b[0], y1 = b[1], z1 = b[2], x2 = b[3], y2 = b[4], z2 = b[5];
        bx[s] = x1;
        bx[P + s] = y1;
        bx[2 * P + s] = z1;
        bx[3 * P + s] = x2;
        bx[4 * P + s] = y2;
        bx[5 * P + s] = z2;
        area[s] = ((x2 - x1) * (y2 - y1)) * (z2 - z1);
        cls[s] = classes[base + src];
        alive[s] = ok ? 1 : 0;
    }
    __syncthreads();

    for (int i = 0; i + 1 < P; ++i) {
        if (!alive[i]) continue;  // the same LDS byte for every thread, last written before the previous barrier
        const float ix1 = bx[i], iy1 = bx[P + i], iz1 = bx[2 * P + i];
        const float ix2 = bx[3 * P + i], iy2 = bx[4 * P + i], iz2 = bx[5 * P + i];
        const float ia = area[i];
        const int64_t ic = cls[i];
        for (int j = i + 1 + threadIdx.x; j < P; j += kNmsThreads) {
            if (!alive[j]) continue;
            const float xx1 = fmaxf(ix1, bx[j]);
            const float yy1 = fmaxf(iy1, bx[P + j]);
            const float zz1 = fmaxf(iz1, bx[2 * P + j]);
            const float xx2 = fminf(ix2, bx[3 * P + j]);
            const float yy2 = fminf(iy2, bx[4 * P + j]);
            const float zz2 = fminf(iz2, bx[5 * P + j]);
            const float l = fmaxf(0.0f, xx2 - xx1);
            const float w = fmaxf(0.0f, yy2 - yy1);
            const float h = fmaxf(0.0f, zz2 - zz1);
            const float inter = (l * w) * h;
            float o = inter / ((ia + area[j]) - inter);
            o = o * (cls[j] == ic ? 1.0f : 0.0f);
            if (!is_nan_bits(o) && o > thr) alive[j] = 0;  // 0 / 0 (two boxes without volume) compares false
        }
        __syncthreads();
    }
    __syncthreads();
    for (int s = threadIdx.x; s < P; s += kNmsThreads) {
        const int64_t src = order[base + s];
        if (src >= 0 && src < P) keep[base + src] = alive[s];
    }
}

size_t nms_lds_bytes(int P) { return align_up((size_t)P * (8 + 7 * 4 + 1), 16); }

// ------------------------------------------------------------------------------------------------ rotated IoU
struct P2 {
    double x, y;
};

// Area of rectangle `subj` clipped by the convex rectangle `clip` (both counter-clockwise): polygon_clip's
// Sutherland-Hodgman with its strict inside test and its computeIntersection, then the shoelace sum in vertex order.
__device__ double clipped_area(const P2 *subj, const P2 *clip)
{
    P2 a[8], b[8];
    P2 *in = a, *out = b;
    int n = 4;
    for (int k = 0; k < 4; ++k) out[k] = subj[k];
    P2 cp1 = clip[3];
    for (int c = 0; c < 4; ++c) {
        const P2 cp2 = clip[c];
        P2 *t = in;
        in = out;
        out = t;
        const int nin = n;
        n = 0;
        P2 s = in[nin - 1];
        const double ex = cp2.x - cp1.x, ey = cp2.y - cp1.y;
        bool s_in = ex * (s.y - cp1.y) > ey * (s.x - cp1.x);
        for (int k = 0; k < nin; ++k) {
            const P2 e = in[k];
            const bool e_in = ex * (e.y - cp1.y) > ey * (e.x - cp1.x);
            if (e_in != s_in) {
                const double dcx = cp1.x - cp2.x, dcy = cp1.y - cp2.y;
                const double dpx = s.x - e.x, dpy = s.y - e.y;
                const double n1 = cp1.x * cp2.y - cp1.y * cp2.x;
                const double n2 = s.x * e.y - s.y * e.x;
                const double n3 = 1.0 / (dcx * dpy - dcy * dpx);
                if (n < 8) {
                    out[n].x = (n1 * dpx - n2 * dcx) * n3;
                    out[n].y = (n1 * dpy - n2 * dcy) * n3;
                    ++n;
                }
            }
            if (e_in && n < 8) out[n++] = e;
            s = e;
            s_in = e_in;
        }
        cp1 = cp2;
        if (n == 0) return 0.0;
    }
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const P2 p = out[k], q = out[k + 1 < n ? k + 1 : 0];
        sum = sum + (p.x * q.y - q.x * p.y);
    }
    return 0.5 * fabs(sum);
}

__device__ __forceinline__ double edge_len(const float *c, int i, int j)
{
    const double dx = (double)c[3 * i] - (double)c[3 * j];
    const double dy = (double)c[3 * i + 1] - (double)c[3 * j + 1];
    const double dz = (double)c[3 * i + 2] - (double)c[3 * j + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// box3d_vol: the product of three edge lengths
__device__ __forceinline__ double box_volume(const float *c) { return (edge_len(c, 0, 1) * edge_len(c, 1, 2)) * edge_len(c, 0, 4); }

// box3d_iou on two (8, 3) fp32 corner sets, float64 arithmetic on the promoted values
__device__ double box_iou(const float *c1, const float *c2)
{
    P2 r1[4], r2[4];
    for (int k = 0; k < 4; ++k) {
        r1[k].x = (double)c1[3 * k];
        r1[k].y = (double)c1[3 * k + 1];
        r2[k].x = (double)c2[3 * k];
        r2[k].y = (double)c2[3 * k + 1];
    }
    const double inter_area = clipped_area(r1, r2);
    const double zmin = fmax((double)c1[2], (double)c2[2]);
    const double zmax = fmin((double)c1[14], (double)c2[14]);
    const double inter_vol = inter_area * fmax(0.0, zmax - zmin);
    const double v1 = box_volume(c1), v2 = box_volume(c2);
    return inter_vol / ((v1 + v2) - inter_vol);
}

__global__ void __launch_bounds__(kPairThreads)
box3d_iou_kernel(const float *__restrict__ c1, const float *__restrict__ c2, int64_t n, int64_t m, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (e >= n * m) return;
    out[e] = box_iou(c1 + (e / m) * 24, c2 + (e % m) * 24);
}

// ------------------------------------------------------------------------------------------------ AP matching
// One thread per detection: the first maximum of the IoU over the ground-truth boxes of its scene and class.
__global__ void __launch_bounds__(kPairThreads)
box_best_gt_kernel(const float *__restrict__ det, const int64_t *__restrict__ det_cls, const int64_t *__restrict__ det_scene,
                   int64_t D, const float *__restrict__ gt, const int64_t *__restrict__ gt_cls,
                   const int64_t *__restrict__ gt_start, int64_t G, int64_t S, double *__restrict__ ovmax,
                   int64_t *__restrict__ jmax)
{
    const int64_t d = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (d >= D) return;
    double best = -HUGE_VAL;
    int64_t at = -1;
    const int64_t sc = det_scene[d];
    if (sc >= 0 && sc < S) {
        int64_t lo = gt_start[sc], hi = gt_start[sc + 1];
        if (lo < 0) lo = 0;
        if (hi > G) hi = G;
        const int64_t c = det_cls[d];
        for (int64_t j = lo; j < hi; ++j) {
            if (gt_cls[j] != c) continue;
            const double iou = box_iou(det + d * 24, gt + j * 24);
            if (!is_nan_bits(iou) && iou > best) {
                best = iou;
                at = j;
            }
        }
    }
    ovmax[d] = best;
    jmax[d] = at;
}

// Position p of the visiting order leads a group when its (scene, class) differs from position p - 1.  The leader walks
// its group in order; a ground-truth box belongs to one group only, so its `taken` flags have a single writer.
__global__ void __launch_bounds__(kPairThreads)
ap_match_kernel(const int64_t *__restrict__ order, const int64_t *__restrict__ det_cls, const int64_t *__restrict__ det_scene,
                int64_t D, const double *__restrict__ ovmax, const int64_t *__restrict__ jmax, int64_t G,
                const double *__restrict__ thr, int T, uint8_t *__restrict__ taken, uint8_t *__restrict__ tp)
{
    const int64_t p = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (p >= D) return;
    const int64_t d0 = order[p];
    if (d0 < 0 || d0 >= D) return;
    const int64_t c = det_cls[d0], sc = det_scene[d0];
    if (p > 0) {
        const int64_t dp = order[p - 1];
        if (dp >= 0 && dp < D && det_cls[dp] == c && det_scene[dp] == sc) return;
    }
    for (int64_t q = p; q < D; ++q) {
        const int64_t d = order[q];
        if (d < 0 || d >= D || det_cls[d] != c || det_scene[d] != sc) break;
        const double ov = ovmax[d];
        const int64_t j = jmax[d];
        for (int t = 0; t < T; ++t) {
            uint8_t hit = 0;
            if (j >= 0 && j < G && ov > thr[t] && !taken[(int64_t)t * G + j]) {
                taken[(int64_t)t * G + j] = 1;
                hit = 1;
            }
            tp[d * T + t] = hit;
        }
    }
}

}  // namespace
}  // namespace tp3d

using namespace tp3d;

TP3D_EXPORT int tp3d_box_nms_max_boxes(void) { return TP3D_BOX_NMS_MAX_BOXES; }

TP3D_EXPORT int tp3d_box_nms_f32(const float *boxes, const int64_t *classes, const int64_t *order, int B, int P,
                                 float overlap_threshold, uint8_t *keep, void *stream)
{
    if (B < 0 || P < 0) return TP3D_E_BADARG;
    if (P > TP3D_BOX_NMS_MAX_BOXES) return TP3D_E_TOOBIG;
    if (B == 0 || P == 0) return TP3D_OK;
    if (!boxes || !classes || !order || !keep) return TP3D_E_BADARG;
    const size_t lds = nms_lds_bytes(P);
    if (lds > 64 * 1024) allow_large_dynamic_lds<&box_nms_kernel>((int)nms_lds_bytes(TP3D_BOX_NMS_MAX_BOXES));
    hipLaunchKernelGGL(box_nms_kernel, dim3(B), dim3(kNmsThreads), lds, (hipStream_t)stream, boxes, classes, order, P,
                       overlap_threshold, keep);
    return check_launch();
}

TP3D_EXPORT int tp3d_box3d_iou_f64(const float *corners1, const float *corners2, int64_t n, int64_t m, double *iou,
                                   void *stream)
{
    if (n < 0 || m < 0) return TP3D_E_BADARG;
    if (n == 0 || m == 0) return TP3D_OK;
    if (!corners1 || !corners2 || !iou) return TP3D_E_BADARG;
    if (n > ((int64_t)1 << 40) / m) return TP3D_E_TOOBIG;
    const int64_t blocks = (n * m + kPairThreads - 1) / kPairThreads;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(box3d_iou_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, (hipStream_t)stream, corners1,
                       corners2, n, m, iou);
    return check_launch();
}

TP3D_EXPORT int tp3d_box_best_gt_f64(const float *det_corners, const int64_t *det_class, const int64_t *det_scene, int64_t D,
                                     const float *gt_corners, const int64_t *gt_class, const int64_t *gt_scene_start,
                                     int64_t G, int64_t S, double *ovmax, int64_t *jmax, void *stream)
{
    if (D < 0 || G < 0 || S < 0) return TP3D_E_BADARG;
    if (D == 0) return TP3D_OK;
    if (!det_corners || !det_class || !det_scene || !ovmax || !jmax) return TP3D_E_BADARG;
    if (G > 0 && (!gt_corners || !gt_class)) return TP3D_E_BADARG;
    if (S > 0 && !gt_scene_start) return TP3D_E_BADARG;
    const int64_t blocks = (D + kPairThreads - 1) / kPairThreads;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    hipLaunchKernelGGL(box_best_gt_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, (hipStream_t)stream, det_corners,
                       det_class, det_scene, D, gt_corners, gt_class, gt_scene_start, G, S, ovmax, jmax);
    return check_launch();
}

TP3D_EXPORT int tp3d_ap_match(const int64_t *order, const int64_t *det_class, const int64_t *det_scene, int64_t D,
                              const double *ovmax, const int64_t *jmax, int64_t G, const double *thresholds, int T,
                              uint8_t *taken, uint8_t *tp, void *stream)
{
    if (D < 0 || G < 0 || T < 0) return TP3D_E_BADARG;
    if (D == 0 || T == 0) return TP3D_OK;
    if (!order || !det_class || !det_scene || !ovmax || !jmax || !thresholds || !tp) return TP3D_E_BADARG;
    if (G > 0 && !taken) return TP3D_E_BADARG;
    const int64_t blocks = (D + kPairThreads - 1) / kPairThreads;
    if (blocks > 0x7fffffff) return TP3D_E_TOOBIG;
    int rc = zero_async(taken, (size_t)T * (size_t)G, (hipStream_t)stream);
    if (rc != TP3D_OK) return rc;
    hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, (hipStream_t)stream, order, det_class,
                       det_scene, D, ovmax, jmax, G, thresholds, T, taken, tp);
    return check_launch();
}
