// The rectangle footprint shared by the box kernels (boxes.hip, union_overlap.hip, detection_ap.hip, detection_eval.hip,
// detection_metrics.hip, detection_iou_loss.hip): boxToShapely's vertices, the shoelace sum, the clipped area of two
// footprints, their IoU, and the anchor decode of the detection metrics and the IoU loss.
#pragma once
#include "common.h"

namespace lisec {

struct Pt { double x, y; };

__device__ __forceinline__ void box_corners(const double* b, Pt* c) {
    // boxToShapely (serialize_data.py:149-162): [topRight, botRight, botLeft, topLeft]
    const double th = b[6], l = b[3], w = b[4];
    const double cs = cos(th), sn = sin(th);
    const double rx = b[0] + cs * (w / 2), ry = b[1] - sn * (w / 2);
    const double lx = b[0] - cs * (w / 2), ly = b[1] + sn * (w / 2);
    const double sx = sn * (l / 2), sy = cs * (l / 2);
    c[0] = {rx + sx, ry + sy}; c[1] = {rx - sx, ry - sy}; c[2] = {lx - sx, ly - sy}; c[3] = {lx + sx, ly + sy};
}

__device__ __forceinline__ double signed_area(const Pt* p, int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) {
        const Pt& u = p[i];
        const Pt& v = p[i + 1 == n ? 0 : i + 1];
        a += u.x * v.y - v.x * u.y;
    }
    return 0.5 * a;
}

// area of the intersection of two convex quadrilaterals (Sutherland-Hodgman + shoelace)
__device__ inline double quad_intersection_area(const Pt* pa, const Pt* qa) {
    Pt p[4], q[4];
    const bool pf = signed_area(pa, 4) < 0, qf = signed_area(qa, 4) < 0;
    for (int i = 0; i < 4; ++i) { p[i] = pa[pf ? 3 - i : i]; q[i] = qa[qf ? 3 - i : i]; }
    Pt bufA[10], bufB[10];
    Pt* in = bufA;
    Pt* out = bufB;
    int n = 4;
    for (int i = 0; i < 4; ++i) out[i] = p[i];
    for (int e = 0; e < 4 && n > 0; ++e) {
        Pt* t = in; in = out; out = t;
        const int nin = n;
        n = 0;
        const Pt a = q[e], b = q[(e + 1) & 3];
        const double ex = b.x - a.x, ey = b.y - a.y;
        for (int j = 0; j < nin; ++j) {
            const Pt c = in[j], d = in[j + 1 == nin ? 0 : j + 1];
            const double sc = ex * (c.y - a.y) - ey * (c.x - a.x);
            const double sd = ex * (d.y - a.y) - ey * (d.x - a.x);
            if (sc >= 0) out[n++] = c;
            if ((sc >= 0) != (sd >= 0)) {
                const double t = sc / (sc - sd);
                out[n++] = {c.x + t * (d.x - c.x), c.y + t * (d.y - c.y)};
            }
        }
    }
    if (n < 3) return 0.0;
    return fabs(signed_area(out, n));
}

// IoU of two boxes (x, y, z, l, w, h, yaw) under LISEC_IOU_3D / LISEC_IOU_BEV (include/lisec_hip.h, lisec_boxes_match): the
// clipped footprints, times the clamped height overlap in 3D; 0 for a zero extent.  Shared by detection_ap.hip and
// detection_metrics.hip.
__device__ inline double pair_iou(const double* p, const double* g, int mode) {
    if (p[3] == 0.0 || p[4] == 0.0 || g[3] == 0.0 || g[4] == 0.0) return 0.0;
    if (mode == LISEC_IOU_3D && (p[5] == 0.0 || g[5] == 0.0)) return 0.0;
    // footprints further apart than the sum of their circumradii do not meet: area 0, IoU exactly 0
    const double dx = p[0] - g[0], dy = p[1] - g[1];
    const double r = 0.5 * (hypot(p[3], p[4]) + hypot(g[3], g[4]));
    if (dx * dx + dy * dy > r * r * 1.0000001) return 0.0;
    Pt cp[4], cg[4];
    box_corners(p, cp);
    box_corners(g, cg);
    double inter = quad_intersection_area(cp, cg);             // flips a mirrored (negative extent) footprint itself
    double sp = fabs(p[3] * p[4]), sg = fabs(g[3] * g[4]);
    if (mode == LISEC_IOU_3D) {
        const double hp = 0.5 * fabs(p[5]), hg = 0.5 * fabs(g[5]);
        inter *= fmax(0.0, fmin(p[2] + hp, g[2] + hg) - fmax(p[2] - hp, g[2] - hg));
        sp = fabs(p[3] * p[4] * p[5]);
        sg = fabs(g[3] * g[4] * g[5]);
    }
    const double uni = sp + sg - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// Candidate i = a * M + m of the anchor grid (anchor a, cell m = ix * outY + iy) decoded to its box b[7]: the anchor at the
// cell centre with applyRegrssion on top (rpnToRegion.py:75-150).  k_rpn_decode (boxes.hip) and the detection output
// (detect.hip) share it.
__device__ __forceinline__ void rpn_decode_box(const lisec_rpn_cfg& cfg, const float* __restrict__ reg, int reg_stride, int i,
                                               double* __restrict__ b) {
    const int M = cfg.outX * cfg.outY;
    const int a = i / M, m = i - a * M;
    const int ix = m / cfg.outY, iy = m - ix * cfg.outY;
    const double* an = cfg.anchors[a];
    const float* t = reg + (size_t)m * reg_stride + a * 7;
    const double x = ix * cfg.vx + cfg.vx / 2, y = iy * cfg.vy + cfg.vy / 2;
    b[0] = (double)t[0] * an[0] + x;
    b[1] = (double)t[1] * an[1] + y;
    b[2] = (double)t[2] * an[2] + 1.0;
    b[3] = exp((double)t[3]) * an[0];
    b[4] = exp((double)t[4]) * an[1];
    b[5] = exp((double)t[5]) * an[2];
    b[6] = (double)t[6] + an[3];
}

__device__ __forceinline__ bool finite7(const double* b) {
    return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && isfinite(b[4]) && isfinite(b[5]) &&
           isfinite(b[6]);
}

// The decode of k_rpn_decode (csrc/boxes.hip) for the prediction r and target t of one anchor an = (l, w, h, yaw), without
// the anchor centre both boxes share; false when either box is not finite.
__device__ __forceinline__ bool decode_pair(const double* r, const double* t, const double* an, double* p, double* g) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = r[k] * an[k];
        g[k] = t[k] * an[k];
        p[3 + k] = exp(r[3 + k]) * an[k];
        g[3 + k] = exp(t[3 + k]) * an[k];
    }
    p[6] = r[6] + an[3];
    g[6] = t[6] + an[3];
    return finite7(p) && finite7(g);
}

// IoU of the decoded prediction and target of one anchor; 0 for anything that is not finite (a yaw that is not finite has
// no footprint, hence no finite IoU)
__device__ inline double decoded_iou(const double* r, const double* t, const double* an, int mode) {
    double p[7], g[7];
    if (!decode_pair(r, t, an, p, g)) return 0.0;
    const double iou = pair_iou(p, g, mode);
    return isfinite(iou) ? iou : 0.0;
}

}  // namespace lisec
