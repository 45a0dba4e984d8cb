// The rectangle footprint shared by the box kernels (boxes.hip, union_overlap.hip, detection_ap.hip): boxToShapely's vertices,
// the shoelace sum and the clipped area of two footprints.
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

}  // namespace lisec
