// The rectangle footprint shared by the box kernels (boxes.hip, union_overlap.hip): boxToShapely's vertices and the shoelace sum.
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

}  // namespace lisec
