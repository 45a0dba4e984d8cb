// Scoring a set of detections against a set of annotations (gfx950): calcIntersectAll / calcUnionAll, rpnToRegion.py:202-222.
//
// The reference unions each side with shapely's cascaded_union and takes the area of the intersection of the two unions.
// Here a workgroup owns a sample and the three areas -- (U P) n (U L), U P, U L -- come out of one boundary integral:
// the boundary of each region is made of pieces of rectangle edges, and area = 1/2 * sum over the pieces of x0*y1 - x1*y0.
//
// Per edge E = A -> B of rectangle i (one thread per edge), every other rectangle k of the sample cuts the LINE of E in an
// interval of the edge parameter t (clipping against its four half planes), so "which part of E bounds the region" is
// interval algebra on [0, 1], and a piece [t0, t1] contributes (t1 - t0) * (A x B).  A piece bounds a region G with the
// orientation of rectangle i iff a point just INSIDE rectangle i across the piece lies in G and a point just OUTSIDE does
// not.  The two points differ only where E runs along an edge of rectangle k: there the inside point belongs to k iff the
// two rectangles lie on the same side of the common line.  Among edges that coincide with the same orientation (a duplicate
// box, equal extents) all see the same two points, and the one of the lowest box index counts.
//
// Nothing is stored per edge: the sweep along t re-derives the intervals for each piece (pieces per edge: a handful), so
// any number of boxes per side works; the rectangles of a sample are cached in LDS up to kCached of them.
//
// Consistency matters more than accuracy here: if edge E decides that it leaves rectangle k at one point and the edge of k
// that it crosses decides it enters rectangle i at another, a stretch of boundary is counted twice or not at all and the
// error is that stretch times the distance to the origin.  So everything two edges have to agree on -- whether they run
// along one line, whether they are parallel, where their lines cross -- is computed ONCE per pair, by pair_relation(), with
// the edge of the lower box index first, and each of the two threads evaluates the same expression on the same operands.
// float64 throughout; latency-bound scalar code: no MFMA, LDS for the rectangle cache and the final fixed-order reduction.
#include "box_geom.h"
#include "reduce.h"

namespace lisec {
namespace {

constexpr int kThreads = 256;
constexpr int kCached = 128;                                   // rectangles of a sample kept in LDS (12 KB); the rest are rebuilt

struct Rect {
    Pt c[4];
    double o;                                                  // +1 counter-clockwise, -1 clockwise, 0: no footprint
    double cx, cy, r;                                          // circumcircle, for the far-apart test
};

__device__ Rect make_rect(const double* b) {
    Rect R;
    box_corners(b, R.c);
    const double a = signed_area(R.c, 4);
    R.o = (b[3] == 0.0 || b[4] == 0.0) ? 0.0 : a > 0 ? 1.0 : a < 0 ? -1.0 : 0.0;
    R.cx = b[0]; R.cy = b[1]; R.r = 0.5 * hypot(b[3], b[4]);
    return R;
}

__device__ __forceinline__ double cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// What two edges must agree on.  lo = the edge of the lower box index.
struct PairRel {
    int kind;                                                  // 0: the lines cross at X, 1: one line, 2: parallel apart
    double c;                                                  // d_lo x d_hi
    Pt X;
    double s_lo, s_hi;                                         // kind 2: d_hi x (A_lo - A_hi), d_lo x (A_hi - A_lo)
};

__device__ PairRel pair_relation(Pt Alo, Pt Blo, Pt Ahi, Pt Bhi) {
    PairRel p;
    const double lx = Blo.x - Alo.x, ly = Blo.y - Alo.y, hx = Bhi.x - Ahi.x, hy = Bhi.y - Ahi.y;
    p.c = cross(lx, ly, hx, hy);
    const double s1 = cross(lx, ly, Ahi.x - Alo.x, Ahi.y - Alo.y), s2 = cross(lx, ly, Bhi.x - Alo.x, Bhi.y - Alo.y);
    const double s3 = cross(hx, hy, Alo.x - Ahi.x, Alo.y - Ahi.y), s4 = cross(hx, hy, Blo.x - Ahi.x, Blo.y - Ahi.y);
    p.s_lo = s3; p.s_hi = s1;
    // one line: all four end points within eta of the other edge's line.  eta = 1e-12 of the coordinate magnitude, a few
    // thousand ulps: yaw = pi/2 is not exactly a quarter turn in float64, and such edges must still count as running along
    // each other.  Treating them so moves the boundary by at most eta.
    const double mag = 1.0 + fmax(fmax(fabs(Alo.x) + fabs(Alo.y), fabs(Blo.x) + fabs(Blo.y)),
                                  fmax(fabs(Ahi.x) + fabs(Ahi.y), fabs(Bhi.x) + fabs(Bhi.y)));
    const double el = 1e-12 * mag * hypot(lx, ly), eh = 1e-12 * mag * hypot(hx, hy);
    if (fabs(s1) <= el && fabs(s2) <= el && fabs(s3) <= eh && fabs(s4) <= eh) { p.kind = 1; return p; }
    if (p.c == 0.0) { p.kind = 2; return p; }
    p.kind = 0;
    const double t = s3 / p.c;                                 // A_lo + t d_lo = A_hi + u d_hi
    p.X = {Alo.x + t * lx, Alo.y + t * ly};
    return p;
}

// The parts of E's parameter line over which a point just inside (in) / just outside (out) rectangle i lies in rectangle K.
struct Span {
    double lo_in, hi_in, lo_out, hi_out;
    bool twin;                                                 // K has an edge along E with K on the same side as rectangle i
};

__device__ Span rect_span(Pt A, Pt B, double oi, bool e_is_lo, const Rect& K) {
    Span S = {-INFINITY, INFINITY, -INFINITY, INFINITY, false};
    const double dx = B.x - A.x, dy = B.y - A.y, dd = dx * dx + dy * dy;
    for (int j = 0; j < 4; ++j) {
        const Pt C = K.c[j], D = K.c[(j + 1) & 3];
        const PairRel p = e_is_lo ? pair_relation(A, B, C, D) : pair_relation(C, D, A, B);
        if (p.kind == 1) {
            const bool same = oi * K.o * (dx * (D.x - C.x) + dy * (D.y - C.y)) > 0;
            if (same) { S.lo_out = INFINITY; S.twin = true; }
            else S.lo_in = INFINITY;
        } else if (p.kind == 2) {
            const double n0 = K.o * (e_is_lo ? p.s_lo : p.s_hi);          // K.o * (C->D) x (A - C)
            if (!(n0 > 0)) { S.lo_in = INFINITY; S.lo_out = INFINITY; }
        } else {
            const double n1 = K.o * (e_is_lo ? -p.c : p.c);               // K.o * (C->D) x (A->B)
            const double ts = ((p.X.x - A.x) * dx + (p.X.y - A.y) * dy) / dd;
            if (n1 > 0) { S.lo_in = fmax(S.lo_in, ts); S.lo_out = fmax(S.lo_out, ts); }
            else { S.hi_in = fmin(S.hi_in, ts); S.hi_out = fmin(S.hi_out, ts); }
        }
    }
    return S;
}

// sum over the workgroup in a fixed order (the tree of reduce.h), result in every thread
__device__ double block_sum(double v, double (&red)[1][kThreads]) {
    const double a[1] = {v};
    __syncthreads();                                           // red is free of the call before
    tree_sums<kThreads>(a, red);
    return red[0][0];
}

__global__ void __launch_bounds__(kThreads)
k_union_overlap(const double* __restrict__ pred, const int32_t* __restrict__ pred_start, const double* __restrict__ label,
                const int32_t* __restrict__ label_start, double* __restrict__ out) {
    __shared__ Rect cache[kCached];
    __shared__ double red[1][kThreads];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int p0 = pred_start[s], l0 = label_start[s];
    const int nP = max(pred_start[s + 1] - p0, 0), nL = max(label_start[s + 1] - l0, 0), n = nP + nL;
    auto box = [&](int k) { return k < nP ? pred + (size_t)(p0 + k) * 7 : label + (size_t)(l0 + k - nP) * 7; };
    auto rect = [&](int k) { return k < kCached ? cache[k] : make_rect(box(k)); };

    double volP = 0.0, volL = 0.0;
    for (int k = tid; k < n; k += kThreads) {
        const double* b = box(k);
        if (k < kCached) cache[k] = make_rect(b);
        (k < nP ? volP : volL) += b[3] * b[4] * b[5];
    }
    __syncthreads();

    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (int e = tid; e < 4 * n; e += kThreads) {
        const int i = e >> 2, side = e & 3;
        const Rect R = rect(i);
        if (R.o == 0.0) continue;
        const Pt A = R.c[side], B = R.c[(side + 1) & 3];
        const bool selfP = i < nP;
        const double mx = 0.5 * (A.x + B.x), my = 0.5 * (A.y + B.y), half = 0.5 * hypot(B.x - A.x, B.y - A.y);
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, t = 0.0;
        while (t < 1.0) {
            double tn = 1.0;
            bool p_in = selfP, p_out = false, l_in = !selfP, l_out = false, twinP = false, twinL = false;
            for (int k = 0; k < n; ++k) {
                if (k == i) continue;
                const Rect K = rect(k);
                if (K.o == 0.0) continue;
                const double reach = (K.r + half) * 1.000001 + 1e-9;         // circles apart: K cannot reach E
                if ((K.cx - mx) * (K.cx - mx) + (K.cy - my) * (K.cy - my) > reach * reach) continue;
                const Span S = rect_span(A, B, R.o, i < k, K);
                if (S.lo_in > t && S.lo_in < tn) tn = S.lo_in;
                if (S.hi_in > t && S.hi_in < tn) tn = S.hi_in;
                if (S.lo_out > t && S.lo_out < tn) tn = S.lo_out;
                if (S.hi_out > t && S.hi_out < tn) tn = S.hi_out;
                const bool ci = S.lo_in <= t && t < S.hi_in, co = S.lo_out <= t && t < S.hi_out;
                const bool twin = ci && S.twin && k < i;                    // the lowest index of coinciding edges counts
                if (k < nP) { p_in |= ci; p_out |= co; twinP |= twin; }
                else { l_in |= ci; l_out |= co; twinL |= twin; }
            }
            const double len = tn - t;
            if (p_in && l_in && !(p_out && l_out) && !twinP && !twinL) m0 += len;
            if (selfP && !p_out && !twinP) m1 += len;
            if (!selfP && !l_out && !twinL) m2 += len;
            t = tn;
        }
        const double w = 0.5 * R.o * cross(A.x, A.y, B.x, B.y);
        acc0 += w * m0; acc1 += w * m1; acc2 += w * m2;
    }
    const double r0 = block_sum(acc0, red), r1 = block_sum(acc1, red), r2 = block_sum(acc2, red);
    const double r3 = block_sum(volP, red), r4 = block_sum(volL, red);
    if (tid == 0) {
        double* o = out + (size_t)s * 5;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
    }
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_boxes_union_overlap_workspace_bytes(int n_samples, int max_pred, int max_label) {
    (void)n_samples; (void)max_pred; (void)max_label;
    return 0;                                                  // the sweep keeps nothing per edge
}

extern "C" int lisec_boxes_union_overlap(const double* pred_boxes, const int32_t* pred_start, const double* label_boxes,
                                         const int32_t* label_start, int n_samples, void* workspace, size_t workspace_bytes,
                                         double* out, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(pred_boxes && pred_start && label_boxes && label_start && out && n_samples >= 0, "bad arguments");
    LISEC_CHECK_ARG(workspace_bytes >= lisec_boxes_union_overlap_workspace_bytes(n_samples, 0, 0), "workspace too small");
    (void)workspace;
    if (n_samples == 0) return LISEC_OK;
    LISEC_LAUNCH(k_union_overlap, dim3(n_samples), dim3(kThreads), 0, static_cast<hipStream_t>(stream_), pred_boxes,
                 pred_start, label_boxes, label_start, out);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
