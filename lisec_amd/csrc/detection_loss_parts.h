// The launches of the VoxelNet detection loss, shared by detection_loss.hip (lisec_detection_loss*) and
// detection_iou_loss.hip (lisec_detection_iou_loss*, which adds a pass over the positive anchors):
//   k_det_count     one workgroup over y_cls (M*2 floats): N_pos and N_neg, exact integers, before any gradient is scaled
//   k_det_loss      the element layout of k_head_loss (csrc/losses.hip): thread i holds element i of the flat head; every
//                   element in double from the fp32 inputs, the gradient rounded once; per-workgroup fp64 partials of
//                   {sum_pos class, sum_neg class, sum_pos regression}, not yet normalised
//   k_det_finalize  one workgroup: the partials summed, normalised by the counts
// The count and the partials are order W of reduce.h, the finalize is order T: no atomics and a fixed partition.  Every
// address is fixed and nothing is read back: the launches record into a step plan as they are.
#pragma once
#include "reduce.h"
#include "sample_weights.h"

namespace lisec {
namespace {

constexpr int kDetThreads = 256;             // 16 cells of 16 lanes
constexpr int kDetBlocks = 1024;             // lisec_head_loss's partition
constexpr int kDetVals = 3;                  // partials per workgroup: S_pos (class), S_neg (class), S_reg
constexpr int kCountThreads = 1024;
constexpr int kCountUnroll = 16;

__device__ __forceinline__ bool is_pos(float code) { return code > 1.5f; }
__device__ __forceinline__ bool is_neg(float code) { return code > 0.5f && code <= 1.5f; }

// counts[0] = N_pos, counts[1] = N_neg over the 2M codes; a NaN code compares false twice: ignored
__global__ void __launch_bounds__(kCountThreads)
k_det_count(const float* __restrict__ ycls, long long n, long long* __restrict__ counts, long long* __restrict__ counts_out) {
    __shared__ long long red[2][kCountThreads / 64];
    long long np = 0, nn = 0;
    // one workgroup is latency-bound: kCountUnroll independent loads in flight per lane, so the Lyft map (40 000 codes)
    // is 3 round trips to memory, not 40
    for (long long base = 0; base < n; base += (long long)kCountThreads * kCountUnroll) {
        float c[kCountUnroll];
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u) {
            const long long i = base + (long long)u * kCountThreads + threadIdx.x;
            c[u] = i < n ? ycls[i] : 0.f;                    // 0: ignored
        }
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u) {
            np += is_pos(c[u]) ? 1 : 0;
            nn += is_neg(c[u]) ? 1 : 0;
        }
    }
    const long long v[2] = {np, nn};
    const long long a = block_sum_own<kCountThreads>(v, red);
    if (threadIdx.x < 2) {
        counts[threadIdx.x] = a;
        if (counts_out) counts_out[threadIdx.x] = a;
    }
}

// sp(x) = max(x,0) + log1p(exp(-|x|)) with e = exp(-|x|) given; the maximum is a comparison, so a NaN stays a NaN (in e)
__device__ __forceinline__ double softplus_e(double x, double e) { return (x > 0.0 ? x : 0.0) + log1p(e); }

// S(d) of the regression term and its derivative; b = smooth_l1_beta
__device__ __forceinline__ double smooth_l1(double d, double b) {
    const double ad = fabs(d);
    return ad < b ? d * d / (2.0 * b) : ad - 0.5 * b;
}
__device__ __forceinline__ double smooth_l1_grad(double d, double b) {
    return fabs(d) < b ? d / b : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d));
}

// dhead == nullptr: values only (the evaluation entry)
// WEIGHTED (one CellWeights behind parts; sample_weights.h): cell m carries the factor w_cls[m] on its two class channels and w_reg[m] on its fourteen
// regression channels: the gradient scale is (wpos * (double)w), (wneg * (double)w) or (wreg * (double)w) times the
// derivative, in that order, and the sums add (double)w * v.  The counts stay unweighted.  w == 1.0f gives the bits of the
// unweighted instantiation, which this template leaves as it was.
template <bool WEIGHTED, typename... W>
__global__ void __launch_bounds__(kDetThreads)
k_det_loss(lisec_detection_loss_cfg cfg, const float* __restrict__ head, const float* __restrict__ ycls,
           const float* __restrict__ yreg, long long M, float gscale, const long long* __restrict__ counts,
           float* __restrict__ dhead, double* __restrict__ parts, W... cw_) {
    [[maybe_unused]] const CellWeights cw = the_weights(cw_...);
    __shared__ double red[kDetVals][kDetThreads / 64];
    const int c = threadIdx.x & 15;
    const bool grad = dhead != nullptr;
    const long long cp = counts[0], cn = counts[1];
    const double npos = cp > 0 ? (double)cp : 1.0, nneg = cn > 0 ? (double)cn : 1.0;
    const double gs = (double)gscale;
    const double wpos = gs * cfg.weight[0] * cfg.alpha / npos, wneg = gs * cfg.weight[0] * cfg.beta / nneg;
    const double wreg = gs * cfg.weight[1] / npos;
    const double g = cfg.gamma, b = cfg.smooth_l1_beta;
    double spos = 0.0, sneg = 0.0, sreg = 0.0;
    [[maybe_unused]] SweepWeights sws = {};
    if constexpr (WEIGHTED) sws = sweep_weights(cw);
    const long long n = M * 16;
    for (long long base = blockIdx.x * (long long)kDetThreads; base < n; base += (long long)gridDim.x * kDetThreads) {
        const long long i = base + threadIdx.x;
        if (i >= n) break;
        const long long m = i >> 4;
        float gout = 0.f;                                    // +0.0f wherever the loss does not look
        if (c < 2) {
            const float code = ycls[m * 2 + c];
            const bool pos = is_pos(code);
            if (pos || is_neg(code)) {
                const double z = head[i];
                const double e = exp(-fabs(z));              // in (0, 1]: no overflow for any finite logit
                const double lo = e / (1.0 + e), hi = 1.0 / (1.0 + e);
                const double p = z >= 0.0 ? hi : lo, q = z >= 0.0 ? lo : hi;     // sigmoid(z), 1 - sigmoid(z)
                // a positive looks at -z: the roles of p and q swap
                const double x = pos ? -z : z, s = softplus_e(x, e);
                const double px = pos ? q : p, qx = pos ? p : q;                 // sigmoid(x), 1 - sigmoid(x)
                double v = s, dv = px;                                           // gamma == 0: sp(x), d sp / dx
                if (g != 0.0) {
                    const double f = pow(px, g);
                    v = f * s;
                    dv = f * (g * qx * s + px);
                }
                if constexpr (WEIGHTED) {
                    const double w = (double)cell_weight(cw, sws, 0, m);
                    if (pos) spos += w * v; else sneg += w * v;
                    if (grad) gout = (float)(pos ? -((wpos * w) * dv) : (wneg * w) * dv);
                } else {
                    if (pos) spos += v; else sneg += v;
                    if (grad) gout = (float)(pos ? -(wpos * dv) : wneg * dv);    // dx/dz = -1 on a positive
                }
            }
        } else {
            const int a = c < 9 ? 0 : 1;
            if (is_pos(ycls[m * 2 + a])) {
                const double d = (double)head[i] - ((double)yreg[m * 14 + (c - 2)] - cfg.target_offset);
                if constexpr (WEIGHTED) {
                    const double w = (double)cell_weight(cw, sws, 1, m);
                    sreg += w * smooth_l1(d, b);
                    if (grad) gout = (float)((wreg * w) * smooth_l1_grad(d, b));
                } else {
                    sreg += smooth_l1(d, b);
                    if (grad) gout = (float)(wreg * smooth_l1_grad(d, b));
                }
            }
        }
        if (grad) dhead[i] = gout;
    }
    const double v[kDetVals] = {spos, sneg, sreg};
    const double a = block_sum_own<kDetThreads>(v, red);
    if (threadIdx.x < kDetVals) parts[(size_t)blockIdx.x * kDetVals + threadIdx.x] = a;
}

// Training (acc == nullptr): loss_out[3]; evaluation: the same fp32 values added, as doubles, to acc, the sweep counted.
__global__ void __launch_bounds__(256)
k_det_finalize(lisec_detection_loss_cfg cfg, const double* __restrict__ parts, int nparts,
               const long long* __restrict__ counts, float* __restrict__ loss_out, double* __restrict__ acc) {
    __shared__ double red[kDetVals][256];
    double a[kDetVals];
    strided_sums<256>(parts, nparts, a);
    tree_sums<256>(a, red);
    if (threadIdx.x != 0) return;
    const long long cp = counts[0], cn = counts[1];
    const double npos = cp > 0 ? (double)cp : 1.0, nneg = cn > 0 ? (double)cn : 1.0;
    const double lc = cfg.alpha * red[0][0] / npos + cfg.beta * red[1][0] / nneg, lr = red[2][0] / npos;
    const float tot = (float)(cfg.weight[0] * lc + cfg.weight[1] * lr), fc = (float)lc, fr = (float)lr;
    if (acc) {
        acc[0] += (double)tot; acc[1] += (double)fc; acc[2] += (double)fr; acc[3] += 1.0;
    } else {
        loss_out[0] = tot; loss_out[1] = fc; loss_out[2] = fr;
    }
}

int check_det(const lisec_detection_loss_cfg* cfg, long long M, const void* workspace, size_t workspace_bytes) {
    LISEC_CHECK_ARG(cfg, "detection loss: NULL descriptor");
    LISEC_CHECK_ARG(cfg->struct_bytes == (int)sizeof(lisec_detection_loss_cfg),
                    "detection loss: descriptor of %d bytes, this library's has %d", cfg->struct_bytes,
                    (int)sizeof(lisec_detection_loss_cfg));
    LISEC_CHECK_ARG(cfg->alpha >= 0.0 && cfg->beta >= 0.0 && cfg->gamma >= 0.0,
                    "detection loss: alpha, beta and gamma must be >= 0 (got %g, %g, %g)", cfg->alpha, cfg->beta, cfg->gamma);
    LISEC_CHECK_ARG(cfg->smooth_l1_beta > 0.0, "detection loss: smooth_l1_beta must be > 0 (got %g)", cfg->smooth_l1_beta);
    LISEC_CHECK_ARG(M > 0, "detection loss: M must be > 0 (got %lld)", M);
    LISEC_CHECK_ARG(workspace, "detection loss: NULL workspace");
    LISEC_CHECK_ARG(workspace_bytes >= lisec_detection_loss_workspace_bytes(),
                    "detection loss: workspace of %zu bytes, %zu needed", workspace_bytes,
                    lisec_detection_loss_workspace_bytes());
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec
