// The VoxelNet detection loss with a rotated-box IoU term in the regression part (include/lisec_hip.h,
// lisec_detection_iou_loss*):  L_reg = 1/N_pos sum_pos [ sum_k S(r_k - t_k) + iou_weight (1 - IoU(decode r, decode t)) ].
// Four launches: the three of detection_loss_parts.h, and between the element pass and the finalize
//   k_det_iou       thread j holds anchor j = 2m + a, as k_detm_anchors (csrc/detection_metrics.hip); on a positive only:
//                   the decode and pair_iou of the PositiveIoU metric (box_geom.h), the gradient of the IoU in closed form,
//                   and the seven regression channels of dhead stored AGAIN, as the SmoothL1 derivative plus the IoU part
//                   summed in double and rounded once -- where the IoU part is zero that is the bit pattern k_det_loss
//                   stored.  Workgroup b adds iou_weight * sum (1 - IoU) of its anchors to the regression partial of
//                   workgroup b of the element pass (there are never more anchor workgroups than element workgroups), so
//                   k_det_finalize and the workspace are the ones of lisec_detection_loss.
// A fourth launch rather than a branch of the element pass: there a positive's seven channels sit in seven lanes, which
// would clip the same pair of footprints seven times or pass one lane's result through LDS; here one thread holds the
// anchor, and the pass reads 2M codes and touches the ~1 % of positives.
// The gradient needs no differentiation through the clipping: d area(P n G)/d theta is the integral of the normal velocity
// of P's boundary over the parts of it inside G.  Each edge of P meets the convex G in one interval (the edge clipped against
// G's four half-planes, in G's frame) and the velocity is linear along an edge, so midpoint times length is exact.
// No atomics, a fixed partition (order W of reduce.h), every address fixed, nothing read back: the house rules of
// detection_loss.hip.
// 256 threads per workgroup; for k_det_iou the compiler reports 164 VGPRs (3 waves per SIMD), 464 bytes of scratch per lane
// (the clipping buffers of quad_intersection_area) and 16 KiB of LDS (a per-thread array it moves there, and 32 bytes of
// partials): at 40 000 anchors that is 157 workgroups, under one per compute unit, and the launch is bound by its latency.
#include "box_geom.h"
#include "detection_loss_parts.h"

namespace lisec {
namespace {

constexpr int kIouThreads = 256;
constexpr int kIouBlocks = 1024;                               // workgroups at most; beyond, each strides on

// the part of lo <= t <= hi where |c0 + t c1| <= lim; an empty interval has hi < lo
__device__ __forceinline__ void clip_slab(double c0, double c1, double lim, double& lo, double& hi) {
    if (c1 == 0.0) {
        if (fabs(c0) > lim) hi = lo - 1.0;
        return;
    }
    const double ta = (-lim - c0) / c1, tb = (lim - c0) / c1;
    lo = fmax(lo, fmin(ta, tb));
    hi = fmin(hi, fmax(ta, tb));
}

// d area(P n G) / d (x, y, l, w, yaw) of P = p, into da[5]; G = g is fixed.  Both footprints as box_corners has them: a
// boundary point of P is c + s u w/2 + t v l/2 with u = (cos yaw, -sin yaw), v = (sin yaw, cos yaw), s, t in [-1, 1].
__device__ void footprint_area_grad(const double* p, const double* g, double* da) {
    const double cs = cos(p[6]), sn = sin(p[6]), gc = cos(g[6]), gs = sin(g[6]);
    const double hw = 0.5 * p[4], hl = 0.5 * p[3], ghw = 0.5 * g[4], ghl = 0.5 * g[3];
    const double ux = cs, uy = -sn, vx = sn, vy = cs;
    const double dx = p[0] - g[0], dy = p[1] - g[1];
    // G's frame: a along its u, b along its v
    const double da0 = dx * gc - dy * gs, db0 = dx * gs + dy * gc;
    const double ua = ux * gc - uy * gs, ub = ux * gs + uy * gc;
    const double va = vx * gc - vy * gs, vb = vx * gs + vy * gc;
    double ax = 0.0, ay = 0.0, al = 0.0, aw = 0.0, ayaw = 0.0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const double sg = e ? -1.0 : 1.0;
        {   // the edge s = sg, t running: outward normal sg u
            double lo = -1.0, hi = 1.0;
            clip_slab(da0 + sg * hw * ua, hl * va, ghw, lo, hi);
            clip_slab(db0 + sg * hw * ub, hl * vb, ghl, lo, hi);
            if (hi > lo) {
                const double len = hl * (hi - lo), mid = 0.5 * (lo + hi);
                ax += sg * ux * len;
                ay += sg * uy * len;
                aw += 0.5 * len;
                ayaw += sg * mid * hl * len;
            }
        }
        {   // the edge t = sg, s running: outward normal sg v
            double lo = -1.0, hi = 1.0;
            clip_slab(da0 + sg * hl * va, hw * ua, ghw, lo, hi);
            clip_slab(db0 + sg * hl * vb, hw * ub, ghl, lo, hi);
            if (hi > lo) {
                const double len = hw * (hi - lo), mid = 0.5 * (lo + hi);
                ax += sg * vx * len;
                ay += sg * vy * len;
                al += 0.5 * len;
                ayaw -= sg * mid * hw * len;
            }
        }
    }
    da[0] = ax; da[1] = ay; da[2] = al; da[3] = aw; da[4] = ayaw;
}

// 1 - IoU of the decoded prediction r and target t of one anchor, and d (1 - IoU) / d r into dterm[7].  IoU 0 -- a box that
// is not finite, the early-outs of pair_iou, footprints or height intervals that do not meet -- leaves dterm at +0.0.
__device__ double iou_term(const double* r, const double* t, const double* an, int mode, double* dterm) {
#pragma unroll
    for (int k = 0; k < 7; ++k) dterm[k] = 0.0;
    double p[7], g[7];
    if (!decode_pair(r, t, an, p, g)) return 1.0;
    const double iou = pair_iou(p, g, mode);
    if (!(iou > 0.0) || !isfinite(iou)) return 1.0;
    const bool d3 = mode == LISEC_IOU_3D;
    // iou = I / (S - I) with S = S_p + S_g: U = S / (1 + iou) and I = iou U, without clipping twice
    const double fp = p[3] * p[4], sp = d3 ? fp * p[5] : fp, sg = d3 ? g[3] * g[4] * g[5] : g[3] * g[4];
    const double uni = (sp + sg) / (1.0 + iou), inter = iou * uni;
    double hz = 1.0, top_in = 0.0, bot_in = 0.0;
    if (d3) {
        const double pt = p[2] + 0.5 * p[5], pb = p[2] - 0.5 * p[5], gt = g[2] + 0.5 * g[5], gb = g[2] - 0.5 * g[5];
        hz = fmin(pt, gt) - fmax(pb, gb);
        top_in = pt < gt ? 1.0 : 0.0;
        bot_in = pb > gb ? 1.0 : 0.0;
    }
    double da[5];
    footprint_area_grad(p, g, da);
    // d I and d S_p by (x, y, z, l, w, h, yaw)
    const double area = inter / hz;
    const double di[7] = {da[0] * hz, da[1] * hz, area * (top_in - bot_in), da[2] * hz, da[3] * hz,
                          area * 0.5 * (top_in + bot_in), da[4] * hz};
    const double ds[7] = {0.0, 0.0, 0.0, d3 ? p[4] * p[5] : p[4], d3 ? p[3] * p[5] : p[3], d3 ? fp : 0.0, 0.0};
    // the decode: d p_k / d r_k
    const double chain[7] = {an[0], an[1], an[2], p[3], p[4], p[5], 1.0};
    double out[7];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double diou = (di[k] * (1.0 + iou) - iou * ds[k]) / uni;
        out[k] = (d3 || (k != 2 && k != 5)) ? -(diou * chain[k]) : 0.0;
        ok = ok && isfinite(out[k]);
    }
    if (ok) {                                                  // products of extents near the end of the range: no gradient
#pragma unroll
        for (int k = 0; k < 7; ++k) dterm[k] = out[k];
    }
    return 1.0 - iou;
}

// dhead == nullptr: values only (the evaluation entry)
// WEIGHTED (one CellWeights behind parts): the anchor's term and its gradient carry w_reg of the anchor's cell, as in the weighted k_det_loss:
// (wreg * (double)w) times the derivative, the sum adds (double)w * (1 - IoU).
template <bool WEIGHTED, typename... W>
__global__ void __launch_bounds__(kIouThreads)
k_det_iou(lisec_detection_iou_loss_cfg cfg, const float* __restrict__ head, const float* __restrict__ ycls,
          const float* __restrict__ yreg, long long M, float gscale, const long long* __restrict__ counts,
          float* __restrict__ dhead, double* __restrict__ parts, W... cw_) {
    [[maybe_unused]] const CellWeights cw = the_weights(cw_...);
    __shared__ double red[1][kIouThreads / 64];
    const long long cp = counts[0];
    const double npos = cp > 0 ? (double)cp : 1.0;
    const double wreg = (double)gscale * cfg.det.weight[1] / npos;     // k_det_loss's
    const double b = cfg.det.smooth_l1_beta, iw = cfg.iou_weight;
    double sum = 0.0;
    [[maybe_unused]] SweepWeights sws = {};
    if constexpr (WEIGHTED) sws = sweep_weights(cw);
    const long long n = M * 2;
    for (long long base = blockIdx.x * (long long)kIouThreads; base < n; base += (long long)gridDim.x * kIouThreads) {
        const long long j = base + threadIdx.x;
        if (j >= n) break;
        if (!is_pos(ycls[j])) continue;
        const long long m = j >> 1;
        const int a = (int)(j & 1);
        double r[7], t[7], an[4], dterm[7];
#pragma unroll
        for (int k = 0; k < 4; ++k) an[k] = a ? cfg.anchors[1][k] : cfg.anchors[0][k];    // a select: no indexed copy
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            r[k] = head[m * 16 + 2 + 7 * a + k];
            t[k] = (double)yreg[m * 14 + 7 * a + k] - cfg.det.target_offset;
        }
        [[maybe_unused]] double w = 1.0;
        if constexpr (WEIGHTED) {
            w = (double)cell_weight(cw, sws, 1, m);
            sum += w * iou_term(r, t, an, cfg.iou_mode, dterm);
        } else {
            sum += iou_term(r, t, an, cfg.iou_mode, dterm);
        }
        if (dhead) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const double s = smooth_l1_grad(r[k] - t[k], b), e = iw * dterm[k];
                // e == 0: k_det_loss's bits
                if constexpr (WEIGHTED) dhead[m * 16 + 2 + 7 * a + k] = (float)((wreg * w) * (e != 0.0 ? s + e : s));
                else dhead[m * 16 + 2 + 7 * a + k] = (float)(wreg * (e != 0.0 ? s + e : s));
            }
        }
    }
    const double v[1] = {sum};
    double s[1];
    block_sums_all<kIouThreads>(v, red, s);
    // this workgroup alone writes the word, after k_det_loss
    if (threadIdx.x == 0) parts[(size_t)blockIdx.x * kDetVals + 2] += iw * s[0];
}

int check_iou(const lisec_detection_iou_loss_cfg* cfg, long long M, const void* workspace, size_t workspace_bytes) {
    LISEC_CHECK_ARG(cfg, "detection IoU loss: NULL descriptor");
    LISEC_CHECK_ARG(cfg->struct_bytes == (int)sizeof(lisec_detection_iou_loss_cfg),
                    "detection IoU loss: descriptor of %d bytes, this library's has %d", cfg->struct_bytes,
                    (int)sizeof(lisec_detection_iou_loss_cfg));
    LISEC_CHECK_ARG(cfg->iou_weight >= 0.0 && std::isfinite(cfg->iou_weight),
                    "detection IoU loss: iou_weight must be finite and >= 0 (got %g)", cfg->iou_weight);
    LISEC_CHECK_ARG(cfg->iou_mode == LISEC_IOU_3D || cfg->iou_mode == LISEC_IOU_BEV,
                    "detection IoU loss: unknown IoU mode %d", cfg->iou_mode);
    for (int a = 0; a < 2; ++a) {
        const double* an = cfg->anchors[a];
        LISEC_CHECK_ARG(std::isfinite(an[0]) && std::isfinite(an[1]) && std::isfinite(an[2]) && std::isfinite(an[3]) &&
                            an[0] > 0.0 && an[1] > 0.0 && an[2] > 0.0,
                        "detection IoU loss: anchor %d needs finite values and extents > 0 (got %g, %g, %g, %g)", a, an[0],
                        an[1], an[2], an[3]);
    }
    return check_det(&cfg->det, M, workspace, workspace_bytes);
}

int run_iou(const lisec_detection_iou_loss_cfg& cfg, const float* head, const float* y_cls, const float* y_reg,
            long long M, float grad_scale, float* dhead, float* loss_out, long long* counts_out, double* acc,
            void* workspace, hipStream_t st, const lisec_sample_weights* sw = nullptr) {
    static_assert(kIouBlocks <= kDetBlocks && kIouThreads * 8 >= kDetThreads,
                  "k_det_iou's workgroup b adds to the partial of k_det_loss's workgroup b");
    Carver ws(workspace);
    long long* counts = ws.take<long long>(2);
    double* parts = ws.take<double>((size_t)kDetBlocks * kDetVals);
    const int nb = grid_blocks(M * 16, kDetThreads, kDetBlocks);
    LISEC_LAUNCH(k_det_count, dim3(1), dim3(kCountThreads), 0, st, y_cls, M * 2, counts, counts_out);
    const int nbi = grid_blocks(M * 2, kIouThreads, kIouBlocks);
    if (sw) {
        const CellWeights cw = cell_weights(*sw);
        LISEC_LAUNCH(k_det_loss<true, CellWeights>, dim3(nb), dim3(kDetThreads), 0, st, cfg.det, head, y_cls, y_reg, M,
                     grad_scale, counts, dhead, parts, cw);
        LISEC_LAUNCH(k_det_iou<true, CellWeights>, dim3(nbi), dim3(kIouThreads), 0, st, cfg, head, y_cls, y_reg, M, grad_scale,
                     counts, dhead, parts, cw);
    } else {
        LISEC_LAUNCH(k_det_loss<false>, dim3(nb), dim3(kDetThreads), 0, st, cfg.det, head, y_cls, y_reg, M, grad_scale, counts,
                     dhead, parts);
        LISEC_LAUNCH(k_det_iou<false>, dim3(nbi), dim3(kIouThreads), 0, st, cfg, head, y_cls, y_reg, M, grad_scale, counts, dhead,
                     parts);
    }
    LISEC_LAUNCH(k_det_finalize, dim3(1), dim3(256), 0, st, cfg.det, parts, nb, counts, loss_out, acc);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_detection_iou_loss_workspace_bytes(void) { return lisec_detection_loss_workspace_bytes(); }

extern "C" int lisec_detection_iou_loss(const lisec_detection_iou_loss_cfg* cfg, const float* head, const float* y_cls,
                                        const float* y_reg, long long M, float grad_scale, float* dhead, float* loss_out,
                                        long long* counts_out, void* workspace, size_t workspace_bytes,
                                        lisec_stream_t stream_) {
    if (int rc = check_iou(cfg, M, workspace, workspace_bytes)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && counts_out, "detection IoU loss: NULL pointer");
    return run_iou(*cfg, head, y_cls, y_reg, M, grad_scale, dhead, loss_out, counts_out, nullptr, workspace,
                   static_cast<hipStream_t>(stream_));
}

extern "C" int lisec_detection_iou_loss_eval(const lisec_detection_iou_loss_cfg* cfg, const float* head,
                                             const float* y_cls, const float* y_reg, long long M, double* acc,
                                             void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_iou(cfg, M, workspace, workspace_bytes)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc, "detection IoU loss: NULL pointer");
    return run_iou(*cfg, head, y_cls, y_reg, M, 1.0f, nullptr, nullptr, nullptr, acc, workspace,
                   static_cast<hipStream_t>(stream_));
}

// The weighted entries: the same four launches with the weighted k_det_loss and k_det_iou, the same workspace.
extern "C" size_t lisec_detection_iou_loss_weighted_workspace_bytes(void) { return lisec_detection_loss_workspace_bytes(); }

extern "C" int lisec_detection_iou_loss_weighted(const lisec_detection_iou_loss_cfg* cfg, const lisec_sample_weights* sw,
                                                 const float* head, const float* y_cls, const float* y_reg, long long M,
                                                 float grad_scale, float* dhead, float* loss_out, long long* counts_out,
                                                 void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_iou(cfg, M, workspace, workspace_bytes)) return rc;
    if (int rc = check_sample_weights(sw, nullptr)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && counts_out, "detection IoU loss: NULL pointer");
    return run_iou(*cfg, head, y_cls, y_reg, M, grad_scale, dhead, loss_out, counts_out, nullptr, workspace,
                   static_cast<hipStream_t>(stream_), sw);
}

extern "C" int lisec_detection_iou_loss_weighted_eval(const lisec_detection_iou_loss_cfg* cfg,
                                                      const lisec_sample_weights* sw, const float* head,
                                                      const float* y_cls, const float* y_reg, long long M, double* acc,
                                                      void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_iou(cfg, M, workspace, workspace_bytes)) return rc;
    if (int rc = check_sample_weights(sw, nullptr)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc, "detection IoU loss: NULL pointer");
    return run_iou(*cfg, head, y_cls, y_reg, M, 1.0f, nullptr, nullptr, nullptr, acc, workspace,
                   static_cast<hipStream_t>(stream_), sw);
}
