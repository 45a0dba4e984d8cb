// Metrics that read the 0 / 1 / 2 label code of the VoxelNet detection loss (include/lisec_hip.h, lisec_detection_metrics):
// anchor precision / recall / accuracy of the class logits, mean absolute error and box IoU of the regression output on the
// positives.  Each metric is a pair {num, den} of sums over the 2M anchors of a sweep.  Two launches:
//   k_detm_anchors   thread j holds anchor j = 2m + a (y_cls is read as it lies): the code, the logit, and -- on a positive
//                    only -- its seven regression channels, the decode of k_rpn_decode (csrc/boxes.hip) without the centre
//                    both boxes share, and pair_iou (box_geom.h); everything in double from the fp32 inputs; per-workgroup
//                    fp64 partials of the 2 * n_metrics sums
//   k_detm_finalize  one workgroup: the partials summed in index order, stored to out or added to it
// No atomics and a fixed partition (k_detm_anchors: order W of reduce.h; the finalize has a strand order of its own), the
// house rules of detection_loss.hip: every address fixed, nothing read back, so the launches record into a step plan.
// Positives are ~1 % of the anchors, so the clipping branch is rare and divergent: a wave that holds one positive pays for
// it alone.  At 40 000 anchors (the Lyft grid) that is 157 workgroups of 4 waves, under one per compute unit, and the launch
// is bound by its latency, not by the lanes idle in the branch; no compaction pass is worth a third launch.  256 threads,
// four waves, per workgroup: the compiler reports 196 VGPRs (2 waves per SIMD), 528 bytes of scratch per lane for the clipping
// buffers of quad_intersection_area and 16.5 KiB of LDS (a per-thread array it moves there, and 512 bytes of partials) -- one
// workgroup per compute unit fits with room to spare, and that is all this launch asks for.
#include "box_geom.h"
#include "reduce.h"

namespace lisec {
namespace {

constexpr int kDetmThreads = 256;
constexpr int kDetmBlocks = 1024;                              // workgroups at most; beyond, each strides on
constexpr int kDetmVals = 2 * LISEC_DET_MAX_METRICS;           // partials per workgroup: num0, den0, num1, den1, ...

// is_pos / is_neg of detection_loss.hip: a NaN code compares false twice and is ignored
__device__ __forceinline__ bool is_pos(float code) { return code > 1.5f; }
__device__ __forceinline__ bool is_neg(float code) { return code > 0.5f && code <= 1.5f; }

__global__ void __launch_bounds__(kDetmThreads)
k_detm_anchors(lisec_detection_metrics_cfg cfg, const float* __restrict__ head, const float* __restrict__ ycls,
               const float* __restrict__ yreg, long long M, double* __restrict__ parts) {
    __shared__ double red[kDetmVals][kDetmThreads / 64];
    const int nmet = cfg.n_metrics;
    bool want_mae = false, want_iou[2] = {false, false};       // [LISEC_IOU_3D], [LISEC_IOU_BEV]
#pragma unroll
    for (int i = 0; i < LISEC_DET_MAX_METRICS; ++i) {
        if (i < nmet) {
            if (cfg.metric[i].kind == LISEC_DET_METRIC_POSITIVE_MAE) want_mae = true;
            if (cfg.metric[i].kind == LISEC_DET_METRIC_POSITIVE_IOU) {
                if (cfg.metric[i].mode == LISEC_IOU_3D) want_iou[0] = true; else want_iou[1] = true;
            }
        }
    }
    double num[LISEC_DET_MAX_METRICS], den[LISEC_DET_MAX_METRICS];
#pragma unroll
    for (int i = 0; i < LISEC_DET_MAX_METRICS; ++i) num[i] = den[i] = 0.0;
    const long long n = M * 2;
    for (long long base = blockIdx.x * (long long)kDetmThreads; base < n; base += (long long)gridDim.x * kDetmThreads) {
        const long long j = base + threadIdx.x;
        if (j >= n) break;
        const float code = ycls[j];
        const bool pos = is_pos(code), neg = is_neg(code);
        if (!pos && !neg) continue;
        const long long m = j >> 1;
        const int a = (int)(j & 1);
        const double z = head[m * 16 + a];
        const double e = exp(-fabs(z));                        // in (0, 1]: no overflow for any finite logit
        const double prob = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        double mae = 0.0, iou[2] = {0.0, 0.0};
        if (pos && (want_mae || want_iou[0] || want_iou[1])) {
            double r[7], t[7], an[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) an[k] = a ? cfg.anchors[1][k] : cfg.anchors[0][k];    // a select: no indexed copy
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                r[k] = head[m * 16 + 2 + 7 * a + k];
                t[k] = (double)yreg[m * 14 + 7 * a + k] - cfg.target_offset;
                mae += fabs(r[k] - t[k]);
            }
            if (want_iou[0]) iou[0] = decoded_iou(r, t, an, LISEC_IOU_3D);
            if (want_iou[1]) iou[1] = decoded_iou(r, t, an, LISEC_IOU_BEV);
        }
#pragma unroll
        for (int i = 0; i < LISEC_DET_MAX_METRICS; ++i) {
            if (i >= nmet) continue;
            const bool pred = prob > cfg.metric[i].threshold;  // false for a NaN logit
            switch (cfg.metric[i].kind) {
            case LISEC_DET_METRIC_ANCHOR_PRECISION:
                num[i] += pos && pred ? 1.0 : 0.0;
                den[i] += pred ? 1.0 : 0.0;
                break;
            case LISEC_DET_METRIC_ANCHOR_RECALL:
                num[i] += pos && pred ? 1.0 : 0.0;
                den[i] += pos ? 1.0 : 0.0;
                break;
            case LISEC_DET_METRIC_ANCHOR_ACCURACY:
                num[i] += pos == pred ? 1.0 : 0.0;             // pos and predicted, or neg and not predicted
                den[i] += 1.0;
                break;
            case LISEC_DET_METRIC_POSITIVE_MAE:
                num[i] += mae;                                 // 0 on a negative
                den[i] += pos ? 7.0 : 0.0;
                break;
            default:                                           // LISEC_DET_METRIC_POSITIVE_IOU
                num[i] += cfg.metric[i].mode == LISEC_IOU_3D ? iou[0] : iou[1];
                den[i] += pos ? 1.0 : 0.0;
                break;
            }
        }
    }
    double v[kDetmVals];
#pragma unroll
    for (int i = 0; i < LISEC_DET_MAX_METRICS; ++i) {
        v[2 * i] = num[i];
        v[2 * i + 1] = den[i];
    }
    const double s = block_sum_own<kDetmThreads>(v, red);
    if (threadIdx.x < kDetmVals) parts[(size_t)blockIdx.x * kDetmVals + threadIdx.x] = s;
}

// thread t sums value t & 15 over the workgroups (t >> 4) + 16 i in index order; 16 threads then add the 16 strands in order
__global__ void __launch_bounds__(256)
k_detm_finalize(const double* __restrict__ parts, int nparts, int nvals, double* __restrict__ out, int accumulate) {
    __shared__ double red[kDetmVals][16];
    const int v = threadIdx.x & (kDetmVals - 1), g = threadIdx.x >> 4;
    double s = 0.0;
    for (int p = g; p < nparts; p += 16) s += parts[(size_t)p * kDetmVals + v];
    red[v][g] = s;
    __syncthreads();
    if ((int)threadIdx.x >= nvals) return;
    double total = 0.0;
    for (int k = 0; k < 16; ++k) total += red[threadIdx.x][k];
    out[threadIdx.x] = accumulate ? out[threadIdx.x] + total : total;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_detection_metrics_workspace_bytes(void) {
    return align_up(sizeof(double) * (size_t)kDetmBlocks * kDetmVals, 256);
}

extern "C" int lisec_detection_metrics(const lisec_detection_metrics_cfg* cfg, const float* head, const float* y_cls,
                                       const float* y_reg, long long M, double* out, int accumulate, void* workspace,
                                       size_t workspace_bytes, lisec_stream_t stream_) {
    static_assert(kDetmVals == 16, "k_detm_finalize splits a workgroup into 16 values x 16 strands");
    LISEC_CHECK_ARG(cfg, "detection metrics: NULL descriptor");
    LISEC_CHECK_ARG(cfg->struct_bytes == (int)sizeof(lisec_detection_metrics_cfg),
                    "detection metrics: descriptor of %d bytes, this library's has %d", cfg->struct_bytes,
                    (int)sizeof(lisec_detection_metrics_cfg));
    LISEC_CHECK_ARG(cfg->n_metrics >= 1 && cfg->n_metrics <= LISEC_DET_MAX_METRICS,
                    "detection metrics: n_metrics must lie in 1..%d (got %d)", LISEC_DET_MAX_METRICS, cfg->n_metrics);
    for (int i = 0; i < cfg->n_metrics; ++i) {
        const lisec_detection_metric& t = cfg->metric[i];
        LISEC_CHECK_ARG(t.kind >= LISEC_DET_METRIC_ANCHOR_PRECISION && t.kind <= LISEC_DET_METRIC_POSITIVE_IOU,
                        "detection metrics: unknown kind %d of metric %d", t.kind, i);
        if (t.kind == LISEC_DET_METRIC_POSITIVE_IOU) {
            LISEC_CHECK_ARG(t.mode == LISEC_IOU_3D || t.mode == LISEC_IOU_BEV,
                            "detection metrics: unknown IoU mode %d of metric %d", t.mode, i);
        } else if (t.kind != LISEC_DET_METRIC_POSITIVE_MAE) {
            LISEC_CHECK_ARG(t.threshold > 0.0 && t.threshold < 1.0,
                            "detection metrics: the threshold of metric %d must lie in (0, 1) (got %g)", i, t.threshold);
        }
    }
    LISEC_CHECK_ARG(M > 0, "detection metrics: M must be > 0 (got %lld)", M);
    LISEC_CHECK_ARG(head && y_cls && y_reg && out, "detection metrics: NULL pointer");
    LISEC_CHECK_ARG(workspace, "detection metrics: NULL workspace");
    LISEC_CHECK_ARG(workspace_bytes >= lisec_detection_metrics_workspace_bytes(),
                    "detection metrics: workspace of %zu bytes, %zu needed", workspace_bytes,
                    lisec_detection_metrics_workspace_bytes());
    hipStream_t st = static_cast<hipStream_t>(stream_);
    double* parts = static_cast<double*>(workspace);
    const int nb = grid_blocks(M * 2, kDetmThreads, kDetmBlocks);
    LISEC_LAUNCH(k_detm_anchors, dim3(nb), dim3(kDetmThreads), 0, st, *cfg, head, y_cls, y_reg, M, parts);
    LISEC_LAUNCH(k_detm_finalize, dim3(1), dim3(256), 0, st, parts, nb, 2 * cfg->n_metrics, out, accumulate);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
