// Detection average precision (gfx950): score-ranked boxes against annotations at a list of IoU thresholds, the PASCAL-VOC
// style rule of DESIGN section 7 (no counterpart in the reference, whose only check is calcIoUAll; parity unpinned).
//
//   lisec_boxes_pair_iou           the pairwise IoU matrices alone, into the caller's buffer (boxes.box_iou)
//   lisec_boxes_match              pairwise IoU matrices, each prediction's candidate label, true / false positive per threshold
//   lisec_boxes_average_precision  ranked cumulative TP count, precision envelope from the right, the recall-weighted sum
//
// IoU (ours, like bev_iou: geometrically consistent, NOT calculateIoU with its unclamped z term):
//   3d   inter = area(fp_p n fp_g) * max(0, min(z_p + |h_p|/2, z_g + |h_g|/2) - max(z_p - |h_p|/2, z_g - |h_g|/2))
//        union = |l w h|_p + |l w h|_g - inter,  iou = inter / union, 0 when union <= 0
//   bev  the same with areas only.
// The footprint is box_corners' quadrilateral, the clipping quad_intersection_area, the IoU pair_iou (all box_geom.h), a pair
// per thread.  The pair offsets, the pair kernel and the owner search are detection_pairs.h's, shared with detection_eval.hip.
//
// The take-or-miss walk without a serial part.  In rank order a prediction is a true positive at t when its candidate's IoU
// exceeds t and the candidate is still free at t.  A label is taken at t by the FIRST prediction in rank order that has it as
// candidate with iou > t, and stays taken: so after any set J of earlier predictions, "label c is taken at t" is exactly
// "some j in J has candidate c and iou_j > t".  Hence, with m_i = max iou_j over the predictions j of the same sample that
// rank before i and share i's candidate,
//        tp_i(t) = iou_i > t  and not  m_i > t,
// which every prediction evaluates on its own, for all thresholds at once, by one pass over the sample's predictions; "j ranks
// before i" is score_j > score_i, or equal scores and j the lower row (sample-major rows: the global tie rule restricted to
// one sample).  No flags are kept and nothing depends on the order in which threads run.
//
// float64 and integers only; the one accumulation (tp_count) is an integer atomic, the AP sum has a fixed order: results are
// bit-identical from run to run.  Latency-bound scalar code, no MFMA; LDS only for the scans of the integration.
#include "detection_pairs.h"

namespace lisec {
namespace {

// the label of the prediction's own sample with the largest IoU, the lowest row among equals; -1 / 0.0 without labels
__global__ void __launch_bounds__(kThreads)
k_candidates(const int32_t* __restrict__ pred_start, const int32_t* __restrict__ label_start, int n_samples, int total_pred,
             const long long* __restrict__ pair_off, const int* __restrict__ ok, const double* __restrict__ iou,
             double* __restrict__ best_iou, int32_t* __restrict__ best_label) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= total_pred) return;
    if (!*ok) { best_iou[g] = nan(""); best_label[g] = -1; return; }
    const int s = owner(pred_start, n_samples, g);
    const int nL = label_start[s + 1] - label_start[s];
    const double* row = iou + pair_off[s] + (long long)(g - pred_start[s]) * nL;
    double best = 0.0;
    int at = -1;
    if (nL > 0) { best = row[0]; at = 0; }
    for (int j = 1; j < nL; ++j) {
        const double v = row[j];
        if (v > best) { best = v; at = j; }
    }
    best_iou[g] = best;
    best_label[g] = at;
}

__global__ void __launch_bounds__(kThreads)
k_match(const double* __restrict__ scores, const int32_t* __restrict__ pred_start, int n_samples, int total_pred, Thresholds thr,
        const int* __restrict__ ok, const double* __restrict__ best_iou, const int32_t* __restrict__ best_label,
        uint8_t* __restrict__ tp, int32_t* __restrict__ tp_count) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= total_pred) return;
    if (!*ok) {                                                // nothing that could pass for a result: tp_count is -1 already
        for (int t = 0; t < thr.n; ++t) tp[(size_t)t * total_pred + g] = 0;
        return;
    }
    const int s = owner(pred_start, n_samples, g);
    const int p0 = pred_start[s], p1 = pred_start[s + 1];
    const int c = best_label[g];
    const double v = best_iou[g], sc = scores[g];
    double m = -1.0;                                           // the best IoU an earlier-ranked prediction brought to label c
    for (int j = p0; j < p1 && c >= 0; ++j) {
        if (j == g || best_label[j] != c) continue;
        const double sj = scores[j];
        if (sj > sc || (sj == sc && j < g)) m = fmax(m, best_iou[j]);
    }
    for (int t = 0; t < thr.n; ++t) {
        const bool hit = c >= 0 && v > thr.t[t] && !(m > thr.t[t]);
        tp[(size_t)t * total_pred + g] = hit;
        if (hit) atomicAdd(&tp_count[(size_t)s * thr.n + t], 1);
    }
}

// One workgroup per threshold.  With C = all true positives, the walk runs from the right in chunks of kScan ranks: the
// cumulative count at rank k is C minus the hits to its right, the envelope the running maximum of cum / k from the right,
// and only ranks that are hits move the recall: AP = sum over hits of (cum / G - (cum - 1) / G) * envelope.
__global__ void __launch_bounds__(kScan)
k_average_precision(const int64_t* __restrict__ rank, const uint8_t* __restrict__ tp, int N, int G, double* __restrict__ out_ap,
                    double* __restrict__ out_curve) {
    __shared__ int cnt[kScan];
    __shared__ double mx[kScan];
    const int t = blockIdx.x, tid = threadIdx.x;
    const uint8_t* row = tp + (size_t)t * N;
    auto hit_at = [&](int k) -> int {
        const long long r = rank[k];
        return r >= 0 && r < N ? row[r] != 0 : 0;              // a rank outside the table counts as a miss, never a stray read
    };
    int mine = 0;
    for (int k = tid; k < N; k += kScan) mine += hit_at(k);
    cnt[tid] = mine;
    __syncthreads();
    for (int o = kScan / 2; o > 0; o >>= 1) {
        if (tid < o) cnt[tid] += cnt[tid + o];
        __syncthreads();
    }
    const int C = cnt[0];
    int right = 0;                                             // hits to the right of the current chunk
    double env_right = 0.0, acc = 0.0;                         // mpre ends with 0
    for (int chunk = (N + kScan - 1) / kScan - 1; chunk >= 0; --chunk) {
        const int k = chunk * kScan + tid;
        const int flag = k < N ? hit_at(k) : 0;
        __syncthreads();
        cnt[tid] = flag;
        __syncthreads();
        for (int o = 1; o < kScan; o <<= 1) {                  // inclusive suffix sum
            const int u = tid + o < kScan ? cnt[tid + o] : 0;
            __syncthreads();
            cnt[tid] += u;
            __syncthreads();
        }
        const int cum = C - right - (cnt[tid] - flag);
        const double prec = k < N ? (double)cum / (double)(k + 1) : 0.0;
        mx[tid] = prec;
        __syncthreads();
        for (int o = 1; o < kScan; o <<= 1) {                  // inclusive suffix maximum
            const double u = tid + o < kScan ? mx[tid + o] : 0.0;
            __syncthreads();
            mx[tid] = fmax(mx[tid], u);
            __syncthreads();
        }
        const double env = fmax(mx[tid], env_right);
        if (flag) acc += ((double)cum / (double)G - (double)(cum - 1) / (double)G) * env;
        if (out_curve && k < N) {
            double* o = out_curve + ((size_t)t * N + k) * 2;
            o[0] = (double)cum / (double)G;
            o[1] = prec;
        }
        right += cnt[0];
        env_right = fmax(env_right, mx[0]);
    }
    __syncthreads();
    mx[tid] = acc;
    __syncthreads();
    for (int o = kScan / 2; o > 0; o >>= 1) {                  // fixed tree
        if (tid < o) mx[tid] += mx[tid + o];
        __syncthreads();
    }
    if (tid == 0) out_ap[t] = mx[0];
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_boxes_match_workspace_bytes(int n_samples, int total_pred, long long total_pairs, int n_thresholds) {
    if (!sizes_ok(n_samples, total_pred, total_pairs, n_thresholds)) return 0;
    return MatchWs(nullptr, n_samples, total_pairs).bytes;
}

extern "C" int lisec_boxes_match(const double* pred_boxes, const double* pred_scores, const int32_t* pred_start,
                                 const double* label_boxes, const int32_t* label_start, int n_samples, int total_pred,
                                 long long total_pairs, const double* thresholds, int n_thresholds, int mode, void* workspace,
                                 size_t workspace_bytes, double* best_iou, int32_t* best_label, uint8_t* tp, int32_t* tp_count,
                                 lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxThresholds && thresholds,
                    "boxes_match takes 1 to %d IoU thresholds", kMaxThresholds);
    Thresholds thr;
    thr.n = n_thresholds;
    for (int t = 0; t < kMaxThresholds; ++t) thr.t[t] = t < n_thresholds ? thresholds[t] : 0.0;
    for (int t = 0; t < n_thresholds; ++t)
        LISEC_CHECK_ARG(thr.t[t] >= 0.0 && thr.t[t] < 1.0, "IoU threshold %d = %g is outside [0, 1)", t, thr.t[t]);
    LISEC_CHECK_ARG(mode == LISEC_IOU_3D || mode == LISEC_IOU_BEV, "unknown IoU mode %d", mode);
    LISEC_CHECK_ARG(sizes_ok(n_samples, total_pred, total_pairs, n_thresholds) && pred_start && label_start && workspace &&
                    tp_count && (total_pred == 0 || (pred_boxes && pred_scores && best_iou && best_label && tp)) &&
                    (total_pairs == 0 || label_boxes), "bad arguments");
    MatchWs ws(workspace, n_samples, total_pairs);
    if (workspace_bytes < ws.bytes) {
        set_error("boxes_match workspace too small");
        return LISEC_ENOSPC;
    }
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (int rc = launch_pair_iou(pred_boxes, pred_start, label_boxes, label_start, n_samples, total_pred, total_pairs,
                                 n_thresholds, mode, ws.pair_off, ws.ok, ws.iou, tp_count, st))
        return rc;
    if (total_pred > 0) {
        LISEC_LAUNCH(k_candidates, dim3(cdiv(total_pred, kThreads)), dim3(kThreads), 0, st, pred_start, label_start, n_samples,
                     total_pred, ws.pair_off, ws.ok, ws.iou, best_iou, best_label);
        LISEC_LAUNCH(k_match, dim3(cdiv(total_pred, kThreads)), dim3(kThreads), 0, st, pred_scores, pred_start, n_samples,
                     total_pred, thr, ws.ok, best_iou, best_label, tp, tp_count);
    }
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_boxes_pair_iou(const double* pred_boxes, const int32_t* pred_start, const double* label_boxes,
                                    const int32_t* label_start, int n_samples, int total_pred, long long total_pairs, int mode,
                                    void* workspace, size_t workspace_bytes, double* out_iou, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(mode == LISEC_IOU_3D || mode == LISEC_IOU_BEV, "unknown IoU mode %d", mode);
    LISEC_CHECK_ARG(sizes_ok(n_samples, total_pred, total_pairs, 1) && pred_start && label_start && workspace &&
                    (total_pairs == 0 || (pred_boxes && label_boxes && out_iou)), "bad arguments");
    MatchWs ws(workspace, n_samples, 0);                       // the offsets and the consistency word only
    if (workspace_bytes < ws.bytes) {
        set_error("boxes_pair_iou workspace too small");
        return LISEC_ENOSPC;
    }
    return launch_pair_iou(pred_boxes, pred_start, label_boxes, label_start, n_samples, total_pred, total_pairs, 0, mode,
                           ws.pair_off, ws.ok, out_iou, nullptr, static_cast<hipStream_t>(stream_));
}

extern "C" int lisec_boxes_average_precision(const int64_t* rank, const uint8_t* tp, int n_pred, int n_labels, int n_thresholds,
                                             double* out_ap, double* out_curve, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n_labels > 0, "average precision needs at least one label (G = %d)", n_labels);
    LISEC_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxThresholds && n_pred >= 0 && out_ap &&
                    (n_pred == 0 || (rank && tp)), "bad arguments");
    LISEC_LAUNCH(k_average_precision, dim3(n_thresholds), dim3(kScan), 0, static_cast<hipStream_t>(stream_), rank, tp, n_pred,
                 n_labels, out_ap, out_curve);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
