// Detection evaluation (gfx950): the matcher and integrator of detection_ap.hip with what a lidar benchmark adds to them --
// ignored labels and predictions, a heading-aware score, the true-positive errors and the best-F1 operating point.  The
// definition is DESIGN section 7's and include/lisec_hip.h's; not in the reference, parity with any devkit unpinned.
//
//   lisec_boxes_evaluate            pairwise IoU (detection_pairs.h, the same kernels as lisec_boxes_match), each prediction's
//                                   candidate among the NON-ignored labels, its largest IoU with an ignored one, the four
//                                   geometry words against the candidate, the state (FP / TP / ignored) per threshold
//   lisec_boxes_evaluate_integrate  AP, AOS, ATE, ASE, AOE, best F1 and its score per threshold, one workgroup each
//
// The state keeps k_match's form: with m_i = the largest candidate IoU among the predictions of the same sample that rank
// before i and share i's candidate (a non-ignored label), tp_i(t) = best_iou_i > t and not m_i > t; a prediction that is no
// true positive is ignored at t when ignored_iou_i > t or its own flag is set, else a false positive.  An ignored label is
// never a candidate, so it is never taken and absorbs any number of predictions.
//
// The integration walks the ranks from the right in chunks of kScan, as k_average_precision does, with the ignored ranks
// contributing nothing: cumTP, cumFP and cumSim at a rank are the totals minus what lies to its right.  cumSim is carried
// in fixed point (two int64 limbs, resolution 2^-52 per addend, sim in [0, 1]): integer sums neither cancel nor depend on an
// order, so total - suffix is the prefix itself.  The AP sum has k_average_precision's terms and order: without flags its
// bits.  float64 and integers only, the one atomic an integer one (tp_count), every float sum a fixed tree.
#include "detection_pairs.h"

namespace lisec {
namespace {

constexpr int kWords = LISEC_EVAL_WORDS;

// candidates: the non-ignored label with the largest IoU (lowest row among equals), the largest IoU with an ignored label,
// and geom = (sim, dist, scale, yaw) against the candidate
__global__ void __launch_bounds__(kThreads)
k_eval_candidates(const double* __restrict__ pred, const int32_t* __restrict__ pred_start, const double* __restrict__ label,
                  const int32_t* __restrict__ label_start, const uint8_t* __restrict__ label_ignore, int n_samples,
                  int total_pred, const long long* __restrict__ pair_off, const int* __restrict__ ok,
                  const double* __restrict__ iou, double* __restrict__ best_iou, int32_t* __restrict__ best_label,
                  double* __restrict__ ignored_iou, double* __restrict__ geom) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= total_pred) return;
    double* o = geom + (size_t)g * 4;
    if (!*ok) {
        best_iou[g] = nan(""); best_label[g] = -1; ignored_iou[g] = nan("");
        o[0] = o[1] = o[2] = o[3] = nan("");
        return;
    }
    const int s = owner(pred_start, n_samples, g);
    const int l0 = label_start[s], nL = label_start[s + 1] - l0;
    const double* row = iou + pair_off[s] + (long long)(g - pred_start[s]) * nL;
    double best = 0.0, ign = 0.0;
    int at = -1;
    for (int j = 0; j < nL; ++j) {
        const double v = row[j];
        if (label_ignore && label_ignore[l0 + j]) { if (v > ign) ign = v; continue; }
        if (at < 0 || v > best) { best = v; at = j; }
    }
    best_iou[g] = best;
    best_label[g] = at;
    ignored_iou[g] = ign;
    if (at < 0) { o[0] = o[1] = o[2] = o[3] = nan(""); return; }
    const double* p = pred + (size_t)g * 7;
    const double* q = label + (size_t)(l0 + at) * 7;
    const double d = p[6] - q[6], sn = sin(d), cs = cos(d);
    const double dx = p[0] - q[0], dy = p[1] - q[1];
    const double vp = fabs(p[3] * p[4] * p[5]), vg = fabs(q[3] * q[4] * q[5]);
    const double v = fmin(fabs(p[3]), fabs(q[3])) * fmin(fabs(p[4]), fabs(q[4])) * fmin(fabs(p[5]), fabs(q[5]));
    const double den = vp + vg - v;
    o[0] = 0.5 * (1.0 + cs);
    o[1] = sqrt(dx * dx + dy * dy);
    o[2] = den > 0.0 ? 1.0 - v / den : 1.0;
    o[3] = fabs(atan2(sn, cs));
}

__global__ void __launch_bounds__(kThreads)
k_eval_state(const double* __restrict__ scores, const int32_t* __restrict__ pred_start, const uint8_t* __restrict__ pred_ignore,
             int n_samples, int total_pred, Thresholds thr, const int* __restrict__ ok, const double* __restrict__ best_iou,
             const int32_t* __restrict__ best_label, const double* __restrict__ ignored_iou, uint8_t* __restrict__ state,
             int32_t* __restrict__ tp_count) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= total_pred) return;
    if (!*ok) {                                                // nothing that could pass for a result: tp_count is -1 already
        for (int t = 0; t < thr.n; ++t) state[(size_t)t * total_pred + g] = 0;
        return;
    }
    const int s = owner(pred_start, n_samples, g);
    const int p0 = pred_start[s], p1 = pred_start[s + 1];
    const int c = best_label[g];
    const double v = best_iou[g], sc = scores[g], ign = ignored_iou[g];
    const bool flagged = pred_ignore && pred_ignore[g];
    double m = -1.0;                                           // the best IoU an earlier-ranked prediction brought to label c
    for (int j = p0; j < p1 && c >= 0; ++j) {
        if (j == g || best_label[j] != c) continue;
        const double sj = scores[j];
        if (sj > sc || (sj == sc && j < g)) m = fmax(m, best_iou[j]);
    }
    for (int t = 0; t < thr.n; ++t) {
        const bool hit = c >= 0 && v > thr.t[t] && !(m > thr.t[t]);
        state[(size_t)t * total_pred + g] = hit ? 1 : (ign > thr.t[t] || flagged) ? 2 : 0;
        if (hit) atomicAdd(&tp_count[(size_t)s * thr.n + t], 1);
    }
}

// sim in [0, 1] as hi * 2^-20 + lo * 2^-52 with integer limbs (NaN and anything outside count as the nearer end)
__device__ __forceinline__ void sim_split(double s, long long& hi, long long& lo) {
    s = fmin(fmax(s, 0.0), 1.0);
    const double h = floor(s * 1048576.0);
    hi = (long long)h;
    lo = (long long)rint((s - h * (1.0 / 1048576.0)) * 4503599627370496.0);
}
__device__ __forceinline__ double sim_join(long long hi, long long lo) {
    hi += lo >> 32;                                            // both limbs exact in a double, one rounding in the sum
    lo &= 0xffffffffLL;
    return (double)hi * (1.0 / 1048576.0) + (double)lo * (1.0 / 4503599627370496.0);
}

// One workgroup per threshold; see the head of the file.
__global__ void __launch_bounds__(kScan)
k_eval_integrate(const int64_t* __restrict__ rank, const uint8_t* __restrict__ state, const double* __restrict__ geom,
                 const double* __restrict__ scores, int N, int G, double* __restrict__ out, double* __restrict__ out_curve) {
    __shared__ int cT[kScan], cF[kScan], fk[kScan];
    __shared__ long long sH[kScan], sL[kScan];
    __shared__ double mP[kScan], mO[kScan], fv[kScan];
    const int t = blockIdx.x, tid = threadIdx.x;
    const uint8_t* row = state + (size_t)t * N;
    auto row_at = [&](int k) -> long long {                    // the row ranked k-th, -1 for one outside the table
        const long long r = rank[k];
        return r >= 0 && r < N ? r : -1;
    };

    // the true-positive errors: sums over the rows in flat order, thread by thread, then a fixed tree
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    int rows = 0;
    for (int g = tid; g < N; g += kScan) {
        if (row[g] != 1) continue;
        const double* o = geom + (size_t)g * 4;
        e0 += o[1]; e1 += o[2]; e2 += o[3];
        ++rows;
    }
    mP[tid] = e0; mO[tid] = e1; fv[tid] = e2; cT[tid] = rows;
    __syncthreads();
    for (int o = kScan / 2; o > 0; o >>= 1) {
        if (tid < o) { mP[tid] += mP[tid + o]; mO[tid] += mO[tid + o]; fv[tid] += fv[tid + o]; cT[tid] += cT[tid + o]; }
        __syncthreads();
    }
    const double sum_dist = mP[0], sum_scale = mO[0], sum_yaw = fv[0];
    const int n_rows = cT[0];
    __syncthreads();

    // the totals over the ranks (a rank outside the table counts as a false positive, never a stray read)
    int myT = 0, myF = 0;
    long long myH = 0, myL = 0;
    for (int k = tid; k < N; k += kScan) {
        const long long r = row_at(k);
        const int st = r >= 0 ? row[r] : 0;
        if (st == 1) {
            long long h, l;
            sim_split(geom[(size_t)r * 4], h, l);
            ++myT; myH += h; myL += l;
        } else if (st == 0) ++myF;
    }
    cT[tid] = myT; cF[tid] = myF; sH[tid] = myH; sL[tid] = myL;
    __syncthreads();
    for (int o = kScan / 2; o > 0; o >>= 1) {
        if (tid < o) { cT[tid] += cT[tid + o]; cF[tid] += cF[tid + o]; sH[tid] += sH[tid + o]; sL[tid] += sL[tid + o]; }
        __syncthreads();
    }
    const int CT = cT[0], CF = cF[0];
    const long long CH = sH[0], CL = sL[0];

    int rightT = 0, rightF = 0;                                // what lies to the right of the current chunk
    long long rightH = 0, rightL = 0;
    double envP_right = 0.0, envO_right = 0.0, accP = 0.0, accO = 0.0;      // both envelopes end with 0
    double best_f1 = -1.0;
    int best_k = -1;
    for (int chunk = (N + kScan - 1) / kScan - 1; chunk >= 0; --chunk) {
        const int k = chunk * kScan + tid;
        int st = 2;                                            // past the end: as an ignored rank, nothing
        long long r = -1;
        if (k < N) {
            r = row_at(k);
            st = r >= 0 ? row[r] : 0;
        }
        const int flag = st == 1, miss = st == 0;
        long long h = 0, l = 0;
        if (flag) sim_split(geom[(size_t)r * 4], h, l);
        __syncthreads();
        cT[tid] = flag; cF[tid] = miss; sH[tid] = h; sL[tid] = l;
        __syncthreads();
        for (int o = 1; o < kScan; o <<= 1) {                  // inclusive suffix sums
            const bool in = tid + o < kScan;
            const int uT = in ? cT[tid + o] : 0, uF = in ? cF[tid + o] : 0;
            const long long uH = in ? sH[tid + o] : 0, uL = in ? sL[tid + o] : 0;
            __syncthreads();
            cT[tid] += uT; cF[tid] += uF; sH[tid] += uH; sL[tid] += uL;
            __syncthreads();
        }
        const int cum = CT - rightT - (cT[tid] - flag);
        const int cumF = CF - rightF - (cF[tid] - miss);
        const double cumSim = sim_join(CH - rightH - (sH[tid] - h), CL - rightL - (sL[tid] - l));
        const bool counts = st != 2;
        const double prec = counts ? (double)cum / (double)(cum + cumF) : 0.0;
        const double os = counts ? cumSim / (double)(cum + cumF) : 0.0;
        mP[tid] = prec; mO[tid] = os;
        fv[tid] = counts ? (2.0 * (double)cum) / (double)((long long)cum + cumF + G) : -1.0;
        fk[tid] = k;
        __syncthreads();
        for (int o = 1; o < kScan; o <<= 1) {                  // inclusive suffix maxima
            const bool in = tid + o < kScan;
            const double uP = in ? mP[tid + o] : 0.0, uO = in ? mO[tid + o] : 0.0;
            __syncthreads();
            mP[tid] = fmax(mP[tid], uP); mO[tid] = fmax(mO[tid], uO);
            __syncthreads();
        }
        const double env = fmax(mP[tid], envP_right), envO = fmax(mO[tid], envO_right);
        if (flag) {
            accP += ((double)cum / (double)G - (double)(cum - 1) / (double)G) * env;
            accO += ((double)cum / (double)G - (double)(cum - 1) / (double)G) * envO;
        }
        if (out_curve && k < N) {
            double* o = out_curve + ((size_t)t * N + k) * 3;
            o[0] = counts ? (double)cum / (double)G : nan("");
            o[1] = counts ? prec : nan("");
            o[2] = counts ? os : nan("");
        }
        for (int o = kScan / 2; o > 0; o >>= 1) {              // the largest F1 of the chunk, the lowest rank among equals
            if (tid < o) {
                const double a = fv[tid], b = fv[tid + o];
                if (b > a || (b == a && fk[tid + o] < fk[tid])) { fv[tid] = b; fk[tid] = fk[tid + o]; }
            }
            __syncthreads();
        }
        if (fv[0] >= 0.0 && fv[0] >= best_f1) { best_f1 = fv[0]; best_k = fk[0]; }   // this chunk lies to the left: it wins ties
        rightT += cT[0]; rightF += cF[0]; rightH += sH[0]; rightL += sL[0];
        envP_right = fmax(envP_right, mP[0]);
        envO_right = fmax(envO_right, mO[0]);
    }
    __syncthreads();
    mP[tid] = accP; mO[tid] = accO;
    __syncthreads();
    for (int o = kScan / 2; o > 0; o >>= 1) {                  // fixed tree
        if (tid < o) { mP[tid] += mP[tid + o]; mO[tid] += mO[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        double* w = out + (size_t)t * kWords;
        const double none = nan("");
        w[0] = mP[0];
        w[1] = mO[0];
        w[2] = n_rows > 0 ? sum_dist / (double)n_rows : none;
        w[3] = n_rows > 0 ? sum_scale / (double)n_rows : none;
        w[4] = n_rows > 0 ? sum_yaw / (double)n_rows : none;
        w[5] = best_f1 >= 0.0 ? best_f1 : 0.0;
        const long long r = CT > 0 && best_k >= 0 ? row_at(best_k) : -1;
        w[6] = r >= 0 ? scores[r] : none;
    }
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_boxes_evaluate_workspace_bytes(int n_samples, int total_pred, long long total_pairs, int n_thresholds) {
    if (!sizes_ok(n_samples, total_pred, total_pairs, n_thresholds)) return 0;
    return MatchWs(nullptr, n_samples, total_pairs).bytes;
}

extern "C" int lisec_boxes_evaluate(const double* pred_boxes, const double* pred_scores, const int32_t* pred_start,
                                    const uint8_t* pred_ignore, const double* label_boxes, const int32_t* label_start,
                                    const uint8_t* label_ignore, int n_samples, int total_pred, long long total_pairs,
                                    const double* thresholds, int n_thresholds, int mode, void* workspace, size_t workspace_bytes,
                                    double* best_iou, int32_t* best_label, double* ignored_iou, double* geom, uint8_t* state,
                                    int32_t* tp_count, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxThresholds && thresholds,
                    "boxes_evaluate takes 1 to %d IoU thresholds", kMaxThresholds);
    Thresholds thr;
    thr.n = n_thresholds;
    for (int t = 0; t < kMaxThresholds; ++t) thr.t[t] = t < n_thresholds ? thresholds[t] : 0.0;
    for (int t = 0; t < n_thresholds; ++t)
        LISEC_CHECK_ARG(thr.t[t] >= 0.0 && thr.t[t] < 1.0, "IoU threshold %d = %g is outside [0, 1)", t, thr.t[t]);
    LISEC_CHECK_ARG(mode == LISEC_IOU_3D || mode == LISEC_IOU_BEV, "unknown IoU mode %d", mode);
    LISEC_CHECK_ARG(best_iou && best_label && ignored_iou && geom && state && tp_count, "boxes_evaluate: an output is NULL");
    LISEC_CHECK_ARG(sizes_ok(n_samples, total_pred, total_pairs, n_thresholds) && pred_start && label_start && workspace &&
                    (total_pred == 0 || (pred_boxes && pred_scores)) && (total_pairs == 0 || label_boxes), "bad arguments");
    LISEC_CHECK_ARG(aligned(pred_boxes, 8) && aligned(pred_scores, 8) && aligned(label_boxes, 8) && aligned(best_iou, 8) &&
                    aligned(ignored_iou, 8) && aligned(geom, 8) && aligned(workspace, 8) && aligned(pred_start, 4) &&
                    aligned(label_start, 4) && aligned(best_label, 4) && aligned(tp_count, 4),
                    "boxes_evaluate: a buffer is misaligned for its element type");
    MatchWs ws(workspace, n_samples, total_pairs);
    LISEC_CHECK_ARG(workspace_bytes >= ws.bytes, "boxes_evaluate workspace too small: %zu bytes given, %zu needed",
                    workspace_bytes, ws.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (int rc = launch_pair_iou(pred_boxes, pred_start, label_boxes, label_start, n_samples, total_pred, total_pairs,
                                 n_thresholds, mode, ws.pair_off, ws.ok, ws.iou, tp_count, st))
        return rc;
    if (total_pred > 0) {
        LISEC_LAUNCH(k_eval_candidates, dim3(cdiv(total_pred, kThreads)), dim3(kThreads), 0, st, pred_boxes, pred_start,
                     label_boxes, label_start, label_ignore, n_samples, total_pred, ws.pair_off, ws.ok, ws.iou, best_iou,
                     best_label, ignored_iou, geom);
        LISEC_LAUNCH(k_eval_state, dim3(cdiv(total_pred, kThreads)), dim3(kThreads), 0, st, pred_scores, pred_start, pred_ignore,
                     n_samples, total_pred, thr, ws.ok, best_iou, best_label, ignored_iou, state, tp_count);
    }
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_boxes_evaluate_integrate(const int64_t* rank, const uint8_t* state, const double* geom, const double* scores,
                                              int n_pred, int n_labels, int n_thresholds, double* out, double* out_curve,
                                              lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n_labels > 0, "the evaluation needs at least one label that is not ignored (G = %d)", n_labels);
    LISEC_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxThresholds, "boxes_evaluate_integrate takes 1 to %d IoU thresholds",
                    kMaxThresholds);
    LISEC_CHECK_ARG(n_pred >= 0 && out && (n_pred == 0 || (rank && state && geom && scores)), "bad arguments");
    LISEC_CHECK_ARG(aligned(rank, 8) && aligned(geom, 8) && aligned(scores, 8) && aligned(out, 8) && aligned(out_curve, 8),
                    "boxes_evaluate_integrate: a buffer is misaligned for its element type");
    LISEC_LAUNCH(k_eval_integrate, dim3(n_thresholds), dim3(kScan), 0, static_cast<hipStream_t>(stream_), rank, state, geom,
                 scores, n_pred, n_labels, out, out_curve);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
