// tf.keras 2.4 losses and metrics of Model.compile(loss=, loss_weights=, metrics=) on the (M,16) head
// (include/lisec_hip.h, lisec_head_loss*).  One pass over head / y_cls / y_reg in the element layout of k_loss
// (csrc/eltwise.hip): thread i of the grid-stride loop holds element i of the flat (M,16) head, so the 16 lanes of a
// cell are 16 consecutive lanes of one wave and a per-cell metric (categorical accuracy) is a butterfly over them.
// It writes dhead and per-workgroup fp64 partials of both losses and of every metric (order W of reduce.h); one
// single-workgroup finalize sums them (order T).  The evaluation entry is the same kernels with a NULL gradient, so it
// reproduces the training entry's values bit for bit.
//
// Values: MSE and the two halves of lisec_rpn_loss kind 1 use k_loss's fp32 element arithmetic (so dhead of
// ['mse','mse'] at unit weights is k_loss's, bit for bit); every other kind evaluates its element loss and gradient in
// double from the fp32 inputs, then rounds the gradient once.  Sums are fp64 in both cases.
#include "reduce.h"
#include "sample_weights.h"

namespace lisec {
namespace {

constexpr int kLossThreads = 256;                            // 16 cells of 16 lanes per wave-quad
constexpr int kLossBlocks = 1024;
constexpr int kLossVals = 2 + 2 * LISEC_LOSS_MAX_METRICS;   // partials per workgroup: L_cls, L_reg, metrics [out][j]
constexpr int kLossValsW = kLossVals + 4;                     // weighted: + sum of w over elements [out], over cells [out]
constexpr double kEps = 1e-7;                                // K.epsilon()

// Value slot k of the partials is in use: the two losses, and metric j of output o while j < n_metrics[o].
__device__ __forceinline__ bool slot_used(const lisec_loss_cfg& cfg, int k) {
    if (k < 2) return true;
    const int o = (k - 2) / LISEC_LOSS_MAX_METRICS, j = (k - 2) % LISEC_LOSS_MAX_METRICS;
    return j < cfg.n_metrics[o];
}

// The weighted partials: the four sums of weights are always in use.
__device__ __forceinline__ bool slot_used_w(const lisec_loss_cfg& cfg, int k) { return k >= kLossVals || slot_used(cfg, k); }

__device__ __forceinline__ double dsign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }
__device__ __forceinline__ double softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }

// Element value of term T at (p, t); with `grad`, also g = the scaled gradient: wf (fp32) for the fp32-arithmetic kinds,
// wd (fp64) for the others -- both are grad_scale * weight / (M*C).
__device__ __forceinline__ double term(const lisec_loss_term& T, float p, float t, bool grad, float wf, double wd,
                                       float& g) {
    const double pd = p, td = t, e = pd - td;
    double v = 0.0, gd = 0.0;
    switch (T.kind) {
    case LISEC_LOSS_MSE: {
        const float d = p - t;                                           // k_loss kind 0
        if (grad) g = 2.f * d * wf;
        return (double)d * d;
    }
    case LISEC_LOSS_SIGMOID_CE_CLAMPED: {                                // k_loss kind 1, class half
        const float tt = fminf(fmaxf(t, 0.f), 1.f);
        if (grad) g = (1.f / (1.f + expf(-p)) - tt) * wf;
        return (double)(fmaxf(p, 0.f) - p * tt + log1pf(expf(-fabsf(p))));
    }
    case LISEC_LOSS_SMOOTH_L1: {                                         // k_loss kind 1, regression half
        const float d = p - t;
        const float ad = fabsf(d);
        if (grad) g = (ad < 1.f ? d : (d > 0.f ? 1.f : -1.f)) * wf;
        return (double)(ad < 1.f ? 0.5f * d * d : ad - 0.5f);
    }
    case LISEC_LOSS_MAE:
        v = fabs(e);
        gd = dsign(e);
        break;
    case LISEC_LOSS_MAPE: {
        const double den = fmax(fabs(td), kEps);
        v = 100.0 * fabs((td - pd) / den);
        gd = -100.0 * dsign(td - pd) / den;
        break;
    }
    case LISEC_LOSS_MSLE: {
        const double a = fmax(pd, kEps), diff = log1p(a) - log1p(fmax(td, kEps));
        v = diff * diff;
        gd = pd >= kEps ? 2.0 * diff / (a + 1.0) : 0.0;                 // Maximum: the gradient goes to x where x >= y
        break;
    }
    case LISEC_LOSS_HUBER: {
        const double delta = T.param, ae = fabs(e);
        v = ae <= delta ? 0.5 * e * e : 0.5 * delta * delta + delta * (ae - delta);
        gd = ae <= delta ? e : delta * dsign(e);
        break;
    }
    case LISEC_LOSS_LOGCOSH:
        v = e + softplus(-2.0 * e) - 0.69314718055994530942;
        gd = tanh(e);
        break;
    case LISEC_LOSS_BCE: {
        const double ls = T.label_smoothing, ts = td * (1.0 - ls) + 0.5 * ls;
        if (T.from_logits) {
            // nn.sigmoid_cross_entropy_with_logits: where(p >= 0, p, 0) - p*t + log1p(exp(where(p >= 0, -p, p)))
            v = fmax(pd, 0.0) - pd * ts + log1p(exp(-fabs(pd)));
            gd = 1.0 / (1.0 + exp(-pd)) - ts;
        } else {
            const double o = fmin(fmax(pd, kEps), 1.0 - kEps);
            v = -(ts * log(o + kEps) + (1.0 - ts) * log(1.0 - o + kEps));
            gd = (pd >= kEps && pd <= 1.0 - kEps) ? -(ts / (o + kEps) - (1.0 - ts) / (1.0 - o + kEps)) : 0.0;
        }
        break;
    }
    case LISEC_LOSS_POISSON:
        v = pd - td * log(pd + kEps);
        gd = 1.0 - td / (pd + kEps);
        break;
    case LISEC_METRIC_BINARY_ACCURACY:
        return t == (p > T.param ? 1.f : 0.f) ? 1.0 : 0.0;
    default:
        break;
    }
    if (grad) g = (float)(gd * wd);
    return v;
}

// argmax over the lanes of this lane's 16-lane cell group for which `in` holds (every lane of the group calls it);
// the first index wins ties
__device__ __forceinline__ int group_argmax(float x, int c, bool in) {
    float v = in ? x : -INFINITY;
    int k = in ? c : 16 + c;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int k2 = __shfl_xor(k, o, 64);
        if (v2 > v || (v2 == v && k2 < k)) { v = v2; k = k2; }
    }
    return k;
}

// dhead == nullptr: values only (the evaluation entry).  The grid-stride loop runs the same trip count on every lane of
// a workgroup, so the butterflies of the categorical metric see whole cell groups.
// WEIGHTED (one CellWeights behind parts; sample_weights.h): cell m of output o carries the factor w = cell_weight(...):
// the gradient scale is wf * w (one fp32 multiply) or wd * (double)w, the loss sum adds (double)w * v, a weighted metric
// adds (double)w * v to its sum, and the sums of w over the elements and over the cells of each output leave as four more
// partials.  w == 1.0f is every product by one: the bits of the unweighted instantiation, whose code is what it was.
template <bool WEIGHTED, typename... W>
__global__ void __launch_bounds__(kLossThreads)
k_head_loss(lisec_loss_cfg cfg, const float* __restrict__ head, const float* __restrict__ ycls,
            const float* __restrict__ yreg, long long M, float gscale, float* __restrict__ dhead, double* __restrict__ parts,
            W... cw_) {
    constexpr int NV = WEIGHTED ? kLossValsW : kLossVals;
    [[maybe_unused]] const CellWeights cw = the_weights(cw_...);
    __shared__ double red[NV][kLossThreads / 64];
    const int c = threadIdx.x & 15, o = c < 2 ? 0 : 1;
    const lisec_loss_term L = cfg.loss[o];
    const int nmet = cfg.n_metrics[o];
    const long long C = o ? 14 : 2;
    const float wf = gscale * cfg.weight[o] / (float)(M * C);
    const double wd = (double)gscale * (double)cfg.weight[o] / (double)(M * C);
    const bool grad = dhead != nullptr;
    bool cat = false;
    for (int j = 0; j < cfg.n_metrics[0]; ++j) cat |= cfg.metric[0][j].kind == LISEC_METRIC_CATEGORICAL_ACCURACY;
    for (int j = 0; j < cfg.n_metrics[1]; ++j) cat |= cfg.metric[1][j].kind == LISEC_METRIC_CATEGORICAL_ACCURACY;
    double lacc = 0.0, macc[LISEC_LOSS_MAX_METRICS];
#pragma unroll
    for (int j = 0; j < LISEC_LOSS_MAX_METRICS; ++j) macc[j] = 0.0;
    [[maybe_unused]] SweepWeights sws = {};
    [[maybe_unused]] unsigned wmask = 0u;
    [[maybe_unused]] double dene = 0.0, denc = 0.0;
    if constexpr (WEIGHTED) {
        sws = sweep_weights(cw);
        wmask = o ? cw.metrics[1] : cw.metrics[0];
    }
    const long long n = M * 16;
    for (long long base = blockIdx.x * (long long)kLossThreads; base < n; base += (long long)gridDim.x * kLossThreads) {
        const long long i = base + threadIdx.x, m = i >> 4;
        const bool valid = i < n;                   // whole cell groups are valid or not (n is a multiple of 16)
        float p = 0.f, t = 0.f;
        [[maybe_unused]] float w = 1.f;
        if (valid) {
            p = head[i];
            t = o ? yreg[m * 14 + (c - 2)] : ycls[m * 2 + c];
            if constexpr (WEIGHTED) w = cell_weight(cw, sws, o, m);
        }
        if (cat) {                                  // uniform branch: every lane takes part in the butterflies
            const int ap = group_argmax(p, c, c >= 2), at = group_argmax(t, c, c >= 2);
            const int bp = group_argmax(p, c, c < 2), bt = group_argmax(t, c, c < 2);
            const double hit = (c == 0 && bp == bt) || (c == 2 && ap == at) ? 1.0 : 0.0;
#pragma unroll
            for (int j = 0; j < LISEC_LOSS_MAX_METRICS; ++j)
                if (valid && j < nmet && cfg.metric[o][j].kind == LISEC_METRIC_CATEGORICAL_ACCURACY) {
                    if constexpr (WEIGHTED) macc[j] += (wmask >> j & 1u) ? (double)w * hit : hit;
                    else macc[j] += hit;
                }
        }
        if (!valid) continue;
        float g = 0.f;
        if constexpr (WEIGHTED) {
            lacc += (double)w * term(L, p, t, grad, wf * w, wd * (double)w, g);
            dene += (double)w;
            if (c == 0 || c == 2) denc += (double)w;            // the lane of a cell that holds its categorical hit
        } else {
            lacc += term(L, p, t, grad, wf, wd, g);
        }
        if (grad) dhead[i] = g;
#pragma unroll
        for (int j = 0; j < LISEC_LOSS_MAX_METRICS; ++j) {
            if (j < nmet && cfg.metric[o][j].kind != LISEC_METRIC_CATEGORICAL_ACCURACY) {
                float unused;
                if constexpr (WEIGHTED) {
                    const double mv = term(cfg.metric[o][j], p, t, false, 0.f, 0.0, unused);
                    macc[j] += (wmask >> j & 1u) ? (double)w * mv : mv;
                } else {
                    macc[j] += term(cfg.metric[o][j], p, t, false, 0.f, 0.0, unused);
                }
            }
        }
    }
    double v[NV];
    v[0] = o == 0 ? lacc : 0.0;
    v[1] = o == 1 ? lacc : 0.0;
#pragma unroll
    for (int j = 0; j < LISEC_LOSS_MAX_METRICS; ++j) {
        v[2 + j] = o == 0 ? macc[j] : 0.0;
        v[2 + LISEC_LOSS_MAX_METRICS + j] = o == 1 ? macc[j] : 0.0;
    }
    if constexpr (WEIGHTED) {
        v[kLossVals + 0] = o == 0 ? dene : 0.0;
        v[kLossVals + 1] = o == 1 ? dene : 0.0;
        v[kLossVals + 2] = o == 0 ? denc : 0.0;
        v[kLossVals + 3] = o == 1 ? denc : 0.0;
    }
    // uniform: the unused slots are never read
    const auto used = [&](int k) { return WEIGHTED ? slot_used_w(cfg, k) : slot_used(cfg, k); };
    const double a = block_sum_own<kLossThreads>(v, red, used);
    if (threadIdx.x < NV && used(threadIdx.x)) parts[(size_t)blockIdx.x * NV + threadIdx.x] = a;
}

// One workgroup: the partials of every value in use, in order T.  Training (acc == nullptr): loss_out[3] and
// metric_out; evaluation: the same fp32 values added, as doubles, to acc, and the sweep counted.
__global__ void __launch_bounds__(256)
k_head_loss_finalize(lisec_loss_cfg cfg, const double* __restrict__ parts, int nparts, double M, float* __restrict__ loss_out,
                     float* __restrict__ metric_out, double* __restrict__ acc) {
    __shared__ double red[kLossVals][256];
    const auto used = [&](int k) { return slot_used(cfg, k); };
    double a[kLossVals];
    strided_sums<256>(parts, nparts, a, used);
    tree_sums<256>(a, red, used);
    if (threadIdx.x != 0) return;
    const double lc = red[0][0] / (M * 2.0), lr = red[1][0] / (M * 14.0);
    const float tot = (float)((double)cfg.weight[0] * lc + (double)cfg.weight[1] * lr), fc = (float)lc, fr = (float)lr;
    if (acc) {
        acc[0] += (double)tot; acc[1] += (double)fc; acc[2] += (double)fr;
    } else {
        loss_out[0] = tot; loss_out[1] = fc; loss_out[2] = fr;
    }
    int k = 0;
    for (int o = 0; o < 2; ++o) {
        for (int j = 0; j < cfg.n_metrics[o]; ++j, ++k) {
            const double cells = cfg.metric[o][j].kind == LISEC_METRIC_CATEGORICAL_ACCURACY ? M : M * (o ? 14.0 : 2.0);
            const float val = (float)(red[2 + o * LISEC_LOSS_MAX_METRICS + j][0] / cells);
            if (acc) acc[3 + k] += (double)val;
            else metric_out[k] = val;
        }
    }
    if (acc) acc[3 + k] += 1.0;
}

// The weighted form.  The losses are those of k_head_loss_finalize; every metric leaves as the fp64 pair {num, den}: den
// is the sum of w over the output's elements (cells, for the categorical accuracy) where the metric is weighted, the
// element or cell count where it is not.  Training (acc == nullptr): loss_out[3] and pairs_out[2k], [2k + 1];
// evaluation: acc = {total, class, regression, sweeps, num0, den0, ...}, the fp32 losses and the pairs added.
__global__ void __launch_bounds__(256)
k_head_loss_finalize_w(lisec_loss_cfg cfg, CellWeights cw, const double* __restrict__ parts, int nparts, double M,
                       float* __restrict__ loss_out, double* __restrict__ pairs_out, double* __restrict__ acc) {
    __shared__ double red[kLossValsW][256];
    const auto used = [&](int k) { return slot_used_w(cfg, k); };
    double a[kLossValsW];
    strided_sums<256>(parts, nparts, a, used);
    tree_sums<256>(a, red, used);
    if (threadIdx.x != 0) return;
    const double lc = red[0][0] / (M * 2.0), lr = red[1][0] / (M * 14.0);
    const float tot = (float)((double)cfg.weight[0] * lc + (double)cfg.weight[1] * lr), fc = (float)lc, fr = (float)lr;
    if (acc) {
        acc[0] += (double)tot; acc[1] += (double)fc; acc[2] += (double)fr; acc[3] += 1.0;
    } else {
        loss_out[0] = tot; loss_out[1] = fc; loss_out[2] = fr;
    }
    int k = 0;
    for (int o = 0; o < 2; ++o) {
        for (int j = 0; j < cfg.n_metrics[o]; ++j, ++k) {
            const bool percell = cfg.metric[o][j].kind == LISEC_METRIC_CATEGORICAL_ACCURACY;
            const double num = red[2 + o * LISEC_LOSS_MAX_METRICS + j][0];
            const double den = (cw.metrics[o] >> j & 1u) ? red[kLossVals + (percell ? 2 : 0) + o][0]
                                                         : (percell ? M : M * (o ? 14.0 : 2.0));
            if (acc) {
                acc[4 + 2 * k] += num; acc[5 + 2 * k] += den;
            } else {
                pairs_out[2 * k] = num; pairs_out[2 * k + 1] = den;
            }
        }
    }
}

bool valid_term(const lisec_loss_term& T, bool metric) {
    if (T.kind < 0 || T.kind > (metric ? LISEC_METRIC_CATEGORICAL_ACCURACY : LISEC_LOSS_SMOOTH_L1)) return false;
    if (T.kind == LISEC_LOSS_HUBER && !(T.param > 0.f)) return false;
    if (T.kind == LISEC_LOSS_BCE && !(T.label_smoothing >= 0.f && T.label_smoothing <= 1.f)) return false;
    return true;
}

int check_cfg(const lisec_loss_cfg* cfg) {
    LISEC_CHECK_ARG(cfg, "NULL loss descriptor");
    for (int o = 0; o < 2; ++o) {
        LISEC_CHECK_ARG(valid_term(cfg->loss[o], false), "head loss: bad loss kind or parameter for output %d", o);
        LISEC_CHECK_ARG(cfg->n_metrics[o] >= 0 && cfg->n_metrics[o] <= LISEC_LOSS_MAX_METRICS,
                        "head loss: 0 to %d metrics per output", LISEC_LOSS_MAX_METRICS);
        for (int j = 0; j < cfg->n_metrics[o]; ++j)
            LISEC_CHECK_ARG(valid_term(cfg->metric[o][j], true), "head loss: bad metric kind or parameter (output %d, #%d)",
                            o, j);
    }
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_head_loss_workspace_bytes(void) {
    return align_up(sizeof(double) * (size_t)kLossBlocks * kLossVals, 256);
}

extern "C" int lisec_head_loss(const lisec_loss_cfg* cfg, const float* head, const float* y_cls, const float* y_reg,
                               long long M, float grad_scale, float* dhead, float* loss_out, float* metric_out,
                               void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_cfg(cfg)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && workspace && M > 0, "NULL pointer");
    LISEC_CHECK_ARG(metric_out || cfg->n_metrics[0] + cfg->n_metrics[1] == 0, "NULL metric_out with metrics");
    if (workspace_bytes < lisec_head_loss_workspace_bytes()) {
        set_error("head loss workspace too small");
        return LISEC_ENOSPC;
    }
    hipStream_t st = static_cast<hipStream_t>(stream_);
    double* parts = static_cast<double*>(workspace);
    const int nb = grid_blocks(M * 16, kLossThreads, kLossBlocks);
    LISEC_LAUNCH(k_head_loss<false>, dim3(nb), dim3(kLossThreads), 0, st, *cfg, head, y_cls, y_reg, M, grad_scale, dhead, parts);
    LISEC_LAUNCH(k_head_loss_finalize, dim3(1), dim3(256), 0, st, *cfg, parts, nb, (double)M, loss_out, metric_out,
                 (double*)nullptr);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_head_loss_eval(const lisec_loss_cfg* cfg, const float* head, const float* y_cls, const float* y_reg,
                                    long long M, double* acc, void* workspace, size_t workspace_bytes,
                                    lisec_stream_t stream_) {
    if (int rc = check_cfg(cfg)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc && workspace && M > 0, "NULL pointer");
    if (workspace_bytes < lisec_head_loss_workspace_bytes()) {
        set_error("head loss workspace too small");
        return LISEC_ENOSPC;
    }
    hipStream_t st = static_cast<hipStream_t>(stream_);
    double* parts = static_cast<double*>(workspace);
    const int nb = grid_blocks(M * 16, kLossThreads, kLossBlocks);      // lisec_head_loss's partition: the same partials
    LISEC_LAUNCH(k_head_loss<false>, dim3(nb), dim3(kLossThreads), 0, st, *cfg, head, y_cls, y_reg, M, 1.0f, (float*)nullptr,
                 parts);
    LISEC_LAUNCH(k_head_loss_finalize, dim3(1), dim3(256), 0, st, *cfg, parts, nb, (double)M, (float*)nullptr,
                 (float*)nullptr, acc);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" size_t lisec_head_loss_weighted_workspace_bytes(void) {
    return align_up(sizeof(double) * (size_t)kLossBlocks * kLossValsW, 256);
}

namespace {
int run_head_weighted(const lisec_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head, const float* y_cls,
                      const float* y_reg, long long M, float grad_scale, float* dhead, float* loss_out, double* pairs_out,
                      double* acc, void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (workspace_bytes < lisec_head_loss_weighted_workspace_bytes()) {
        set_error("weighted head loss workspace too small");
        return LISEC_ENOSPC;
    }
    const CellWeights cw = cell_weights(*sw);
    double* parts = static_cast<double*>(workspace);
    const int nb = grid_blocks(M * 16, kLossThreads, kLossBlocks);      // lisec_head_loss's partition
    LISEC_LAUNCH(k_head_loss<true, CellWeights>, dim3(nb), dim3(kLossThreads), 0, st, *cfg, head, y_cls, y_reg, M,
                 grad_scale, dhead, parts, cw);
    LISEC_LAUNCH(k_head_loss_finalize_w, dim3(1), dim3(256), 0, st, *cfg, cw, parts, nb, (double)M, loss_out, pairs_out, acc);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
}  // namespace

extern "C" int lisec_head_loss_weighted(const lisec_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head,
                                        const float* y_cls, const float* y_reg, long long M, float grad_scale, float* dhead,
                                        float* loss_out, double* metric_pairs, void* workspace, size_t workspace_bytes,
                                        lisec_stream_t stream_) {
    if (int rc = check_cfg(cfg)) return rc;
    if (int rc = check_sample_weights(sw, cfg->n_metrics)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && workspace && M > 0, "NULL pointer");
    LISEC_CHECK_ARG(metric_pairs || cfg->n_metrics[0] + cfg->n_metrics[1] == 0, "NULL metric_pairs with metrics");
    return run_head_weighted(cfg, sw, head, y_cls, y_reg, M, grad_scale, dhead, loss_out, metric_pairs, nullptr, workspace,
                             workspace_bytes, static_cast<hipStream_t>(stream_));
}

extern "C" int lisec_head_loss_weighted_eval(const lisec_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head,
                                             const float* y_cls, const float* y_reg, long long M, double* acc,
                                             void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_cfg(cfg)) return rc;
    if (int rc = check_sample_weights(sw, cfg->n_metrics)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc && workspace && M > 0, "NULL pointer");
    return run_head_weighted(cfg, sw, head, y_cls, y_reg, M, 1.0f, nullptr, nullptr, nullptr, acc, workspace,
                             workspace_bytes, static_cast<hipStream_t>(stream_));
}
