// What the two matchers (detection_ap.hip, detection_eval.hip) share: the sample-major layout's pair offsets with the
// consistency word, the IoU of every pair, the owner search and the workspace both carve.  Internal linkage: each file
// compiles its own copy of the two kernels from this one text.
#pragma once
#include "box_geom.h"

namespace lisec {
namespace {

constexpr int kThreads = 256;
constexpr int kScan = 1024;
constexpr int kMaxThresholds = 16;
constexpr long long kMaxPairGrid = 1 << 20;                    // workgroups of the pair kernel; beyond, each strides on

struct Thresholds {
    double t[kMaxThresholds];
    int n;
};

struct MatchWs {
    double* iou;                                               // [total_pairs] sample after sample, rows = predictions
    long long* pair_off;                                       // [n_samples + 1] first pair of each sample
    int* ok;                                                   // 1 when the offset tables agree with the sizes given
    size_t bytes;
    MatchWs(void* base, int n_samples, long long total_pairs) {
        Carver c(base);
        iou = c.take<double>((size_t)total_pairs);
        pair_off = c.take<long long>((size_t)n_samples + 1);
        ok = c.take<int>(4);
        bytes = c.off;
    }
};

// the last s in [0, n) with start[s] <= q (start ascending, start[0] <= q): the sample that owns row / pair q
template <typename T>
__device__ __forceinline__ int owner(const T* __restrict__ start, int n, long long q) {
    int lo = 0, hi = n;                                        // start[lo] <= q < start[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)start[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// pair_off = exclusive scan of n_pred * n_label over the samples (one workgroup, chunks of kScan), and the consistency word:
// every later kernel trusts the offsets only when they agree with the sizes the host sized the buffers by.  tp_count = 0 then,
// -1 otherwise (with best_iou = NaN, best_label = -1, tp = 0: nothing that could pass for a result).
__global__ void __launch_bounds__(kScan)
k_pair_offsets(const int32_t* __restrict__ pred_start, const int32_t* __restrict__ label_start, int n_samples, int total_pred,
               long long total_pairs, int n_thresholds, long long* __restrict__ pair_off, int* __restrict__ ok,
               int32_t* __restrict__ tp_count) {
    __shared__ long long scan[kScan];
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = pred_start[0] != 0 || pred_start[n_samples] != total_pred;
    long long carry = 0;
    for (int base = 0; base < n_samples; base += kScan) {
        const int s = base + tid;
        long long v = 0;
        bool neg = false;
        if (s < n_samples) {
            const long long nP = (long long)pred_start[s + 1] - pred_start[s], nL = (long long)label_start[s + 1] - label_start[s];
            neg = nP < 0 || nL < 0;
            v = neg ? 0 : nP * nL;
        }
        __syncthreads();
        if (neg) bad = 1;
        scan[tid] = v;
        __syncthreads();
        for (int o = 1; o < kScan; o <<= 1) {
            const long long u = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += u;
            __syncthreads();
        }
        if (s < n_samples) pair_off[s] = carry + scan[tid] - v;
        carry += scan[kScan - 1];
    }
    __syncthreads();
    const int fine = !bad && carry == total_pairs;
    if (tid == 0) {
        pair_off[n_samples] = carry;
        *ok = fine;
    }
    for (long long k = tid; k < (long long)n_samples * n_thresholds; k += kScan) tp_count[k] = fine ? 0 : -1;
}

__global__ void __launch_bounds__(kThreads)
k_pair_iou(const double* __restrict__ pred, const int32_t* __restrict__ pred_start, const double* __restrict__ label,
           const int32_t* __restrict__ label_start, int n_samples, long long total_pairs, int mode,
           const long long* __restrict__ pair_off, const int* __restrict__ ok, double* __restrict__ iou) {
    const bool fine = *ok != 0;
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < total_pairs; q += (long long)gridDim.x * kThreads) {
        if (!fine) { iou[q] = nan(""); continue; }
        const int s = owner(pair_off, n_samples, q);
        const long long r = q - pair_off[s];
        const int l0 = label_start[s], nL = label_start[s + 1] - l0;
        const int i = (int)(r / nL), j = (int)(r - (long long)i * nL);
        iou[q] = pair_iou(pred + (size_t)(pred_start[s] + i) * 7, label + (size_t)(l0 + j) * 7, mode);
    }
}

bool sizes_ok(int n_samples, int total_pred, long long total_pairs, int n_thresholds) {
    return n_samples >= 0 && total_pred >= 0 && total_pairs >= 0 && n_thresholds >= 1 && n_thresholds <= kMaxThresholds;
}

// pair_off and the consistency word, then the IoU of every pair into iou[total_pairs]; tp_count may be NULL with
// n_thresholds == 0.  A launch that fails is reported at once, before anything reads what it should have written.
int launch_pair_iou(const double* pred_boxes, const int32_t* pred_start, const double* label_boxes, const int32_t* label_start,
                    int n_samples, int total_pred, long long total_pairs, int n_thresholds, int mode, long long* pair_off, int* ok,
                    double* iou, int32_t* tp_count, hipStream_t st) {
    LISEC_LAUNCH(k_pair_offsets, dim3(1), dim3(kScan), 0, st, pred_start, label_start, n_samples, total_pred, total_pairs,
                 n_thresholds, pair_off, ok, tp_count);
    LISEC_LAUNCH_CHECK();
    if (total_pairs > 0) {
        const long long groups = (total_pairs + kThreads - 1) / kThreads;
        LISEC_LAUNCH(k_pair_iou, dim3((unsigned)(groups < kMaxPairGrid ? groups : kMaxPairGrid)), dim3(kThreads), 0, st, pred_boxes,
                     pred_start, label_boxes, label_start, n_samples, total_pairs, mode, pair_off, ok, iou);
        LISEC_LAUNCH_CHECK();
    }
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec
