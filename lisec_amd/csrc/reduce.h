// The three ordered sums behind every deterministic scalar of the loss, metric and update passes (device only).
// A sum here is a fixed sequence of additions: which values meet in which add is decided by the launch geometry and, for
// order V, by the chunk table -- never by arrival order, and there is no atomic.  So the result has the same bits on every
// run, in a replayed plan and after a resume, and an evaluation entry that keeps the training entry's partition
// reproduces its values bit for bit.  loss_out, the evaluation accumulators, the metric pairs, the positive / negative
// counts, the penalty, the trust ratios and the clip scales and norms are all outputs of these orders: changing one
// changes their last bits.  A new pass picks one of the three; it does not write a fourth.
//
//   order W  (a workgroup of THREADS, W = THREADS / 64 waves)  the butterfly of wave_sum in each wave, lane 0 of wave w
//            stores to red[k][w], a barrier, then ONE thread adds red[k][0], ..., red[k][W-1] in that order to 0.
//   order T  (one workgroup of THREADS over a table of nparts rows)  thread t adds rows t, t + THREADS, ... in that order
//            to 0 (strided_sums), then a halving tree over the THREADS sums: for o = THREADS/2, ..., 1 thread t < o adds
//            red[k][t + o] to red[k][t] (tree_sums).
//   order V  (one wave per variable of a chunk table)  lane l adds rows first + l, first + l + 64, ... in that order to 0,
//            then the butterfly of wave_sum (wave_strided_sums).
//
// Every helper takes N values at once (a row of a table holds them interleaved: row p, value k at [p * N + k]) and a
// predicate used(k), uniform over the workgroup: a slot it rejects costs no shuffle, no LDS traffic and no load, and its
// result is undefined.  The LDS array is the caller's: this header declares no __shared__ object.  It holds additions,
// shuffles, LDS traffic and barriers only -- no multiply to contract -- so it reads the same under either setting of
// `#pragma clang fp contract`, and it does not touch the includer's.
#pragma once
#include "common.h"

namespace lisec {

struct EverySlot {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// ---- order W -----------------------------------------------------------------------------------------------------------
// The first half, shared by both forms: butterflies, lane 0's stores, the barrier.
template <int THREADS, int N, typename T, typename Used>
__device__ __forceinline__ void wave_partials(const T (&v)[N], T (&red)[N][THREADS / kWave], Used used) {
    T s[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (used(k)) s[k] = wave_sum(v[k]);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (used(k)) red[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
}
template <int W, typename T>
__device__ __forceinline__ T wave_order_total(const T (&row)[W]) {
    T a = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) a += row[w];
    return a;
}

// Form "own": thread k < N with used(k) returns sum k (the loss kernels: thread k stores partial k); any other thread
// returns 0.  Form "all": thread 0 gets every used sum in out[] (a site that combines them: l1*t1 + l2*t2).  The two
// give the same bits: each is the same ascending adds.
// Both return without a trailing barrier.  A caller that comes back with the same `red` -- a chunk loop -- owns the
// __syncthreads() between the two calls: the reading thread may still be adding while the other waves run ahead.
template <int THREADS, int N, typename T, typename Used = EverySlot>
__device__ __forceinline__ T block_sum_own(const T (&v)[N], T (&red)[N][THREADS / kWave], Used used = Used()) {
    wave_partials<THREADS>(v, red, used);
    return threadIdx.x < N && used(threadIdx.x) ? wave_order_total(red[threadIdx.x]) : T(0);
}
template <int THREADS, int N, typename T, typename Used = EverySlot>
__device__ __forceinline__ void block_sums_all(const T (&v)[N], T (&red)[N][THREADS / kWave], T (&out)[N],
                                               Used used = Used()) {
    wave_partials<THREADS>(v, red, used);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (used(k)) out[k] = wave_order_total(red[k]);
}

// ---- order T -----------------------------------------------------------------------------------------------------------
// a[k] = rows t, t + THREADS, ... of value k, for the calling thread t; the loads of a row's used values issue together.
template <int THREADS, int N, typename Used = EverySlot>
__device__ __forceinline__ void strided_sums(const double* __restrict__ parts, int nparts, double (&a)[N],
                                             Used used = Used()) {
    double s[N];                 // locals, copied out at the end: summed through the reference, the loop compiles larger
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int p = threadIdx.x; p < nparts; p += THREADS) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (used(k)) s[k] += parts[(size_t)p * N + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = s[k];
}
// The tree over one value per thread and slot.  On return red[k][0] holds sum k and every thread may read it (the last
// barrier of the tree is behind the last add).  A caller that reuses `red` owns the barrier in front of the next call.
template <int THREADS, int N, typename Used = EverySlot>
__device__ __forceinline__ void tree_sums(const double (&a)[N], double (&red)[N][THREADS], Used used = Used()) {
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (used(k)) red[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (used(k)) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// ---- order V -----------------------------------------------------------------------------------------------------------
// One wave (a workgroup of 64): s[k] = the sum of value k over rows first, ..., first + count - 1, in every lane.  No LDS
// and no barrier: a loop over variables calls it back to back.
template <int N>
__device__ __forceinline__ void wave_strided_sums(const double* __restrict__ parts, long long first, int count,
                                                  double (&s)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < count; i += kWave) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += parts[(first + i) * N + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = wave_sum(s[k]);
}

}  // namespace lisec
