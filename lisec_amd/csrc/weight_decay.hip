// Decoupled weight decay (optimizers.AdamW / SGDW / extend_with_decoupled_weight_decay; the order of
// tfa.optimizers.DecoupledWeightDecayExtension): one streaming pass over the flat parameter buffer theta IN FRONT of an
// optimizer entry, on the same range and the same stream -- the variable is decayed first, the optimizer then updates the
// decayed variable.  s = state[0] is the iteration count before the update, read from the device and never advanced (no
// ticket is taken: the update entry behind the pass owns the count):
//   wd_t = (float)schedule(s)      the coefficient descriptor (a lisec_lr_schedule in DEVICE memory, its `decay` 0), in
//                                  double by one thread per workgroup (schedule_value of optim_common.h), rounded once and
//                                  handed to the other waves through 4 bytes of LDS, the kernel's only LDS
//   wd_t == 0.0f:  every thread returns and theta keeps its bits ((-0) - (-0) would be +0, and the host cannot know s)
//   else           p = wd_t * w;  w <- w - p      for every element of every chunk: a multiply and a subtraction, each an
//                                  IEEE fp32 round-to-nearest-even operation of its own -- never an fma, never
//                                  w*(1 - wd_t); denormals are kept
// The host cuts every decayed variable into chunks (lisec_decay_chunk: the rules of lisec_reg_chunk) and only those are
// in the table: an excluded variable costs no traffic, and the floats outside every chunk keep their bits.  A launch in
// the shape of k_regularize: one workgroup of 256 per chunk, float4 loads and stores, every element touched by exactly
// one thread -- no atomics, the same bits from run to run; past kDecayBlocks chunks the workgroups stride over the
// table.  Per decayed float it reads 4 bytes and writes 4 and is bound by HBM alone.
#include "common.h"

// hipcc contracts a multiply into a following subtraction by default (-ffp-contract=fast): w - wd_t*w would become
// fma(-wd_t, w, w), one rounding short of the contract (csrc/weight_average.hip measured that 1 ulp).  So everything
// below is compiled with contraction off -- the schedule in double included, which is then the plain sequence of
// operations that lisec_amd/lr_schedules.py evaluates on the host.
#pragma clang fp contract(off)
#include "optim_common.h"

namespace lisec {
namespace {

constexpr int kDecayThreads = 256;
constexpr int kDecayBlocks = 2048;      // 8 workgroups of 256 per CU on 256 CUs; the model's theta is ~1600 chunks

__device__ __forceinline__ float decay_coefficient(const lisec_lr_schedule* __restrict__ coeff, long long s) {
    return (float)schedule_value(coeff, (double)s);
}

// IEEE fp32 round-to-nearest-even operations of their own (the contract in include/lisec_hip.h)
__device__ __forceinline__ float rn_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }

#define LISEC_DECAY_UPD(f) W.f = rn_sub(W.f, rn_mul(wd, W.f));

__global__ void __launch_bounds__(kDecayThreads)
k_weight_decay(float* __restrict__ theta, const lisec_decay_chunk* __restrict__ chunks, int n_chunks,
               const lisec_lr_schedule* __restrict__ coeff, const long long* __restrict__ state) {
    __shared__ float wd_shared;
    if (threadIdx.x == 0) wd_shared = decay_coefficient(coeff, read_iterations(state));
    __syncthreads();
    const float wd = wd_shared;
    if (wd == 0.0f) return;
    for (int c = blockIdx.x; c < n_chunks; c += kDecayBlocks) {         // (the grid is at most kDecayBlocks wide)
        const lisec_decay_chunk ch = chunks[c];
        float4* __restrict__ w4 = reinterpret_cast<float4*>(theta + ch.offset);
        const int n4 = ch.count / 4;
        for (int i = threadIdx.x; i < n4; i += kDecayThreads) {
            float4 W = w4[i];
            LISEC_DECAY_UPD(x) LISEC_DECAY_UPD(y) LISEC_DECAY_UPD(z) LISEC_DECAY_UPD(w)
            w4[i] = W;
        }
    }
}
#undef LISEC_DECAY_UPD

// wd_out[j] = wd_t at s = state[0] + j (lisec_weight_decay_eval): the device function of the pass, for tests.
__global__ void __launch_bounds__(kDecayThreads)
k_weight_decay_eval(const lisec_lr_schedule* __restrict__ coeff, const long long* __restrict__ state, long long k,
                    float* __restrict__ wd_out) {
    const long long s0 = read_iterations(state);
    for (long long j = blockIdx.x * (long long)kDecayThreads + threadIdx.x; j < k; j += (long long)gridDim.x * kDecayThreads)
        wd_out[j] = decay_coefficient(coeff, s0 + j);
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" int lisec_weight_decay(float* theta, const lisec_decay_chunk* chunks, int n_chunks, const lisec_lr_schedule* coeff,
                                  const long long* state, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && chunks && coeff && state, "weight_decay: NULL theta, chunks, coeff or state");
    LISEC_CHECK_ARG(n_chunks >= 0, "weight_decay: n_chunks = %d", n_chunks);
    LISEC_CHECK_ARG(aligned(theta, 16), "weight_decay: theta must be 16-byte aligned");
    LISEC_CHECK_ARG(aligned(state, 8), "weight_decay: state must be 8-byte aligned");
    if (n_chunks == 0) return LISEC_OK;
    LISEC_LAUNCH(k_weight_decay, dim3(grid_blocks(n_chunks, 1, kDecayBlocks)), dim3(kDecayThreads), 0,
                 static_cast<hipStream_t>(stream_), theta, chunks, n_chunks, coeff, state);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_weight_decay_eval(const lisec_lr_schedule* coeff, const long long* state, long long k, float* wd_out,
                                       lisec_stream_t stream_) {
    LISEC_CHECK_ARG(coeff && state && wd_out && k >= 0, "weight_decay_eval: NULL pointer or k < 0");
    LISEC_CHECK_ARG(aligned(state, 8), "weight_decay_eval: state must be 8-byte aligned");
    if (k == 0) return LISEC_OK;
    LISEC_LAUNCH(k_weight_decay_eval, dim3(grid_blocks(k, kDecayThreads, kDecayBlocks)), dim3(kDecayThreads), 0,
                 static_cast<hipStream_t>(stream_), coeff, state, k, wd_out);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
