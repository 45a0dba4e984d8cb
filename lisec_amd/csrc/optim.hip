// Optimizer updates of the flat parameter buffer beyond the reference's SGD-Nesterov (which stays in eltwise.hip):
// tf.keras 2.4 SGD without momentum / with plain momentum / Nesterov, and Adam / AMSGrad (OptimizerV2,
// ResourceApplyGradientDescent / ResourceApplyKerasMomentum / ResourceApplyAdam).
// Single-pass streaming kernels: float4 loads and stores, grid-stride, no LDS.  The iteration count lives on the device
// (state[0]), exactly as for lisec_sgd_nesterov_step_dev, so that a recorded step re-issues them unchanged.
#include "common.h"

namespace lisec {
namespace {

constexpr int kOptBlocks = 1024;
constexpr int kOptThreads = 256;

int opt_blocks(long long work_items) {
    long long b = (work_items + kOptThreads - 1) / kOptThreads;
    if (b < 1) b = 1;
    return (int)(b > kOptBlocks ? kOptBlocks : b);
}

// The iteration count of the step, read by every workgroup before any of them may advance it.
__device__ __forceinline__ long long read_iterations(const long long* state) {
    return __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// advance == 1: the workgroup that takes the last ticket increments state[0], i.e. after every workgroup has read it
// (state[1] is the ticket counter, 0 between launches).  advance == 0: the update of a PART of the variables ahead of
// the rest of the step; the count is left alone.
__device__ __forceinline__ void advance_iterations(long long* state, long long it) {
    __syncthreads();                                                   // every wave of this workgroup has read `it`
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(&state[1]), 1ULL);
        if (t == (unsigned long long)gridDim.x - 1) {
            __hip_atomic_store(&state[1], 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// lr_t = lr / (1 + decay*it), in double and rounded once: what the SGD-Nesterov kernel computes
__device__ __forceinline__ float decayed_lr(double lr, double decay, long long it) {
    return (float)(lr / (1.0 + decay * (double)it));
}

enum SgdKind { kSgdPlain = 0, kSgdMomentum = 1, kSgdNesterov = 2 };

// KIND 0 (momentum == 0):  w <- w - lr_t*g                     (no slot: v is not touched)
// KIND 1:                  v <- m*v - lr_t*g;  w <- w + v
// KIND 2 (Nesterov):       v <- m*v - lr_t*g;  w <- w + m*v - lr_t*g   (the arithmetic of k_sgd_nesterov_dev)
template <int KIND>
__global__ void __launch_bounds__(kOptThreads)
k_sgd_dev(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v, long long n4, double lr,
          double decay, float mom, long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = decayed_lr(lr, decay, it);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 W = reinterpret_cast<float4*>(w)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        if constexpr (KIND == kSgdPlain) {
            W.x -= lr_t * G.x; W.y -= lr_t * G.y; W.z -= lr_t * G.z; W.w -= lr_t * G.w;
        } else {
            float4 V = reinterpret_cast<float4*>(v)[i];
#define LISEC_UPD(f) { float nv = mom * V.f - lr_t * G.f; V.f = nv;                                       \
                       W.f = KIND == kSgdNesterov ? W.f + mom * nv - lr_t * G.f : W.f + nv; }
            LISEC_UPD(x) LISEC_UPD(y) LISEC_UPD(z) LISEC_UPD(w)
#undef LISEC_UPD
            reinterpret_cast<float4*>(v)[i] = V;
        }
        reinterpret_cast<float4*>(w)[i] = W;
    }
    if (advance) advance_iterations(state, it);
}

// Adam (AMSGRAD: the amsgrad path), t = it + 1:
//   alpha = lr_t * sqrt(1 - b2^t) / (1 - b1^t)          (b1^t, b2^t in fp32)
//   m <- m + (g - m)*(1 - b1);  v <- v + (g*g - v)*(1 - b2)
//   AMSGRAD: vhat <- max(vhat, v), and vhat replaces v below
//   w <- w - alpha * m / (sqrt(v) + eps)                 (eps outside the square root, as in TF)
// sqrtf and the divisions are correctly rounded (hipcc's default; no fast-math flag is used anywhere in the library).
template <bool AMSGRAD>
__global__ void __launch_bounds__(kOptThreads)
k_adam_dev(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
           float* __restrict__ vhat, long long n4, double lr, double decay, float b1, float b2, float eps,
           long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = decayed_lr(lr, decay, it);
    const float t = (float)(it + 1);
    const float b1p = powf(b1, t), b2p = powf(b2, t);
    const float alpha = lr_t * sqrtf(1.f - b2p) / (1.f - b1p);
    const float c1 = 1.f - b1, c2 = 1.f - b2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 W = reinterpret_cast<float4*>(w)[i], M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        float4 H;
        if constexpr (AMSGRAD) H = reinterpret_cast<float4*>(vhat)[i];
#define LISEC_UPD(f) {                                                                    \
            M.f += (G.f - M.f) * c1;                                                      \
            V.f += (G.f * G.f - V.f) * c2;                                                \
            float den = V.f;                                                              \
            if constexpr (AMSGRAD) { H.f = fmaxf(H.f, V.f); den = H.f; }                  \
            W.f -= alpha * M.f / (sqrtf(den) + eps); }
        LISEC_UPD(x) LISEC_UPD(y) LISEC_UPD(z) LISEC_UPD(w)
#undef LISEC_UPD
        reinterpret_cast<float4*>(w)[i] = W;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        if constexpr (AMSGRAD) reinterpret_cast<float4*>(vhat)[i] = H;
    }
    if (advance) advance_iterations(state, it);
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" int lisec_sgd_step_dev(float* theta, const float* grad, float* velocity, long long n, double lr, double decay,
                                  float momentum, int nesterov, long long* state, int advance, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && grad && state && n >= 0 && n % 4 == 0, "sgd: NULL pointer or n not a multiple of 4");
    LISEC_CHECK_ARG(momentum >= 0.f && (advance == 0 || advance == 1), "sgd: momentum must be >= 0, advance 0 or 1");
    LISEC_CHECK_ARG((velocity == nullptr) == (momentum == 0.f), "sgd: velocity must be NULL exactly when momentum == 0");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(opt_blocks(n / 4)), block(kOptThreads);
    if (momentum == 0.f)
        LISEC_LAUNCH(k_sgd_dev<kSgdPlain>, grid, block, 0, st, theta, grad, velocity, n / 4, lr, decay, momentum, state, advance);
    else if (nesterov)
        LISEC_LAUNCH(k_sgd_dev<kSgdNesterov>, grid, block, 0, st, theta, grad, velocity, n / 4, lr, decay, momentum, state, advance);
    else
        LISEC_LAUNCH(k_sgd_dev<kSgdMomentum>, grid, block, 0, st, theta, grad, velocity, n / 4, lr, decay, momentum, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adam_step_dev(float* theta, const float* grad, float* m, float* v, float* vhat, long long n,
                                   double lr, double decay, float beta1, float beta2, float epsilon, long long* state,
                                   int advance, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && grad && m && v && state && n >= 0 && n % 4 == 0, "adam: NULL pointer or n not a multiple of 4");
    LISEC_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && epsilon >= 0.f,
                    "adam: beta_1 and beta_2 must lie in [0, 1), epsilon must be >= 0");
    LISEC_CHECK_ARG(advance == 0 || advance == 1, "adam: advance must be 0 or 1");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(opt_blocks(n / 4)), block(kOptThreads);
    if (vhat)                                                          // AMSGrad
        LISEC_LAUNCH(k_adam_dev<true>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, lr, decay, beta1, beta2, epsilon,
                     state, advance);
    else
        LISEC_LAUNCH(k_adam_dev<false>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, lr, decay, beta1, beta2, epsilon,
                     state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
