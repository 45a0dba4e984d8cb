// Optimizer updates of the flat parameter buffer beyond the reference's SGD-Nesterov (which stays in eltwise.hip):
// tf.keras 2.4 SGD without momentum / with plain momentum / Nesterov, and Adam / AMSGrad (OptimizerV2,
// ResourceApplyGradientDescent / ResourceApplyKerasMomentum / ResourceApplyAdam).
// Single-pass streaming kernels: float4 loads and stores, grid-stride, no LDS.  The iteration count lives on the device
// (state[0]), exactly as for lisec_sgd_nesterov_step_dev, so that a recorded step re-issues them unchanged.
// The *_sched kernels take lr_t from a learning-rate schedule descriptor in device memory (lisec_lr_schedule, the
// tf.keras 2.4 optimizers.schedules), evaluated at that iteration count once per workgroup and handed to its other
// waves through 4 bytes of LDS (their only LDS).
#include "optim_common.h"

namespace lisec {
namespace {

enum SgdKind { kSgdPlain = 0, kSgdMomentum = 1, kSgdNesterov = 2 };

// The streaming loops of the update kernels, as macros: the by-value and the descriptor kernels expand the same tokens
// inside the kernel itself (a shared helper function changes the code generated for the existing kernels).
//
// KIND 0 (momentum == 0):  w <- w - lr_t*g                     (no slot: v is not touched)
// KIND 1:                  v <- m*v - lr_t*g;  w <- w + v
// KIND 2 (Nesterov):       v <- m*v - lr_t*g;  w <- w + m*v - lr_t*g   (the arithmetic of k_sgd_nesterov_dev)
#define LISEC_SGD_UPD(f) { float nv = mom * V.f - lr_t * G.f; V.f = nv;                                       \
                           W.f = KIND == kSgdNesterov ? W.f + mom * nv - lr_t * G.f : W.f + nv; }
#define LISEC_SGD_LOOP                                                                                                  \
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) { \
        float4 W = reinterpret_cast<float4*>(w)[i];                                                                     \
        const float4 G = reinterpret_cast<const float4*>(g)[i];                                                         \
        if constexpr (KIND == kSgdPlain) {                                                                              \
            W.x -= lr_t * G.x; W.y -= lr_t * G.y; W.z -= lr_t * G.z; W.w -= lr_t * G.w;                                 \
        } else {                                                                                                        \
            float4 V = reinterpret_cast<float4*>(v)[i];                                                                 \
            LISEC_SGD_UPD(x) LISEC_SGD_UPD(y) LISEC_SGD_UPD(z) LISEC_SGD_UPD(w)                                         \
            reinterpret_cast<float4*>(v)[i] = V;                                                                        \
        }                                                                                                               \
        reinterpret_cast<float4*>(w)[i] = W;                                                                            \
    }

template <int KIND>
__global__ void __launch_bounds__(kOptThreads)
k_sgd_dev(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v, long long n4, double lr,
          double decay, float mom, long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = decayed_lr(lr, decay, it);
    LISEC_SGD_LOOP
    if (advance) advance_iterations(state, it);
}

template <int KIND>
__global__ void __launch_bounds__(kOptThreads)
k_sgd_sched(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v, long long n4,
            const lisec_lr_schedule* __restrict__ sched, float mom, long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = workgroup_lr(sched, it);
    LISEC_SGD_LOOP
    if (advance) advance_iterations(state, it);
}
#undef LISEC_SGD_LOOP
#undef LISEC_SGD_UPD

// Adam (AMSGRAD: the amsgrad path), t = it + 1:
//   alpha = lr_t * sqrt(1 - b2^t) / (1 - b1^t)          (b1^t, b2^t in fp32)
//   m <- m + (g - m)*(1 - b1);  v <- v + (g*g - v)*(1 - b2)
//   AMSGRAD: vhat <- max(vhat, v), and vhat replaces v below
//   w <- w - alpha * m / (sqrt(v) + eps)                 (eps outside the square root, as in TF)
// sqrtf and the divisions are correctly rounded (hipcc's default; no fast-math flag is used anywhere in the library).
#define LISEC_ADAM_UPD(f) {                                                               \
            M.f += (G.f - M.f) * c1;                                                      \
            V.f += (G.f * G.f - V.f) * c2;                                                \
            float den = V.f;                                                              \
            if constexpr (AMSGRAD) { H.f = fmaxf(H.f, V.f); den = H.f; }                  \
            W.f -= alpha * M.f / (sqrtf(den) + eps); }
#define LISEC_ADAM_LOOP                                                                                                 \
    const float t = (float)(it + 1);                                                                                    \
    const float b1p = powf(b1, t), b2p = powf(b2, t);                                                                   \
    const float alpha = lr_t * sqrtf(1.f - b2p) / (1.f - b1p);                                                          \
    const float c1 = 1.f - b1, c2 = 1.f - b2;                                                                           \
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) { \
        float4 W = reinterpret_cast<float4*>(w)[i], M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i]; \
        const float4 G = reinterpret_cast<const float4*>(g)[i];                                                         \
        float4 H;                                                                                                       \
        if constexpr (AMSGRAD) H = reinterpret_cast<float4*>(vhat)[i];                                                  \
        LISEC_ADAM_UPD(x) LISEC_ADAM_UPD(y) LISEC_ADAM_UPD(z) LISEC_ADAM_UPD(w)                                         \
        reinterpret_cast<float4*>(w)[i] = W;                                                                            \
        reinterpret_cast<float4*>(m)[i] = M;                                                                            \
        reinterpret_cast<float4*>(v)[i] = V;                                                                            \
        if constexpr (AMSGRAD) reinterpret_cast<float4*>(vhat)[i] = H;                                                  \
    }

template <bool AMSGRAD>
__global__ void __launch_bounds__(kOptThreads)
k_adam_dev(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
           float* __restrict__ vhat, long long n4, double lr, double decay, float b1, float b2, float eps,
           long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = decayed_lr(lr, decay, it);
    LISEC_ADAM_LOOP
    if (advance) advance_iterations(state, it);
}

template <bool AMSGRAD>
__global__ void __launch_bounds__(kOptThreads)
k_adam_sched(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
             float* __restrict__ vhat, long long n4, const lisec_lr_schedule* __restrict__ sched, float b1, float b2,
             float eps, long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = workgroup_lr(sched, it);
    LISEC_ADAM_LOOP
    if (advance) advance_iterations(state, it);
}
#undef LISEC_ADAM_LOOP
#undef LISEC_ADAM_UPD

// lr_out[k] = lr_t at it = state[0] + k (lisec_lr_schedule_eval): one schedule evaluation per element, for tests.
__global__ void __launch_bounds__(kOptThreads)
k_lr_schedule_eval(const lisec_lr_schedule* __restrict__ sched, const long long* __restrict__ state, long long n,
                   float* __restrict__ lr_out) {
    const long long it0 = read_iterations(state);
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
        lr_out[k] = scheduled_lr(sched, it0 + k);
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
    const dim3 grid(grid_blocks(n / 4, kOptThreads, kOptBlocks)), block(kOptThreads);
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
    const dim3 grid(grid_blocks(n / 4, kOptThreads, kOptBlocks)), block(kOptThreads);
    if (vhat)                                                          // AMSGrad
        LISEC_LAUNCH(k_adam_dev<true>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, lr, decay, beta1, beta2, epsilon,
                     state, advance);
    else
        LISEC_LAUNCH(k_adam_dev<false>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, lr, decay, beta1, beta2, epsilon,
                     state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_lr_schedule_set(lisec_lr_schedule* dev_desc, const lisec_lr_schedule* host_desc,
                                     lisec_stream_t stream_) {
    LISEC_CHECK_ARG(dev_desc && host_desc, "lr_schedule_set: NULL descriptor");
    const lisec_lr_schedule& d = *host_desc;
    LISEC_CHECK_ARG(d.kind >= LISEC_LR_CONSTANT && d.kind <= LISEC_LR_COSINE_RESTARTS, "lr_schedule_set: unknown kind %d",
                    d.kind);
    LISEC_CHECK_ARG(d.kind == LISEC_LR_CONSTANT || d.kind == LISEC_LR_PIECEWISE || d.decay_steps > 0.0,
                    "lr_schedule_set: decay_steps must be > 0");
    LISEC_CHECK_ARG(d.kind != LISEC_LR_PIECEWISE || (d.n_boundaries >= 1 && d.n_boundaries <= LISEC_LR_MAX_BOUNDARIES),
                    "lr_schedule_set: a piecewise schedule takes 1 to %d boundaries", LISEC_LR_MAX_BOUNDARIES);
    LISEC_CHECK_ARG(!plan_recording(), "lr_schedule_set: a step plan is being recorded (it would not re-issue the copy)");
    if (hipMemcpyAsync(dev_desc, host_desc, sizeof(lisec_lr_schedule), hipMemcpyHostToDevice,
                       static_cast<hipStream_t>(stream_)) != hipSuccess) {
        set_error("lr_schedule_set: hipMemcpyAsync failed: %s", hipGetErrorString(hipGetLastError()));
        return LISEC_EHIP;
    }
    return LISEC_OK;
}

extern "C" int lisec_lr_schedule_eval(const lisec_lr_schedule* sched, const long long* state, long long n, float* lr_out,
                                      lisec_stream_t stream_) {
    LISEC_CHECK_ARG(sched && state && lr_out && n >= 0, "lr_schedule_eval: NULL pointer or n < 0");
    if (n == 0) return LISEC_OK;
    LISEC_LAUNCH(k_lr_schedule_eval, dim3(grid_blocks(n, kOptThreads, kOptBlocks)), dim3(kOptThreads), 0,
                 static_cast<hipStream_t>(stream_), sched, state, n, lr_out);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_sgd_step_sched(float* theta, const float* grad, float* velocity, long long n,
                                    const lisec_lr_schedule* sched, float momentum, int nesterov, long long* state,
                                    int advance, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && grad && sched && state && n >= 0 && n % 4 == 0,
                    "sgd_sched: NULL pointer or n not a multiple of 4");
    LISEC_CHECK_ARG(momentum >= 0.f && (advance == 0 || advance == 1), "sgd_sched: momentum must be >= 0, advance 0 or 1");
    LISEC_CHECK_ARG((velocity == nullptr) == (momentum == 0.f), "sgd_sched: velocity must be NULL exactly when momentum == 0");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(grid_blocks(n / 4, kOptThreads, kOptBlocks)), block(kOptThreads);
    if (momentum == 0.f)
        LISEC_LAUNCH(k_sgd_sched<kSgdPlain>, grid, block, 0, st, theta, grad, velocity, n / 4, sched, momentum, state, advance);
    else if (nesterov)
        LISEC_LAUNCH(k_sgd_sched<kSgdNesterov>, grid, block, 0, st, theta, grad, velocity, n / 4, sched, momentum, state,
                     advance);
    else
        LISEC_LAUNCH(k_sgd_sched<kSgdMomentum>, grid, block, 0, st, theta, grad, velocity, n / 4, sched, momentum, state,
                     advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adam_step_sched(float* theta, const float* grad, float* m, float* v, float* vhat, long long n,
                                     const lisec_lr_schedule* sched, float beta1, float beta2, float epsilon,
                                     long long* state, int advance, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && grad && m && v && sched && state && n >= 0 && n % 4 == 0,
                    "adam_sched: NULL pointer or n not a multiple of 4");
    LISEC_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && epsilon >= 0.f,
                    "adam_sched: beta_1 and beta_2 must lie in [0, 1), epsilon must be >= 0");
    LISEC_CHECK_ARG(advance == 0 || advance == 1, "adam_sched: advance must be 0 or 1");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(grid_blocks(n / 4, kOptThreads, kOptBlocks)), block(kOptThreads);
    if (vhat)                                                          // AMSGrad
        LISEC_LAUNCH(k_adam_sched<true>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, sched, beta1, beta2, epsilon,
                     state, advance);
    else
        LISEC_LAUNCH(k_adam_sched<false>, grid, block, 0, st, theta, grad, m, v, vhat, n / 4, sched, beta1, beta2, epsilon,
                     state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
