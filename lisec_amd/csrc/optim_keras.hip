// tf.keras 2.4 (OptimizerV2) RMSprop, Adagrad, Adadelta, Adamax and Nadam on the flat parameter buffer, with the update
// arithmetic of TF's dense kernels: RMSprop's Python path (momentum == 0) and ResourceApplyRMSProp /
// ResourceApplyCenteredRMSProp, ResourceApplyAdagradV2, ResourceApplyAdadelta, ResourceApplyAdaMax, and Nadam's
// _resource_apply_dense.  The kernels of optim.hip in shape and contract: single-pass float4 streaming, grid-stride over
// at most 1024 workgroups of 256 threads, the device iteration count state[0] with its ticket rule (advance = 0: a part
// of the variables ahead of the rest of the step), lr_t by value (*_dev) or from the schedule descriptor (*_sched, whose
// 4-byte LDS hand-off is their only LDS).  Per-step scalars are fp32, as TF computes them; sqrtf and the divisions are
// correctly rounded (no fast-math flag is used anywhere in the library).
#include "optim_common.h"

namespace lisec {
namespace {

#define LISEC_OPT_LOOP                                                                                                  \
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
#define LISEC_F4(p) reinterpret_cast<float4*>(p)[i]
#define LISEC_G4 reinterpret_cast<const float4*>(g)[i]

// The by-value and the descriptor kernel of one optimizer: the same loop (a macro) after a different lr_t.
#define LISEC_KERAS_KERNELS(NAME, TPARAMS, SLOT_PARAMS, HYPER_PARAMS, LOOP)                                           \
    TPARAMS __global__ void __launch_bounds__(kOptThreads)                                                             \
    k_##NAME##_dev(float* __restrict__ w, const float* __restrict__ g, SLOT_PARAMS, long long n4, double lr,           \
                   double decay, HYPER_PARAMS, long long* __restrict__ state, int advance) {                            \
        const long long it = read_iterations(state);                                                                    \
        const float lr_t = decayed_lr(lr, decay, it);                                                                   \
        LOOP                                                                                                            \
        if (advance) advance_iterations(state, it);                                                                     \
    }                                                                                                                   \
    TPARAMS __global__ void __launch_bounds__(kOptThreads)                                                             \
    k_##NAME##_sched(float* __restrict__ w, const float* __restrict__ g, SLOT_PARAMS, long long n4,                     \
                     const lisec_lr_schedule* __restrict__ sched, HYPER_PARAMS, long long* __restrict__ state,          \
                     int advance) {                                                                                     \
        const long long it = read_iterations(state);                                                                    \
        const float lr_t = workgroup_lr(sched, it);                                                                     \
        LOOP                                                                                                            \
        if (advance) advance_iterations(state, it);                                                                     \
    }

#define LISEC_COMMA ,

// RMSprop, c = 1 - rho.  FLAGS: kCentered | kMomentum.
//   momentum == 0 (TF's Python path, eps outside the root):
//     rms <- rho*rms + c*g^2;  centered: mg <- rho*mg + c*g, den = rms - mg^2 (else den = rms);  w <- w - lr_t*g/(sqrt(den) + eps)
//   momentum > 0 (ResourceApplyRMSProp / ResourceApplyCenteredRMSProp, eps inside the root):
//     rms <- rms + (g^2 - rms)*c;  centered: mg <- mg + (g - mg)*c, den = rms - mg^2 + eps (else rms + eps)
//     mom <- mom*momentum + g*lr_t/sqrt(den);  w <- w - mom
constexpr int kCentered = 1, kMomentum = 2;
#define LISEC_RMSPROP_UPD(f) {                                                                                          \
        if constexpr ((FLAGS & kMomentum) != 0) {                                                                       \
            R.f += (G.f * G.f - R.f) * c;                                                                               \
            float den = R.f + eps;                                                                                      \
            if constexpr ((FLAGS & kCentered) != 0) { A.f += (G.f - A.f) * c; den = (R.f - A.f * A.f) + eps; }         \
            P.f = P.f * momentum + (G.f * lr_t) / sqrtf(den);                                                           \
            W.f -= P.f;                                                                                                 \
        } else {                                                                                                        \
            R.f = rho * R.f + c * (G.f * G.f);                                                                          \
            float den = R.f;                                                                                            \
            if constexpr ((FLAGS & kCentered) != 0) { A.f = rho * A.f + c * G.f; den = R.f - A.f * A.f; }               \
            W.f -= lr_t * G.f / (sqrtf(den) + eps);                                                                     \
        } }
#define LISEC_RMSPROP_LOOP                                                                                              \
    const float c = 1.f - rho;                                                                                          \
    LISEC_OPT_LOOP {                                                                                                    \
        float4 W = LISEC_F4(w), R = LISEC_F4(rms), P, A;                                                                \
        const float4 G = LISEC_G4;                                                                                      \
        if constexpr ((FLAGS & kMomentum) != 0) P = LISEC_F4(mom);                                                      \
        if constexpr ((FLAGS & kCentered) != 0) A = LISEC_F4(mg);                                                       \
        LISEC_RMSPROP_UPD(x) LISEC_RMSPROP_UPD(y) LISEC_RMSPROP_UPD(z) LISEC_RMSPROP_UPD(w)                             \
        LISEC_F4(w) = W;                                                                                                \
        LISEC_F4(rms) = R;                                                                                              \
        if constexpr ((FLAGS & kMomentum) != 0) LISEC_F4(mom) = P;                                                      \
        if constexpr ((FLAGS & kCentered) != 0) LISEC_F4(mg) = A;                                                       \
    }
LISEC_KERAS_KERNELS(rmsprop, template <int FLAGS>,
                    float* __restrict__ rms LISEC_COMMA float* __restrict__ mom LISEC_COMMA float* __restrict__ mg,
                    float rho LISEC_COMMA float momentum LISEC_COMMA float eps, LISEC_RMSPROP_LOOP)

// Adagrad (ResourceApplyAdagradV2):  acc <- acc + g^2;  w <- w - g*lr_t/(sqrt(acc) + eps)
#define LISEC_ADAGRAD_UPD(f) { A.f += G.f * G.f; W.f -= G.f * lr_t / (sqrtf(A.f) + eps); }
#define LISEC_ADAGRAD_LOOP                                                                                              \
    LISEC_OPT_LOOP {                                                                                                    \
        float4 W = LISEC_F4(w), A = LISEC_F4(acc);                                                                      \
        const float4 G = LISEC_G4;                                                                                      \
        LISEC_ADAGRAD_UPD(x) LISEC_ADAGRAD_UPD(y) LISEC_ADAGRAD_UPD(z) LISEC_ADAGRAD_UPD(w)                             \
        LISEC_F4(w) = W;                                                                                                \
        LISEC_F4(acc) = A;                                                                                              \
    }
LISEC_KERAS_KERNELS(adagrad, , float* __restrict__ acc, float eps, LISEC_ADAGRAD_LOOP)

// Adadelta (ResourceApplyAdadelta), c = 1 - rho:
//   ag <- ag*rho + g^2*c;  u = sqrt(av + eps) * rsqrt(ag + eps) * g;  w <- w - u*lr_t;  av <- av*rho + u^2*c
#define LISEC_ADADELTA_UPD(f) {                                                                                         \
        AG.f = AG.f * rho + G.f * G.f * c;                                                                              \
        const float u = sqrtf(AV.f + eps) * (1.f / sqrtf(AG.f + eps)) * G.f;                                            \
        W.f -= u * lr_t;                                                                                                \
        AV.f = AV.f * rho + u * u * c; }
#define LISEC_ADADELTA_LOOP                                                                                             \
    const float c = 1.f - rho;                                                                                          \
    LISEC_OPT_LOOP {                                                                                                    \
        float4 W = LISEC_F4(w), AG = LISEC_F4(ag), AV = LISEC_F4(av);                                                   \
        const float4 G = LISEC_G4;                                                                                      \
        LISEC_ADADELTA_UPD(x) LISEC_ADADELTA_UPD(y) LISEC_ADADELTA_UPD(z) LISEC_ADADELTA_UPD(w)                         \
        LISEC_F4(w) = W;                                                                                                \
        LISEC_F4(ag) = AG;                                                                                              \
        LISEC_F4(av) = AV;                                                                                              \
    }
LISEC_KERAS_KERNELS(adadelta, , float* __restrict__ ag LISEC_COMMA float* __restrict__ av,
                    float rho LISEC_COMMA float eps, LISEC_ADADELTA_LOOP)

// Adamax (ResourceApplyAdaMax), t = it + 1, b1^t in fp32:
//   m <- m + (g - m)*(1 - b1);  v <- max(b2*v, |g|);  w <- w - lr_t/(1 - b1^t) * (m/(v + eps))
#define LISEC_ADAMAX_UPD(f) { M.f += (G.f - M.f) * c1; V.f = fmaxf(b2 * V.f, fabsf(G.f)); W.f -= a * (M.f / (V.f + eps)); }
#define LISEC_ADAMAX_LOOP                                                                                               \
    const float a = lr_t / (1.f - powf(b1, (float)(it + 1)));                                                           \
    const float c1 = 1.f - b1;                                                                                          \
    LISEC_OPT_LOOP {                                                                                                    \
        float4 W = LISEC_F4(w), M = LISEC_F4(m), V = LISEC_F4(v);                                                       \
        const float4 G = LISEC_G4;                                                                                      \
        LISEC_ADAMAX_UPD(x) LISEC_ADAMAX_UPD(y) LISEC_ADAMAX_UPD(z) LISEC_ADAMAX_UPD(w)                                 \
        LISEC_F4(w) = W;                                                                                                \
        LISEC_F4(m) = M;                                                                                                \
        LISEC_F4(v) = V;                                                                                                \
    }
LISEC_KERAS_KERNELS(adamax, , float* __restrict__ m LISEC_COMMA float* __restrict__ v,
                    float b1 LISEC_COMMA float b2 LISEC_COMMA float eps, LISEC_ADAMAX_LOOP)

#undef LISEC_KERAS_KERNELS

// Nadam (_resource_apply_dense of tf.keras 2.4), t = it + 1, every per-step scalar in fp32:
//   mu_t = b1*(1 - 0.5*0.96^(d*t)),  mu_t1 = b1*(1 - 0.5*0.96^(d*(t + 1))),  d = schedule_decay
//   P = cache*mu_t,  P1 = P*mu_t1   (cache: the momentum_cache of the step before, 1 at the start)
//   m <- b1*m + (1 - b1)*g;  v <- b2*v + (1 - b2)*g^2
//   w <- w - lr*((1 - mu_t)*(g/(1 - P)) + mu_t1*(m/(1 - P1))) / (sqrt(v/(1 - b2^t)) + eps)
// lr is not divided by 1 + decay*it (a CONSTANT descriptor with decay = 0 gives the same lr_t).  Every workgroup reads
// the cache first; the one that takes the last ticket of an advance = 1 launch writes P back with a vector store, where
// it advances state[0] -- after every workgroup of this launch and of the advance = 0 launch before it has read it.
__device__ __forceinline__ void advance_iterations_cache(long long* state, long long it, float* cache, float p) {
    __syncthreads();                                                   // every wave of this workgroup has read `it`
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(&state[1]), 1ULL);
        if (t == (unsigned long long)gridDim.x - 1) {
            __hip_atomic_store(cache, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[1], 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#define LISEC_NADAM_UPD(f) {                                                                                            \
        const float gp = G.f / omp;                                                                                     \
        M.f = b1 * M.f + c1 * G.f;                                                                                      \
        V.f = b2 * V.f + c2 * (G.f * G.f);                                                                              \
        const float mbar = om_mu * gp + mu_t1 * (M.f / omp1);                                                           \
        W.f -= lr_t * mbar / (sqrtf(V.f / omv) + eps); }
#define LISEC_NADAM_LOOP                                                                                                \
    const float cache0 = __hip_atomic_load(cache, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                          \
    const float t = (float)(it + 1), t1 = (float)(it + 2);                                                              \
    const float mu_t = b1 * (1.f - 0.5f * powf(0.96f, sd * t));                                                         \
    const float mu_t1 = b1 * (1.f - 0.5f * powf(0.96f, sd * t1));                                                       \
    const float p = cache0 * mu_t, p1 = p * mu_t1;                                                                      \
    const float omp = 1.f - p, omp1 = 1.f - p1, omv = 1.f - powf(b2, t), om_mu = 1.f - mu_t;                            \
    const float c1 = 1.f - b1, c2 = 1.f - b2;                                                                           \
    LISEC_OPT_LOOP {                                                                                                    \
        float4 W = LISEC_F4(w), M = LISEC_F4(m), V = LISEC_F4(v);                                                       \
        const float4 G = LISEC_G4;                                                                                      \
        LISEC_NADAM_UPD(x) LISEC_NADAM_UPD(y) LISEC_NADAM_UPD(z) LISEC_NADAM_UPD(w)                                     \
        LISEC_F4(w) = W;                                                                                                \
        LISEC_F4(m) = M;                                                                                                \
        LISEC_F4(v) = V;                                                                                                \
    }                                                                                                                   \
    if (advance) advance_iterations_cache(state, it, cache, p);

__global__ void __launch_bounds__(kOptThreads)
k_nadam_dev(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            float* __restrict__ cache, long long n4, double lr, float b1, float b2, float eps, float sd,
            long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = decayed_lr(lr, 0.0, it);
    LISEC_NADAM_LOOP
}

__global__ void __launch_bounds__(kOptThreads)
k_nadam_sched(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
              float* __restrict__ cache, long long n4, const lisec_lr_schedule* __restrict__ sched, float b1, float b2,
              float eps, float sd, long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = workgroup_lr(sched, it);
    LISEC_NADAM_LOOP
}

#undef LISEC_NADAM_LOOP
#undef LISEC_NADAM_UPD
#undef LISEC_ADAMAX_LOOP
#undef LISEC_ADAMAX_UPD
#undef LISEC_ADADELTA_LOOP
#undef LISEC_ADADELTA_UPD
#undef LISEC_ADAGRAD_LOOP
#undef LISEC_ADAGRAD_UPD
#undef LISEC_RMSPROP_LOOP
#undef LISEC_RMSPROP_UPD
#undef LISEC_COMMA
#undef LISEC_G4
#undef LISEC_F4
#undef LISEC_OPT_LOOP

bool unit_interval(float x) { return x >= 0.f && x < 1.f; }

}  // namespace
}  // namespace lisec

using namespace lisec;

// The checks of every entry, before anything is enqueued; `sched_or_true` is the descriptor of the *_sched form (true
// for the by-value form).
#define LISEC_OPT_CHECKS(who, slots_ok, slots_msg, hyper_ok, hyper_msg, sched_or_true)                                 \
    LISEC_CHECK_ARG(theta && grad && state && (sched_or_true) && n >= 0 && n % 4 == 0,                                 \
                    who ": NULL pointer or n not a multiple of 4");                                                     \
    LISEC_CHECK_ARG(slots_ok, who ": " slots_msg);                                                                      \
    LISEC_CHECK_ARG(hyper_ok, who ": " hyper_msg);                                                                      \
    LISEC_CHECK_ARG(advance == 0 || advance == 1, who ": advance must be 0 or 1");                                      \
    if (n == 0) return LISEC_OK;                                                                                        \
    hipStream_t st = static_cast<hipStream_t>(stream_);                                                                 \
    const dim3 grid(grid_blocks(n / 4, kOptThreads, kOptBlocks)), block(kOptThreads)

#define LISEC_RMSPROP_CHECKS(who, sched_or_true)                                                                        \
    LISEC_OPT_CHECKS(who, rms && (mom == nullptr) == (momentum == 0.f) && (mg == nullptr) == !centered,                \
                     "rms is required; mom must be NULL exactly when momentum == 0, mg exactly when not centered",      \
                     unit_interval(rho) && momentum >= 0.f && epsilon >= 0.f,                                           \
                     "rho must lie in [0, 1), momentum and epsilon must be >= 0", sched_or_true)

template <typename K>
K rmsprop_kernel(K k0, K k1, K k2, K k3, const float* mom, const float* mg) {
    const int flags = (mg ? kCentered : 0) | (mom ? kMomentum : 0);
    return flags == 0 ? k0 : flags == kCentered ? k1 : flags == kMomentum ? k2 : k3;
}

extern "C" int lisec_rmsprop_step_dev(float* theta, const float* grad, float* rms, float* mom, float* mg, long long n,
                                      double lr, double decay, float rho, float momentum, float epsilon, int centered,
                                      long long* state, int advance, lisec_stream_t stream_) {
    LISEC_RMSPROP_CHECKS("rmsprop", true);
    auto k = rmsprop_kernel(k_rmsprop_dev<0>, k_rmsprop_dev<kCentered>, k_rmsprop_dev<kMomentum>,
                            k_rmsprop_dev<kCentered | kMomentum>, mom, mg);
    LISEC_LAUNCH(k, grid, block, 0, st, theta, grad, rms, mom, mg, n / 4, lr, decay, rho, momentum, epsilon, state,
                 advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_rmsprop_step_sched(float* theta, const float* grad, float* rms, float* mom, float* mg, long long n,
                                        const lisec_lr_schedule* sched, float rho, float momentum, float epsilon,
                                        int centered, long long* state, int advance, lisec_stream_t stream_) {
    LISEC_RMSPROP_CHECKS("rmsprop_sched", sched);
    auto k = rmsprop_kernel(k_rmsprop_sched<0>, k_rmsprop_sched<kCentered>, k_rmsprop_sched<kMomentum>,
                            k_rmsprop_sched<kCentered | kMomentum>, mom, mg);
    LISEC_LAUNCH(k, grid, block, 0, st, theta, grad, rms, mom, mg, n / 4, sched, rho, momentum, epsilon, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adagrad_step_dev(float* theta, const float* grad, float* accumulator, long long n, double lr,
                                      double decay, float epsilon, long long* state, int advance,
                                      lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adagrad", accumulator, "accumulator is required", epsilon >= 0.f, "epsilon must be >= 0", true);
    LISEC_LAUNCH(k_adagrad_dev, grid, block, 0, st, theta, grad, accumulator, n / 4, lr, decay, epsilon, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adagrad_step_sched(float* theta, const float* grad, float* accumulator, long long n,
                                        const lisec_lr_schedule* sched, float epsilon, long long* state, int advance,
                                        lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adagrad_sched", accumulator, "accumulator is required", epsilon >= 0.f, "epsilon must be >= 0",
                     sched);
    LISEC_LAUNCH(k_adagrad_sched, grid, block, 0, st, theta, grad, accumulator, n / 4, sched, epsilon, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adadelta_step_dev(float* theta, const float* grad, float* accum_grad, float* accum_var, long long n,
                                       double lr, double decay, float rho, float epsilon, long long* state, int advance,
                                       lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adadelta", accum_grad && accum_var, "accum_grad and accum_var are required",
                     unit_interval(rho) && epsilon >= 0.f, "rho must lie in [0, 1), epsilon must be >= 0", true);
    LISEC_LAUNCH(k_adadelta_dev, grid, block, 0, st, theta, grad, accum_grad, accum_var, n / 4, lr, decay, rho, epsilon,
                 state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adadelta_step_sched(float* theta, const float* grad, float* accum_grad, float* accum_var,
                                         long long n, const lisec_lr_schedule* sched, float rho, float epsilon,
                                         long long* state, int advance, lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adadelta_sched", accum_grad && accum_var, "accum_grad and accum_var are required",
                     unit_interval(rho) && epsilon >= 0.f, "rho must lie in [0, 1), epsilon must be >= 0", sched);
    LISEC_LAUNCH(k_adadelta_sched, grid, block, 0, st, theta, grad, accum_grad, accum_var, n / 4, sched, rho, epsilon,
                 state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adamax_step_dev(float* theta, const float* grad, float* m, float* v, long long n, double lr,
                                     double decay, float beta1, float beta2, float epsilon, long long* state, int advance,
                                     lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adamax", m && v, "m and v are required", unit_interval(beta1) && unit_interval(beta2) && epsilon >= 0.f,
                     "beta_1 and beta_2 must lie in [0, 1), epsilon must be >= 0", true);
    LISEC_LAUNCH(k_adamax_dev, grid, block, 0, st, theta, grad, m, v, n / 4, lr, decay, beta1, beta2, epsilon, state,
                 advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_adamax_step_sched(float* theta, const float* grad, float* m, float* v, long long n,
                                       const lisec_lr_schedule* sched, float beta1, float beta2, float epsilon,
                                       long long* state, int advance, lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("adamax_sched", m && v, "m and v are required",
                     unit_interval(beta1) && unit_interval(beta2) && epsilon >= 0.f,
                     "beta_1 and beta_2 must lie in [0, 1), epsilon must be >= 0", sched);
    LISEC_LAUNCH(k_adamax_sched, grid, block, 0, st, theta, grad, m, v, n / 4, sched, beta1, beta2, epsilon, state,
                 advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_nadam_step_dev(float* theta, const float* grad, float* m, float* v, float* momentum_cache,
                                    long long n, double lr, float beta1, float beta2, float epsilon,
                                    float schedule_decay, long long* state, int advance, lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("nadam", m && v && momentum_cache, "m, v and momentum_cache are required",
                     unit_interval(beta1) && unit_interval(beta2) && epsilon >= 0.f && schedule_decay >= 0.f,
                     "beta_1 and beta_2 must lie in [0, 1), epsilon and schedule_decay must be >= 0", true);
    LISEC_LAUNCH(k_nadam_dev, grid, block, 0, st, theta, grad, m, v, momentum_cache, n / 4, lr, beta1, beta2, epsilon,
                 schedule_decay, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_nadam_step_sched(float* theta, const float* grad, float* m, float* v, float* momentum_cache,
                                      long long n, const lisec_lr_schedule* sched, float beta1, float beta2,
                                      float epsilon, float schedule_decay, long long* state, int advance,
                                      lisec_stream_t stream_) {
    LISEC_OPT_CHECKS("nadam_sched", m && v && momentum_cache, "m, v and momentum_cache are required",
                     unit_interval(beta1) && unit_interval(beta2) && epsilon >= 0.f && schedule_decay >= 0.f,
                     "beta_1 and beta_2 must lie in [0, 1), epsilon and schedule_decay must be >= 0", sched);
    LISEC_LAUNCH(k_nadam_sched, grid, block, 0, st, theta, grad, m, v, momentum_cache, n / 4, sched, beta1, beta2,
                 epsilon, schedule_decay, state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
