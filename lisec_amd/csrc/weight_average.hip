// Weight averaging of the training step (optimizers.MovingAverage / optimizers.SWA): a second buffer `avg`, shaped like
// the flat parameter buffer theta, follows theta with one pass per optimizer UPDATE.  s is the iteration count before
// the update, w = theta after it, a = avg:
//   LISEC_AVG_EMA   decay_s = 0 for s < start;  min(decay, (1 + k)/(10 + k)), k = s - start, with `dynamic`;  else decay
//                   c = (float)(1.0 - decay_s): in double, rounded once
//                   c == 1.0f:  a <- w                     (a store: a - (a - w) is not w in fp32)
//                   else        a <- a - (a - w) * c       (subtract, multiply, subtract: three roundings)
//   LISEC_AVG_SWA   m = max(0, (s - start) / period);  a snapshot iff s >= start and s == start + m*period
//                   m == 0:     a <- w
//                   else        a <- (a * (float)m + w) / (float)(m + 1)       (multiply, add, divide: three roundings)
//                   not a snapshot: every thread returns and a keeps its bits.  The launch is made all the same: whether
//                   a step is a snapshot depends on the DEVICE iteration count, which the host must not read (a recorded
//                   step plan re-issues the same launches at every count), so "enqueue nothing" is not available.
// Every operation is an IEEE fp32 round-to-nearest-even operation of its own: nothing is contracted into an fma, nothing
// is reassociated, denormals are kept.  s = state[0] + state_bias is read from the device, where the update kernels keep
// the count (state_bias: 0 in front of the update that advances it, -1 behind it).  The coefficient is worked out once
// per workgroup, in double, by one thread, and handed to the other waves through 12 bytes of LDS (the kernel's only LDS,
// as in the update kernels' workgroup_lr).  A streaming kernel in the shape of k_grad_accumulate: float4 loads and
// stores, a grid-stride loop over at most kAvgBlocks workgroups, every element touched by exactly one thread -- no
// atomics, the same bits from run to run.  Per float it reads 8 bytes and writes 4 and is bound by HBM alone.
// lisec_weight_swap exchanges two such buffers bit for bit in the same shape (8 bytes read, 8 written per float).
#include "common.h"

// hipcc contracts a multiply into a following add or subtract by default (-ffp-contract=fast), and HIP's __fmul_rn /
// __fsub_rn / __fadd_rn are plain operators compiled under that default in their header: with them a - (a - w)*c becomes
// fma(-(a - w), c, a) and a*m + w becomes fma(a, m, w), one rounding short of the contract (measured: 1 ulp off in 6 % of
// the elements).  So the operations are this file's own, compiled with contraction off: an operation that does not carry
// the permission cannot be fused, whatever it is inlined into.
#pragma clang fp contract(off)

namespace lisec {
namespace {

constexpr int kAvgThreads = 256;
constexpr int kAvgBlocks = 2048;        // 8 workgroups of 256 per CU on 256 CUs: enough loads in flight to fill HBM

enum AvgAction { kAvgKeep = 0, kAvgStore = 1, kAvgEma = 2, kAvgSwa = 3 };

// What the pass does at iteration count s: the action, and its coefficient -- c for EMA (also with kAvgStore, where it
// is 1), (float)m and in coef1 (float)(m + 1) for SWA.  m_out (may be nullptr): SWA's m, -1 off a snapshot.
__device__ __forceinline__ int avg_coefficient(const lisec_weight_average_desc& d, long long s, float* coef, float* coef1,
                                               long long* m_out) {
    *coef1 = 0.f;
    if (d.kind == LISEC_AVG_SWA) {
        const long long q = s - d.start;
        const long long m = q < 0 ? 0 : q / d.period;
        const bool snapshot = q >= 0 && q == m * d.period;
        if (m_out) *m_out = snapshot ? m : -1;
        *coef = (float)m;
        *coef1 = (float)(m + 1);
        return !snapshot ? kAvgKeep : (m == 0 ? kAvgStore : kAvgSwa);
    }
    double decay = 0.0;
    if (s >= d.start) {
        decay = d.decay;
        if (d.dynamic) {
            const double k = (double)(s - d.start);
            decay = fmin(decay, (1.0 + k) / (10.0 + k));
        }
    }
    const float c = (float)(1.0 - decay);
    *coef = c;
    return c == 1.0f ? kAvgStore : kAvgEma;
}

__device__ __forceinline__ long long avg_iterations(const long long* state, long long bias) {
    return __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + bias;
}

// IEEE fp32 round-to-nearest-even operations of their own (the __f*_rn of the contract in include/lisec_hip.h)
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rn_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_div(float a, float b) { return a / b; }      // correctly rounded: no fast-math flag

#define LISEC_AVG_EMA_UPD(f) R.f = rn_sub(A.f, rn_mul(rn_sub(A.f, W.f), coef));
#define LISEC_AVG_SWA_UPD(f) R.f = rn_div(rn_add(rn_mul(A.f, coef), W.f), coef1);

__global__ void __launch_bounds__(kAvgThreads)
k_weight_average(const float* __restrict__ theta, float* __restrict__ avg, long long n4, lisec_weight_average_desc desc,
                 const long long* __restrict__ state, long long state_bias) {
    __shared__ int action_shared;
    __shared__ float coef_shared[2];
    if (threadIdx.x == 0) {
        float c, c1;
        action_shared = avg_coefficient(desc, avg_iterations(state, state_bias), &c, &c1, nullptr);
        coef_shared[0] = c;
        coef_shared[1] = c1;
    }
    __syncthreads();
    const int action = action_shared;
    const float coef = coef_shared[0], coef1 = coef_shared[1];
    if (action == kAvgKeep) return;
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(theta);
    float4* __restrict__ a4 = reinterpret_cast<float4*>(avg);
    const long long stride = (long long)gridDim.x * kAvgThreads;
    for (long long i = blockIdx.x * (long long)kAvgThreads + threadIdx.x; i < n4; i += stride) {
        const float4 W = w4[i];
        if (action == kAvgStore) {
            a4[i] = W;
            continue;
        }
        const float4 A = a4[i];
        float4 R;
        if (action == kAvgEma) {
            LISEC_AVG_EMA_UPD(x) LISEC_AVG_EMA_UPD(y) LISEC_AVG_EMA_UPD(z) LISEC_AVG_EMA_UPD(w)
        } else {
            LISEC_AVG_SWA_UPD(x) LISEC_AVG_SWA_UPD(y) LISEC_AVG_SWA_UPD(z) LISEC_AVG_SWA_UPD(w)
        }
        a4[i] = R;
    }
}
#undef LISEC_AVG_EMA_UPD
#undef LISEC_AVG_SWA_UPD

__global__ void __launch_bounds__(kAvgThreads)
k_weight_swap(float* __restrict__ a, float* __restrict__ b, long long n4) {
    float4* __restrict__ a4 = reinterpret_cast<float4*>(a);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(b);
    const long long stride = (long long)gridDim.x * kAvgThreads;
    for (long long i = blockIdx.x * (long long)kAvgThreads + threadIdx.x; i < n4; i += stride) {
        const float4 A = a4[i], B = b4[i];
        a4[i] = B;
        b4[i] = A;
    }
}

// c_out[j] / m_out[j] at s = state[0] + j (lisec_weight_average_eval): the device function of the pass, for tests.
__global__ void __launch_bounds__(kAvgThreads)
k_weight_average_eval(lisec_weight_average_desc desc, const long long* __restrict__ state, long long k,
                      float* __restrict__ c_out, long long* __restrict__ m_out) {
    const long long s0 = avg_iterations(state, 0);
    for (long long j = blockIdx.x * (long long)kAvgThreads + threadIdx.x; j < k; j += (long long)gridDim.x * kAvgThreads) {
        float c, c1;
        long long m = -1;
        avg_coefficient(desc, s0 + j, &c, &c1, &m);
        if (desc.kind == LISEC_AVG_EMA) c_out[j] = c;
        else m_out[j] = m;
    }
}

dim3 avg_grid(long long items) {
    const long long b = (items + kAvgThreads - 1) / kAvgThreads;
    return dim3((unsigned)(b > kAvgBlocks ? kAvgBlocks : b));
}

// the descriptor's own checks, shared by the pass and its test entry; the error text, or nullptr
const char* avg_desc_error(const lisec_weight_average_desc& d) {
    if (d.kind != LISEC_AVG_EMA && d.kind != LISEC_AVG_SWA) return "unknown kind";
    if (d.start < 0) return "start must be >= 0";
    if (d.kind == LISEC_AVG_EMA && !(d.decay >= 0.0 && d.decay <= 1.0)) return "decay must lie in [0, 1]";
    if (d.kind == LISEC_AVG_SWA && d.period < 1) return "period must be >= 1";
    return nullptr;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" int lisec_weight_average(const float* theta, float* avg, long long n, const lisec_weight_average_desc* desc,
                                    const long long* state, long long state_bias, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && avg && desc && state, "weight_average: NULL theta, avg, desc or state");
    LISEC_CHECK_ARG(theta != avg, "weight_average: theta and avg are the same buffer");
    LISEC_CHECK_ARG(n >= 0 && n % 4 == 0, "weight_average: n = %lld must be a non-negative multiple of 4", n);
    LISEC_CHECK_ARG((reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(avg)) % 16 == 0,
                    "weight_average: theta and avg must be 16-byte aligned");
    LISEC_CHECK_ARG(reinterpret_cast<uintptr_t>(state) % 8 == 0, "weight_average: state must be 8-byte aligned");
    const char* bad = avg_desc_error(*desc);
    LISEC_CHECK_ARG(!bad, "weight_average: %s (kind %d, start %lld, period %lld, decay %g)", bad, desc->kind, desc->start,
                    desc->period, desc->decay);
    if (n == 0) return LISEC_OK;
    LISEC_LAUNCH(k_weight_average, avg_grid(n / 4), dim3(kAvgThreads), 0, static_cast<hipStream_t>(stream_), theta, avg,
                 n / 4, *desc, state, state_bias);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_weight_swap(float* a, float* b, long long n, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(a && b, "weight_swap: NULL buffer");
    LISEC_CHECK_ARG(a != b, "weight_swap: a and b are the same buffer");
    LISEC_CHECK_ARG(n >= 0 && n % 4 == 0, "weight_swap: n = %lld must be a non-negative multiple of 4", n);
    LISEC_CHECK_ARG((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0,
                    "weight_swap: a and b must be 16-byte aligned");
    if (n == 0) return LISEC_OK;
    LISEC_LAUNCH(k_weight_swap, avg_grid(n / 4), dim3(kAvgThreads), 0, static_cast<hipStream_t>(stream_), a, b, n / 4);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_weight_average_eval(const lisec_weight_average_desc* desc, const long long* state, long long k,
                                         float* c_out, long long* m_out, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(desc && state && k >= 0, "weight_average_eval: NULL desc or state, or k < 0");
    const char* bad = avg_desc_error(*desc);
    LISEC_CHECK_ARG(!bad, "weight_average_eval: %s", bad);
    LISEC_CHECK_ARG(desc->kind == LISEC_AVG_EMA ? c_out != nullptr : m_out != nullptr,
                    "weight_average_eval: EMA needs c_out, SWA needs m_out");
    if (k == 0) return LISEC_OK;
    LISEC_LAUNCH(k_weight_average_eval, avg_grid(k), dim3(kAvgThreads), 0, static_cast<hipStream_t>(stream_), *desc, state,
                 k, c_out, m_out);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
