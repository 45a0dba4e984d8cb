// Gradient accumulation of a mini-batch (fit(batch_size=B)): the sweeps of a batch run one after the other through the
// batch-1 forward and backward, and between them the flat gradient buffer g is summed into a second buffer acc of the
// same layout.  One pass over n floats, three forms:
//   LISEC_ACC_BEGIN   acc = g                    (first sweep of a batch)
//   LISEC_ACC_ADD     acc = acc + g              (a sweep in the middle)
//   LISEC_ACC_END     g   = (acc + g) * *scale   (last sweep: g becomes the batch mean; acc is only read)
// so that g = (((g1 + g2) + g3) + ... + gB) * s with every add and the one multiply rounded to fp32 on its own
// (__fadd_rn / __fmul_rn: never contracted, never reassociated).  *scale = 1/b is read from the device, so that one
// recorded step plan serves the short last batch of an epoch.  A streaming kernel: float4 loads and stores, a
// grid-stride loop over at most kAccBlocks workgroups, every element touched by exactly one thread -- no atomics, the
// same bits from run to run.  Each pass reads 8 bytes and writes 4 per float and is bound by HBM alone.
#include "common.h"

namespace lisec {
namespace {

constexpr int kAccThreads = 256;
constexpr int kAccBlocks = 2048;        // 8 workgroups of 256 per CU on 256 CUs: enough loads in flight to fill HBM

template <int MODE>
__global__ void __launch_bounds__(kAccThreads)
k_grad_accumulate(float* __restrict__ g, float* __restrict__ acc, long long n4, const float* __restrict__ scale) {
    float4* __restrict__ g4 = reinterpret_cast<float4*>(g);
    float4* __restrict__ a4 = reinterpret_cast<float4*>(acc);
    const float s = MODE == LISEC_ACC_END ? *scale : 1.0f;
    const long long stride = (long long)gridDim.x * kAccThreads;
    for (long long i = blockIdx.x * (long long)kAccThreads + threadIdx.x; i < n4; i += stride) {
        const float4 G = g4[i];
        if (MODE == LISEC_ACC_BEGIN) {
            a4[i] = G;
        } else {
            const float4 A = a4[i];
            float4 R;
            R.x = __fadd_rn(A.x, G.x);
            R.y = __fadd_rn(A.y, G.y);
            R.z = __fadd_rn(A.z, G.z);
            R.w = __fadd_rn(A.w, G.w);
            if (MODE == LISEC_ACC_ADD) {
                a4[i] = R;
            } else {
                R.x = __fmul_rn(R.x, s);
                R.y = __fmul_rn(R.y, s);
                R.z = __fmul_rn(R.z, s);
                R.w = __fmul_rn(R.w, s);
                g4[i] = R;
            }
        }
    }
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" int lisec_grad_accumulate(float* grad, float* acc, long long n, int mode, const float* scale,
                                     lisec_stream_t stream_) {
    LISEC_CHECK_ARG(grad && acc, "grad_accumulate: NULL grad or acc");
    LISEC_CHECK_ARG(grad != acc, "grad_accumulate: grad and acc are the same buffer");
    LISEC_CHECK_ARG(n >= 0 && n % 4 == 0, "grad_accumulate: n = %lld must be a non-negative multiple of 4", n);
    LISEC_CHECK_ARG(mode == LISEC_ACC_BEGIN || mode == LISEC_ACC_ADD || mode == LISEC_ACC_END,
                    "grad_accumulate: mode = %d", mode);
    LISEC_CHECK_ARG(mode != LISEC_ACC_END || scale, "grad_accumulate: LISEC_ACC_END needs the device scale");
    LISEC_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(acc)) % 16 == 0,
                    "grad_accumulate: grad and acc must be 16-byte aligned");
    LISEC_CHECK_ARG(!scale || reinterpret_cast<uintptr_t>(scale) % 4 == 0, "grad_accumulate: scale must be 4-byte aligned");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const long long n4 = n / 4;
    long long b = (n4 + kAccThreads - 1) / kAccThreads;
    const dim3 grid((unsigned)(b > kAccBlocks ? kAccBlocks : b)), block(kAccThreads);
    if (mode == LISEC_ACC_BEGIN)
        LISEC_LAUNCH(k_grad_accumulate<LISEC_ACC_BEGIN>, grid, block, 0, st, grad, acc, n4, scale);
    else if (mode == LISEC_ACC_ADD)
        LISEC_LAUNCH(k_grad_accumulate<LISEC_ACC_ADD>, grid, block, 0, st, grad, acc, n4, scale);
    else
        LISEC_LAUNCH(k_grad_accumulate<LISEC_ACC_END>, grid, block, 0, st, grad, acc, n4, scale);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
