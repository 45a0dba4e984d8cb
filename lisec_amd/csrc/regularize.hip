// Weight regularizers of tf.keras 2.4 (regularizers.L1L2) on the flat parameter buffer, in front of the optimizer update:
//   grad <- grad + 2*l2*w + l1*sign(w)   (sign(0) = 0),      P = sum over chunks of l1*sum|w| + l2*sum w^2
// The host cuts every regularised variable into chunks of at most LISEC_REG_CHUNK floats (lisec_reg_chunk: a chunk never
// crosses a variable, so it has one (l1, l2)); the table lives on the device.  A chunk flagged LISEC_REG_GRAD_IS_ZERO
// belongs to a variable whose slot of grad no backward pass writes: its term is stored, not added.  Two launches:
//   k_regularize         one workgroup of 256 per chunk: float4 loads of theta and grad, float4 store of grad, sum|w| and
//                        sum w^2 per thread in fp64, summed over the workgroup in order W of reduce.h, one fp64 partial
//                        l1*a1 + l2*a2 per chunk into the workspace;
//   k_regularize_finish  one workgroup: the partials in order T of reduce.h, then *penalty = P (or += P) and, given
//                        loss_total, *loss_total = (float)(*loss_total + P).
// The finish is a launch of its own rather than the last workgroup to arrive: stream order is the only ordering it
// needs, so no ticket, no fence and no counter to keep zero between launches, at ~2 us on a pass that runs under the
// backward.  No atomics of any kind: P and the gradient have the same bits from run to run.
#include "reduce.h"

namespace lisec {
namespace {

constexpr int kRegThreads = 256;

#define LISEC_REG_ELEM(f)                                                                  \
    {                                                                                      \
        const float w = W.f;                                                               \
        a1 += (double)fabsf(w);                                                            \
        a2 += (double)w * (double)w;                                                       \
        G.f = G.f + c2 * w + c1 * (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f));                \
    }

__global__ void __launch_bounds__(kRegThreads)
k_regularize(const float* __restrict__ theta, float* __restrict__ grad, const lisec_reg_chunk* __restrict__ chunks,
             double* __restrict__ partials) {
    __shared__ double red[2][kRegThreads / kWave];
    const lisec_reg_chunk c = chunks[blockIdx.x];
    const int n4 = c.count / 4;
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(theta + c.offset);
    float4* g4 = grad ? reinterpret_cast<float4*>(grad + c.offset) : nullptr;
    const float c1 = c.l1, c2 = 2.0f * c.l2;
    const bool write = g4 != nullptr && (c1 != 0.f || c2 != 0.f);       // a (0, 0) chunk keeps the bits of its gradient
    // LISEC_REG_GRAD_IS_ZERO: no backward pass writes this variable's gradient (it is identically 0), so the slot still
    // holds what the step before stored: the term replaces it instead of being added to it
    const bool load = write && !(c.flags & LISEC_REG_GRAD_IS_ZERO);
    double a1 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < n4; i += kRegThreads) {
        const float4 W = w4[i];
        float4 G = load ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        LISEC_REG_ELEM(x) LISEC_REG_ELEM(y) LISEC_REG_ELEM(z) LISEC_REG_ELEM(w)
        if (write) g4[i] = G;
    }
    const double a[2] = {a1, a2};
    double t[2];
    block_sums_all<kRegThreads>(a, red, t);
    if (threadIdx.x == 0) partials[blockIdx.x] = (double)c.l1 * t[0] + (double)c.l2 * t[1];
}
#undef LISEC_REG_ELEM

__global__ void __launch_bounds__(kRegThreads)
k_regularize_finish(const double* __restrict__ partials, int n, double* __restrict__ penalty, int accumulate,
                    float* __restrict__ loss_total) {
    __shared__ double red[1][kRegThreads];
    double a[1];
    strided_sums<kRegThreads>(partials, n, a);
    tree_sums<kRegThreads>(a, red);
    if (threadIdx.x == 0) {
        const double p = accumulate ? *penalty + red[0][0] : red[0][0];
        *penalty = p;
        if (loss_total) *loss_total = (float)((double)*loss_total + p);
    }
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_regularize_workspace_bytes(int n_chunks) {
    return sizeof(double) * (size_t)(n_chunks > 0 ? n_chunks : 1);
}

extern "C" int lisec_regularize(const float* theta, float* grad, const lisec_reg_chunk* chunks, int n_chunks,
                                double* penalty, int accumulate, float* loss_total, void* workspace,
                                size_t workspace_bytes, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && chunks && penalty && workspace, "regularize: NULL theta, chunks, penalty or workspace");
    LISEC_CHECK_ARG(n_chunks >= 0, "regularize: n_chunks = %d", n_chunks);
    LISEC_CHECK_ARG(accumulate == 0 || accumulate == 1, "regularize: accumulate must be 0 or 1");
    LISEC_CHECK_ARG(workspace_bytes >= lisec_regularize_workspace_bytes(n_chunks),
                    "regularize: workspace of %zu bytes, %zu needed", workspace_bytes,
                    lisec_regularize_workspace_bytes(n_chunks));
    LISEC_CHECK_ARG(aligned(theta, 16) && aligned(grad, 16) && aligned(workspace, 8),
                    "regularize: theta and grad must be 16-byte aligned, the workspace 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream_);
    double* partials = static_cast<double*>(workspace);
    if (n_chunks > 0)
        LISEC_LAUNCH(k_regularize, dim3(n_chunks), dim3(kRegThreads), 0, st, theta, grad, chunks, partials);
    LISEC_LAUNCH(k_regularize_finish, dim3(1), dim3(kRegThreads), 0, st, (const double*)partials, n_chunks, penalty,
                 accumulate, loss_total);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
