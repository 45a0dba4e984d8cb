// LAMB (optimizers.LAMB; You et al. 2019, this project's restatement of tfa.optimizers.LAMB): an Adam step whose length
// per VARIABLE is the trust ratio r = ||w|| / ||u||.  The first update of the library that is not element-wise: between
// forming the step u and applying it sits a reduction over each variable.  t = state[0] + 1, c1 = 1 - beta_1^t and
// c2 = 1 - beta_2^t (in double, rounded once: lamb_scalars), and for every element of every chunk
//   m <- beta_1*m + (1 - beta_1)*g          v <- beta_2*v + (1 - beta_2)*(g*g)
//   u  = (m / c1) / (sqrtf(v / c2) + epsilon);   a decayed chunk: u <- u + weight_decay_rate*w
//   r  = (float)(sqrt(sum w^2) / sqrt(sum u^2)) over the variable when it is adapted and both sums are > 0, else 1.0f
//   w <- w - (r*lr_t)*u
// The host cuts every trainable variable of the range into chunks of at most LISEC_REG_CHUNK floats (lisec_lamb_chunk: a
// chunk never crosses a variable and carries its variable's index and the flags LISEC_LAMB_DECAYED / LISEC_LAMB_ADAPTED);
// lisec_lamb_var gives each variable's first chunk and chunk count.  Three launches, ordered by the stream alone:
//   k_lamb_moments  one workgroup of 256 per chunk (past kLambBlocks chunks the workgroups stride over the table): float4
//                   loads of g, m, v, w, float4 stores of m, v; u stays in registers; sum w^2 and sum u^2 per thread in
//                   fp64, summed over the workgroup in order W of reduce.h, one pair of fp64 partials per chunk into
//                   the workspace.  6 floats of HBM traffic per element.
//   k_lamb_ratios   one WAVE per variable: the pairs of the variable's chunks in order V of reduce.h; r is formed in
//                   fp64, rounded once and stored into the caller's float[n_vars] buffer.
//   k_lamb_apply    4 floats per element: reads m, v, w again, forms the SAME u (the same separately rounded operations, see
//                   below), writes w, and ends the step through the ticket protocol of optim_common.h.
// The reduction is a launch of its own rather than a prologue of k_lamb_apply: stream order is the only ordering it
// needs, so no fence and no counter, and each of the ~1600 workgroups of the apply pass reads 4 bytes instead of
// re-adding up to 320 partials (DESIGN 4.4 has the times).  No atomics besides the ticket: theta, the slots and the
// ratios have the same bits from run to run.  grad is only read; floats outside every chunk keep their bits.
#include "common.h"

// hipcc contracts a multiply into a following add by default (-ffp-contract=fast).  k_lamb_moments and k_lamb_apply must
// form bit-identical u, and whether a contraction happens depends on what surrounds the expression, so everything
// below is compiled with contraction off: every operation named in include/lisec_hip.h is rounded on its own.
#pragma clang fp contract(off)
#include "optim_common.h"
#include "reduce.h"

namespace lisec {
namespace {

constexpr int kLambThreads = 256;
constexpr int kLambBlocks = 2048;       // 8 workgroups of 256 per CU on 256 CUs; the model's theta is ~1650 chunks
constexpr int kLambRatioThreads = kWave;

// The per-step scalars of both passes, from the hyper-parameters and the iteration count: the same fp32 operations in
// both kernels, hence the same bits.
struct LambScalars {
    float b1, b2, omb1, omb2, c1, c2, eps, wd;
};

// b^t for an integer t >= 0 in double, by binary exponentiation: at most 63 squarings and no call of pow(), whose code
// a single lane would walk through for microseconds in front of every workgroup's first load.
__device__ __forceinline__ double pow_int(double b, long long t) {
    double r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r = r * b;
        b = b * b;
    }
    return r;
}

// The bias corrections 1 - beta^t cancel (1 - 0.999^8 is 0.008): in fp32 their error would be 1e-5 of u, and of r.  One
// thread of the workgroup forms them in double and rounds once; the other waves get them through 8 bytes of LDS.
__device__ __forceinline__ LambScalars lamb_scalars(float b1, float b2, float eps, float wd, long long it) {
    __shared__ float corrections[2];
    if (threadIdx.x == 0) {
        corrections[0] = (float)(1.0 - pow_int((double)b1, it + 1));
        corrections[1] = (float)(1.0 - pow_int((double)b2, it + 1));
    }
    __syncthreads();
    LambScalars s;
    s.b1 = b1; s.b2 = b2;
    s.omb1 = 1.f - b1; s.omb2 = 1.f - b2;
    s.c1 = corrections[0]; s.c2 = corrections[1];
    s.eps = eps; s.wd = wd;
    return s;
}

// u of one element from the UPDATED moments and the variable before the update (the contract of include/lisec_hip.h:
// two divisions, a square root, an add, a division; a decayed element: a multiply and an add)
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambScalars& s, bool decayed) {
    const float mh = m / s.c1;
    const float vh = v / s.c2;
    float u = mh / (sqrtf(vh) + s.eps);
    if (decayed) {
        const float p = s.wd * w;
        u = u + p;
    }
    return u;
}

#define LISEC_LAMB_MOMENTS(f)                                                              \
    {                                                                                      \
        const float g = G.f, w = W.f;                                                      \
        const float gg = g * g;                                                            \
        const float ma = s.b1 * M.f, mb = s.omb1 * g;                                      \
        const float va = s.b2 * V.f, vb = s.omb2 * gg;                                     \
        M.f = ma + mb;                                                                     \
        V.f = va + vb;                                                                     \
        const float u = lamb_u(M.f, V.f, w, s, decayed);                                   \
        sw += (double)w * (double)w;                                                       \
        su += (double)u * (double)u;                                                       \
    }

__global__ void __launch_bounds__(kLambThreads)
k_lamb_moments(const float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
               float* __restrict__ v, const lisec_lamb_chunk* __restrict__ chunks, int n_chunks,
               double* __restrict__ partials, float b1, float b2, float eps, float wd,
               const long long* __restrict__ state) {
    __shared__ double red[2][kLambThreads / kWave];
    const LambScalars s = lamb_scalars(b1, b2, eps, wd, read_iterations(state));
    for (int c = blockIdx.x; c < n_chunks; c += kLambBlocks) {           // (the grid is at most kLambBlocks wide)
        const lisec_lamb_chunk ch = chunks[c];
        const bool decayed = (ch.flags & LISEC_LAMB_DECAYED) != 0;
        const float4* __restrict__ w4 = reinterpret_cast<const float4*>(theta + ch.offset);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad + ch.offset);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m + ch.offset);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v + ch.offset);
        const int n4 = ch.count / 4;
        double sw = 0.0, su = 0.0;
        for (int i = threadIdx.x; i < n4; i += kLambThreads) {
            const float4 W = w4[i], G = g4[i];
            float4 M = m4[i], V = v4[i];
            LISEC_LAMB_MOMENTS(x) LISEC_LAMB_MOMENTS(y) LISEC_LAMB_MOMENTS(z) LISEC_LAMB_MOMENTS(w)
            m4[i] = M;
            v4[i] = V;
        }
        const double a[2] = {sw, su};
        double t[2];
        block_sums_all<kLambThreads>(a, red, t);
        if (threadIdx.x == 0) {
            partials[2 * (long long)c] = t[0];
            partials[2 * (long long)c + 1] = t[1];
        }
        __syncthreads();                                                  // red is free for the next chunk
    }
}
#undef LISEC_LAMB_MOMENTS

// One wave per variable.  The partials were written by the launch in front of this one; stream order is the barrier.
__global__ void __launch_bounds__(kLambRatioThreads)
k_lamb_ratios(const lisec_lamb_chunk* __restrict__ chunks, const lisec_lamb_var* __restrict__ vars, int n_vars,
              const double* __restrict__ partials, float* __restrict__ ratios) {
    for (int j = blockIdx.x; j < n_vars; j += kLambBlocks) {
        const lisec_lamb_var var = vars[j];
        double s[2];                                                      // sum w^2, sum u^2
        wave_strided_sums(partials, var.first_chunk, var.n_chunks, s);
        if (threadIdx.x == 0) {
            const bool adapted = var.n_chunks > 0 && (chunks[var.first_chunk].flags & LISEC_LAMB_ADAPTED) != 0;
            ratios[j] = adapted && s[0] > 0.0 && s[1] > 0.0 ? (float)(sqrt(s[0]) / sqrt(s[1])) : 1.0f;
        }
    }
}

#define LISEC_LAMB_APPLY(f)                                                                \
    {                                                                                      \
        const float u = lamb_u(M.f, V.f, W.f, s, decayed);                                 \
        const float d = step * u;                                                          \
        W.f = W.f - d;                                                                     \
    }

__global__ void __launch_bounds__(kLambThreads)
k_lamb_apply(float* __restrict__ theta, const float* __restrict__ m, const float* __restrict__ v,
             const lisec_lamb_chunk* __restrict__ chunks, int n_chunks, const float* __restrict__ ratios, double lr,
             double decay, const lisec_lr_schedule* __restrict__ sched, float b1, float b2, float eps, float wd,
             long long* __restrict__ state, int advance) {
    const long long it = read_iterations(state);
    const float lr_t = sched ? workgroup_lr(sched, it) : decayed_lr(lr, decay, it);     // (sched is launch-uniform)
    const LambScalars s = lamb_scalars(b1, b2, eps, wd, it);
    for (int c = blockIdx.x; c < n_chunks; c += kLambBlocks) {
        const lisec_lamb_chunk ch = chunks[c];
        const bool decayed = (ch.flags & LISEC_LAMB_DECAYED) != 0;
        const float step = ratios[ch.var] * lr_t;
        float4* __restrict__ w4 = reinterpret_cast<float4*>(theta + ch.offset);
        const float4* __restrict__ m4 = reinterpret_cast<const float4*>(m + ch.offset);
        const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v + ch.offset);
        const int n4 = ch.count / 4;
        for (int i = threadIdx.x; i < n4; i += kLambThreads) {
            float4 W = w4[i];
            const float4 M = m4[i], V = v4[i];
            LISEC_LAMB_APPLY(x) LISEC_LAMB_APPLY(y) LISEC_LAMB_APPLY(z) LISEC_LAMB_APPLY(w)
            w4[i] = W;
        }
    }
    if (advance) advance_iterations(state, it);
}
#undef LISEC_LAMB_APPLY

int lamb_step(const char* who, float* theta, const float* grad, float* m, float* v, const lisec_lamb_chunk* chunks,
              int first_chunk, int n_chunks, const lisec_lamb_var* vars, int first_var, int n_vars, float* ratios,
              void* workspace, size_t workspace_bytes, double lr, double decay, const lisec_lr_schedule* sched,
              bool by_descriptor, float wd, float b1, float b2, float eps, long long* state, int advance,
              lisec_stream_t stream_) {
    LISEC_CHECK_ARG(theta && grad && m && v && chunks && vars && ratios && workspace && state &&
                        (sched || !by_descriptor),
                    "%s: NULL theta, grad, m, v, chunks, vars, ratios, workspace, state or descriptor", who);
    LISEC_CHECK_ARG(first_chunk >= 0 && n_chunks >= 0 && first_var >= 0 && n_vars >= 0 && (n_chunks == 0) == (n_vars == 0) &&
                        n_vars <= n_chunks,
                    "%s: chunks [%d, +%d), variables [%d, +%d)", who, first_chunk, n_chunks, first_var, n_vars);
    LISEC_CHECK_ARG((long long)first_chunk + n_chunks <= INT32_MAX && (long long)first_var + n_vars <= INT32_MAX,
                    "%s: the table ends past 2^31 rows", who);
    LISEC_CHECK_ARG(b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f && eps >= 0.f && wd >= 0.f,
                    "%s: beta_1 and beta_2 must lie in [0, 1), epsilon and weight_decay_rate must be >= 0", who);
    LISEC_CHECK_ARG(advance == 0 || advance == 1, "%s: advance must be 0 or 1", who);
    LISEC_CHECK_ARG(workspace_bytes >= lisec_lamb_workspace_bytes(first_chunk + n_chunks, first_var + n_vars),
                    "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                    lisec_lamb_workspace_bytes(first_chunk + n_chunks, first_var + n_vars));
    LISEC_CHECK_ARG(aligned(theta, 16) && aligned(grad, 16) && aligned(m, 16) && aligned(v, 16),
                    "%s: theta, grad, m and v must be 16-byte aligned", who);
    LISEC_CHECK_ARG(aligned(workspace, 8) && aligned(state, 8) && aligned(chunks, 8) && aligned(ratios, 4) &&
                        aligned(vars, 4),
                    "%s: workspace, state and chunks must be 8-byte aligned, ratios and vars 4-byte aligned", who);
    if (n_chunks == 0 && !advance) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    // chunk c of the table has its partials at workspace[2c], variable j its ratio at ratios[j]: both parts of a split
    // update use slots of their own.  A kernel walks its rows from the first row of the RANGE (chunks + first_chunk,
    // vars + first_var), but lisec_lamb_chunk.var and lisec_lamb_var.first_chunk count from the first row of the TABLE:
    // what is indexed by them (ratios in k_lamb_apply; chunks and partials in k_lamb_ratios) is passed whole.
    double* partials = static_cast<double*>(workspace);
    const int wide = grid_blocks(n_chunks, 1, kLambBlocks);            // (1 for an empty range: k_lamb_apply's ticket)
    if (n_chunks > 0) {
        LISEC_LAUNCH(k_lamb_moments, dim3(wide), dim3(kLambThreads), 0, st, (const float*)theta, grad, m, v,
                     chunks + first_chunk, n_chunks, partials + 2 * (long long)first_chunk, b1, b2, eps, wd,
                     (const long long*)state);
        LISEC_LAUNCH(k_lamb_ratios, dim3(grid_blocks(n_vars, 1, kLambBlocks)), dim3(kLambRatioThreads), 0, st,
                     chunks, vars + first_var, n_vars, (const double*)partials, ratios + first_var);
    }
    LISEC_LAUNCH(k_lamb_apply, dim3(wide), dim3(kLambThreads), 0, st, theta, (const float*)m,
                 (const float*)v, chunks + first_chunk, n_chunks, (const float*)ratios, lr, decay, sched, b1, b2, eps, wd,
                 state, advance);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_lamb_workspace_bytes(int n_chunks, int n_vars) {
    (void)n_vars;                       // the ratios live in the caller's buffer; a variable needs no workspace of its own
    return 2 * sizeof(double) * (size_t)(n_chunks > 0 ? n_chunks : 1);
}

extern "C" int lisec_lamb_step_dev(float* theta, const float* grad, float* m, float* v, const lisec_lamb_chunk* chunks,
                                   int first_chunk, int n_chunks, const lisec_lamb_var* vars, int first_var, int n_vars,
                                   float* ratios, void* workspace, size_t workspace_bytes, double lr, double decay,
                                   float weight_decay_rate, float beta1, float beta2, float epsilon, long long* state,
                                   int advance, lisec_stream_t stream) {
    return lamb_step("lamb", theta, grad, m, v, chunks, first_chunk, n_chunks, vars, first_var, n_vars, ratios, workspace,
                     workspace_bytes, lr, decay, nullptr, false, weight_decay_rate, beta1, beta2, epsilon, state, advance,
                     stream);
}

extern "C" int lisec_lamb_step_sched(float* theta, const float* grad, float* m, float* v, const lisec_lamb_chunk* chunks,
                                     int first_chunk, int n_chunks, const lisec_lamb_var* vars, int first_var, int n_vars,
                                     float* ratios, void* workspace, size_t workspace_bytes, const lisec_lr_schedule* sched,
                                     float weight_decay_rate, float beta1, float beta2, float epsilon, long long* state,
                                     int advance, lisec_stream_t stream) {
    return lamb_step("lamb_sched", theta, grad, m, v, chunks, first_chunk, n_chunks, vars, first_var, n_vars, ratios,
                     workspace, workspace_bytes, 0.0, 0.0, sched, true, weight_decay_rate, beta1, beta2, epsilon, state,
                     advance, stream);
}
