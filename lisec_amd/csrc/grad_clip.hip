// Gradient clipping (optimizers.clip_gradients: clipvalue, clipnorm, global_clipnorm of tf.keras 2.4 as this project
// restates them): passes over the flat gradient buffer IN FRONT of an optimizer entry, on the same stream, behind the
// penalty pass and in front of the decoupled weight decay.  The table is LAMB's (lisec_lamb_chunk / lisec_lamb_var: every
// trainable variable cut by the chunk rules, each chunk with its variable's index; the flags are ignored here).
//   k_clip_value    k_weight_decay's launch: one workgroup of 256 per chunk, float4 loads and stores; g <- c where
//                   g > c, g <- -c where g < -c, any other g (a NaN, a -0, a denormal) keeps its BITS: the two
//                   comparisons are ordered and the result is chosen among bit patterns, so nothing is canonicalised.
//                   8 bytes of HBM traffic per element.
//   k_clip_sumsq    one workgroup of 256 per chunk (past kClipBlocks chunks the workgroups stride over the table): float4
//                   loads, (double)g*(double)g per thread, summed over the workgroup in order W of reduce.h, one fp64
//                   partial per chunk into the workspace.  4 bytes per element.
//   k_clip_scales   one WAVE per variable: the partials of its chunks in order V; S -> (scale, norm) by clip_scale below.
//   k_clip_total    ONE workgroup of 256 for the global norm: the strided sums of order T over the partials of the whole
//                   table, then order W over the 256 -- an order fixed by n_chunks alone.
//   k_clip_apply    reads its chunk's scale first; exactly 1.0f: the chunk is skipped (no load, no store); otherwise
//                   g <- g*scale, one fp32 multiply per element.  8 bytes per element of a clipped chunk, 0 of the others.
// Launches are ordered by the stream alone, as k_lamb_moments / k_lamb_ratios / k_lamb_apply are: no fence, no counter,
// no atomics -- grad, scales and norms have the same bits from run to run.  Floats outside every chunk keep their bits.
#include "common.h"

// The sum of squares must be (double)g*(double)g added to the running sum in two roundings (the contract of
// include/lisec_hip.h), not an fma of one: everything below is compiled with contraction off, like its neighbours.
#pragma clang fp contract(off)
#include "reduce.h"

namespace lisec {
namespace {

constexpr int kClipThreads = 256;
constexpr int kClipBlocks = 2048;       // 8 workgroups of 256 per CU on 256 CUs; the model's theta is ~1650 chunks

__device__ __forceinline__ float clip_one(float g, float c, float nc) {
    const unsigned bits = g > c ? __float_as_uint(c) : g < nc ? __float_as_uint(nc) : __float_as_uint(g);
    return __uint_as_float(bits);
}

__global__ void __launch_bounds__(kClipThreads)
k_clip_value(float* __restrict__ grad, const lisec_lamb_chunk* __restrict__ chunks, int n_chunks, float c) {
    const float nc = -c;
    for (int k = blockIdx.x; k < n_chunks; k += kClipBlocks) {           // (the grid is at most kClipBlocks wide)
        const lisec_lamb_chunk ch = chunks[k];
        float4* __restrict__ g4 = reinterpret_cast<float4*>(grad + ch.offset);
        const int n4 = ch.count / 4;
        for (int i = threadIdx.x; i < n4; i += kClipThreads) {
            float4 G = g4[i];
            G.x = clip_one(G.x, c, nc);
            G.y = clip_one(G.y, c, nc);
            G.z = clip_one(G.z, c, nc);
            G.w = clip_one(G.w, c, nc);
            g4[i] = G;
        }
    }
}

__global__ void __launch_bounds__(kClipThreads)
k_clip_sumsq(const float* __restrict__ grad, const lisec_lamb_chunk* __restrict__ chunks, int n_chunks,
             double* __restrict__ partials) {
    __shared__ double red[1][kClipThreads / kWave];
    for (int k = blockIdx.x; k < n_chunks; k += kClipBlocks) {
        const lisec_lamb_chunk ch = chunks[k];
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad + ch.offset);
        const int n4 = ch.count / 4;
        double s = 0.0;
        for (int i = threadIdx.x; i < n4; i += kClipThreads) {
            const float4 G = g4[i];
            s += (double)G.x * (double)G.x;
            s += (double)G.y * (double)G.y;
            s += (double)G.z * (double)G.z;
            s += (double)G.w * (double)G.w;
        }
        const double v[1] = {s};
        double t[1];
        block_sums_all<kClipThreads>(v, red, t);
        if (threadIdx.x == 0) partials[k] = t[0];
        __syncthreads();                                                  // red is free for the next chunk
    }
}

// S, the fp64 sum of squares, -> the scale and the norm (one thread).  The scale is formed in fp64 and rounded once.
__device__ __forceinline__ void clip_scale(double S, float clip, float* __restrict__ scale, float* __restrict__ norm) {
    const double c = (double)clip;
    const double n = sqrt(S);
    float s;
    if (!(fabs(S) <= 1.7976931348623157e308))       // an inf or a NaN among the squares
        s = __uint_as_float(0x7fc00000u);
    else
        s = n > c ? (float)(c / n) : 1.0f;
    *scale = s;
    *norm = (float)n;
}

// One wave per variable.  The partials were written by the launch in front of this one; stream order is the barrier.
__global__ void __launch_bounds__(kWave)
k_clip_scales(const lisec_lamb_var* __restrict__ vars, int n_vars, const double* __restrict__ partials, float clip,
              float* __restrict__ scales, float* __restrict__ norms) {
    for (int j = blockIdx.x; j < n_vars; j += kClipBlocks) {
        const lisec_lamb_var var = vars[j];
        double s[1];
        wave_strided_sums(partials, var.first_chunk, var.n_chunks, s);
        if (threadIdx.x == 0) clip_scale(s[0], clip, scales + j, norms + j);
    }
}

// One workgroup for the whole table: the scale of everything.
__global__ void __launch_bounds__(kClipThreads)
k_clip_total(const double* __restrict__ partials, int n_chunks, float clip, float* __restrict__ scales,
             float* __restrict__ norms) {
    __shared__ double red[1][kClipThreads / kWave];
    double s[1], t[1];
    strided_sums<kClipThreads>(partials, n_chunks, s);
    block_sums_all<kClipThreads>(s, red, t);
    if (threadIdx.x == 0) clip_scale(t[0], clip, scales, norms);
}

// shared_scale: every chunk reads scales[0] (the global norm); otherwise scales[chunk.var].
__global__ void __launch_bounds__(kClipThreads)
k_clip_apply(float* __restrict__ grad, const lisec_lamb_chunk* __restrict__ chunks, int n_chunks,
             const float* __restrict__ scales, int shared_scale) {
    for (int k = blockIdx.x; k < n_chunks; k += kClipBlocks) {
        const lisec_lamb_chunk ch = chunks[k];
        const float scale = scales[shared_scale ? 0 : ch.var];
        if (scale == 1.0f) continue;                                      // (uniform over the workgroup)
        float4* __restrict__ g4 = reinterpret_cast<float4*>(grad + ch.offset);
        const int n4 = ch.count / 4;
        for (int i = threadIdx.x; i < n4; i += kClipThreads) {
            float4 G = g4[i];
            G.x = G.x * scale;
            G.y = G.y * scale;
            G.z = G.z * scale;
            G.w = G.w * scale;
            g4[i] = G;
        }
    }
}

inline bool threshold_ok(float c) { return c > 0.f && c <= 3.402823466e+38f; }       // (a NaN fails both comparisons)
// (1 for n == 0, but no entry launches over an empty range: each returns early, and n_vars is 0 only with n_chunks)
inline int wide(int n) { return grid_blocks(n, 1, kClipBlocks); }

// What every entry asks of its gradient, its chunk range and (unless there is none) its workspace.
int check_range(const char* who, const float* grad, const lisec_lamb_chunk* chunks, int first_chunk, int n_chunks,
                const void* workspace, size_t workspace_bytes, bool has_workspace) {
    LISEC_CHECK_ARG(grad && chunks && (workspace || !has_workspace), "%s: NULL grad, chunks or workspace", who);
    LISEC_CHECK_ARG(first_chunk >= 0 && n_chunks >= 0, "%s: chunks [%d, +%d)", who, first_chunk, n_chunks);
    LISEC_CHECK_ARG((long long)first_chunk + n_chunks <= INT32_MAX, "%s: the table ends past 2^31 rows", who);
    LISEC_CHECK_ARG(aligned(grad, 16), "%s: grad must be 16-byte aligned", who);
    LISEC_CHECK_ARG(aligned(chunks, 8), "%s: chunks must be 8-byte aligned", who);
    if (has_workspace) {
        LISEC_CHECK_ARG(aligned(workspace, 8), "%s: workspace must be 8-byte aligned", who);
        LISEC_CHECK_ARG(workspace_bytes >= lisec_grad_clip_workspace_bytes(first_chunk + n_chunks),
                        "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                        lisec_grad_clip_workspace_bytes(first_chunk + n_chunks));
    }
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_grad_clip_workspace_bytes(int n_chunks) {
    return sizeof(double) * (size_t)(n_chunks > 0 ? n_chunks : 1);
}

extern "C" int lisec_grad_clip_value(float* grad, const lisec_lamb_chunk* chunks, int first_chunk, int n_chunks, float clip,
                                     lisec_stream_t stream_) {
    if (int rc = check_range("grad_clip_value", grad, chunks, first_chunk, n_chunks, nullptr, 0, false)) return rc;
    LISEC_CHECK_ARG(threshold_ok(clip), "grad_clip_value: the threshold must be a finite number > 0, not %g", (double)clip);
    if (n_chunks == 0) return LISEC_OK;
    LISEC_LAUNCH(k_clip_value, dim3(wide(n_chunks)), dim3(kClipThreads), 0, static_cast<hipStream_t>(stream_), grad,
                 chunks + first_chunk, n_chunks, clip);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_grad_clip_norm(float* grad, const lisec_lamb_chunk* chunks, int first_chunk, int n_chunks,
                                    const lisec_lamb_var* vars, int first_var, int n_vars, float clip, float* scales,
                                    float* norms, void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_range("grad_clip_norm", grad, chunks, first_chunk, n_chunks, workspace, workspace_bytes, true))
        return rc;
    LISEC_CHECK_ARG(vars && scales && norms, "grad_clip_norm: NULL vars, scales or norms");
    LISEC_CHECK_ARG(first_var >= 0 && n_vars >= 0 && (n_chunks == 0) == (n_vars == 0) && n_vars <= n_chunks &&
                        (long long)first_var + n_vars <= INT32_MAX,
                    "grad_clip_norm: chunks [%d, +%d), variables [%d, +%d)", first_chunk, n_chunks, first_var, n_vars);
    LISEC_CHECK_ARG(aligned(vars, 4) && aligned(scales, 4) && aligned(norms, 4),
                    "grad_clip_norm: vars, scales and norms must be 4-byte aligned");
    LISEC_CHECK_ARG(threshold_ok(clip), "grad_clip_norm: the threshold must be a finite number > 0, not %g", (double)clip);
    if (n_chunks == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    // chunk c of the table has its partial at workspace[c], variable j its scale at scales[j]: both parts of a split
    // update use slots of their own.  A kernel walks its rows from the first row of the RANGE, but lisec_lamb_chunk.var
    // and lisec_lamb_var.first_chunk count from the first row of the TABLE: what they index is passed whole.
    double* partials = static_cast<double*>(workspace);
    LISEC_LAUNCH(k_clip_sumsq, dim3(wide(n_chunks)), dim3(kClipThreads), 0, st, (const float*)grad, chunks + first_chunk,
                 n_chunks, partials + first_chunk);
    LISEC_LAUNCH(k_clip_scales, dim3(wide(n_vars)), dim3(kWave), 0, st, vars + first_var, n_vars,
                 (const double*)partials, clip, scales + first_var, norms + first_var);
    LISEC_LAUNCH(k_clip_apply, dim3(wide(n_chunks)), dim3(kClipThreads), 0, st, grad, chunks + first_chunk, n_chunks,
                 (const float*)scales, 0);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_grad_clip_global_norm_partials(const float* grad, const lisec_lamb_chunk* chunks, int first_chunk,
                                                    int n_chunks, void* workspace, size_t workspace_bytes,
                                                    lisec_stream_t stream_) {
    if (int rc = check_range("grad_clip_global_norm_partials", grad, chunks, first_chunk, n_chunks, workspace,
                             workspace_bytes, true))
        return rc;
    if (n_chunks == 0) return LISEC_OK;
    LISEC_LAUNCH(k_clip_sumsq, dim3(wide(n_chunks)), dim3(kClipThreads), 0, static_cast<hipStream_t>(stream_), grad,
                 chunks + first_chunk, n_chunks, static_cast<double*>(workspace) + first_chunk);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_grad_clip_global_norm_finish(float* grad, const lisec_lamb_chunk* chunks, int table_chunks,
                                                  int first_chunk, int n_chunks, float clip, float* scales, float* norms,
                                                  void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_range("grad_clip_global_norm_finish", grad, chunks, first_chunk, n_chunks, workspace,
                             workspace_bytes, true))
        return rc;
    LISEC_CHECK_ARG(scales && norms && aligned(scales, 4) && aligned(norms, 4),
                    "grad_clip_global_norm_finish: NULL or misaligned scales or norms");
    LISEC_CHECK_ARG(table_chunks >= 0 && (long long)first_chunk + n_chunks <= table_chunks,
                    "grad_clip_global_norm_finish: chunks [%d, +%d) of a table of %d", first_chunk, n_chunks, table_chunks);
    LISEC_CHECK_ARG(workspace_bytes >= lisec_grad_clip_workspace_bytes(table_chunks),
                    "grad_clip_global_norm_finish: workspace of %zu bytes, %zu needed", workspace_bytes,
                    lisec_grad_clip_workspace_bytes(table_chunks));
    LISEC_CHECK_ARG(threshold_ok(clip), "grad_clip_global_norm_finish: the threshold must be a finite number > 0, not %g",
                    (double)clip);
    hipStream_t st = static_cast<hipStream_t>(stream_);
    LISEC_LAUNCH(k_clip_total, dim3(1), dim3(kClipThreads), 0, st, (const double*)static_cast<double*>(workspace),
                 table_chunks, clip, scales, norms);
    if (n_chunks > 0)
        LISEC_LAUNCH(k_clip_apply, dim3(wide(n_chunks)), dim3(kClipThreads), 0, st, grad, chunks + first_chunk, n_chunks,
                     (const float*)scales, 1);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
