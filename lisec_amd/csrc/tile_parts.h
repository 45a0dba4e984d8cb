// Internal: the pieces the contraction kernels of igemm.hip and wgrad.hip share -- the on-load transforms of a staged
// float4, the W-slab copy, and the MFMA inner loops over one staged image.  One copy each; a kernel differs by template
// constants only.
#pragma once
#include "splitk.h"

#ifdef __HIPCC__
namespace lisec {
namespace {

// ---- on-load transforms of a staged float4, in place (ok = false: padding, stays zero) --------------------------------
__device__ __forceinline__ void masked(float4& v, bool ok) {
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
}

// BatchNormalization (+ReLU, relu_lo = 0; none, relu_lo = -inf) of the producing layer
__device__ __forceinline__ void affine_relu(float4& v, const float4& sc, const float4& sh, float relu_lo, bool ok) {
    v.x = ok ? fmaxf(fmaf(v.x, sc.x, sh.x), relu_lo) : 0.f;
    v.y = ok ? fmaxf(fmaf(v.y, sc.y, sh.y), relu_lo) : 0.f;
    v.z = ok ? fmaxf(fmaf(v.z, sc.z, sh.z), relu_lo) : 0.f;
    v.w = ok ? fmaxf(fmaf(v.w, sc.w, sh.w), relu_lo) : 0.f;
}

// The apply pass of a BatchNormalization(+ReLU) backward: v = the gradient g, y = the layer's raw output,
// dy = scale (gate(y) g - mean(dz) - yhat mean(dz yhat)) with per-channel scale / shift / mean / 1/std / mean(dz) / mean(dz yhat)
__device__ __forceinline__ float bn_fold1(float v, float y, float sc, float sh, float mu, float is, float m1, float m2, bool relu, bool ok) {
    float dz = v;
    if (relu && !(fmaf(y, sc, sh) > 0.f)) dz = 0.f;
    return ok ? sc * (dz - m1 - (y - mu) * is * m2) : 0.f;
}
__device__ __forceinline__ void bn_fold(float4& v, const float4& y, const float4& sc, const float4& sh, const float4& mu, const float4& is,
                                        const float4& m1, const float4& m2, bool relu, bool ok) {
    v.x = bn_fold1(v.x, y.x, sc.x, sh.x, mu.x, is.x, m1.x, m2.x, relu, ok);
    v.y = bn_fold1(v.y, y.y, sc.y, sh.y, mu.y, is.y, m1.y, m2.y, relu, ok);
    v.z = bn_fold1(v.z, y.z, sc.z, sh.z, mu.z, is.z, m1.z, m2.z, relu, ok);
    v.w = bn_fold1(v.w, y.w, sc.w, sh.w, mu.w, is.w, m1.w, m2.w, relu, ok);
}

// ---- W slab: 16 k-quads x NW columns of float4 in the packed [k/4][n][4] order, a linear copy by 256 threads ---------
// wb: the slab's first float4 (rows CoutP float4 apart).  64 columns: four float4 per thread; 32 columns: two (rb2, rb3
// are not touched).  (Four references, not an array: an array captured by the staging lambdas stays in scratch memory.)
template <int NW>
__device__ __forceinline__ void wslab_load(const float* wb, int CoutP, int tid, float4& rb0, float4& rb1, float4& rb2, float4& rb3) {
    const float* wl = wb + (size_t)(tid / NW) * CoutP * 4 + (tid % NW) * 4;
    const size_t wstep = (size_t)(256 / NW) * CoutP * 4;
    rb0 = *reinterpret_cast<const float4*>(wl);
    rb1 = *reinterpret_cast<const float4*>(wl + wstep);
    if (NW == 64) {
        rb2 = *reinterpret_cast<const float4*>(wl + 2 * wstep);
        rb3 = *reinterpret_cast<const float4*>(wl + 3 * wstep);
    }
}
template <int NW>
__device__ __forceinline__ void wslab_store(float* sB, int tid, const float4& rb0, const float4& rb1, const float4& rb2, const float4& rb3) {
    float* bl = sB + ((tid / NW) * NW + (tid % NW)) * 4;
    *reinterpret_cast<float4*>(bl) = rb0;
    *reinterpret_cast<float4*>(bl + 256 * 4) = rb1;
    if (NW == 64) {
        *reinterpret_cast<float4*>(bl + 2 * 256 * 4) = rb2;
        *reinterpret_cast<float4*>(bl + 3 * 256 * 4) = rb3;
    }
}

// ---- one 64-deep K step of a 32 x 32 (TWO: 32 x 64) wave tile --------------------------------------------------------
// aRow: this lane's A row in LDS (k contiguous), bCol: its column of the packed W slab of NW columns.
// Software-pipelined fragment reads: the ds_reads of chunk kc+1 are issued BEFORE the 8 MFMAs of chunk kc (sched_barrier
// pins that order; left alone hipcc reuses the fragment registers and issues the reads after the MFMAs, exposing ~100
// cycles of LDS latency per 512 MFMA cycles).
// No scalar load may be pending when the fragment reads start: LDS returns in order, scalar memory does not, and with an
// s_load in flight (the geometry lives in the kernel-argument segment) the compiler must wait for EVERY LDS read --
// lgkmcnt(0), the reads of the NEXT chunk included -- before each group of MFMAs instead of the older ones only.
template <bool TWO, int NW>
__device__ __forceinline__ void mfma_step64(const float* aRow, const float* bCol, f32x16& acc0, f32x16& acc1) {
    float4 a = *reinterpret_cast<const float4*>(aRow);
    float4 b0 = *reinterpret_cast<const float4*>(bCol);
    float4 b1 = TWO ? *reinterpret_cast<const float4*>(bCol + 32 * 4) : b0;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
        float4 an = a, b0n = b0, b1n = b1;
        if (kc + 1 < 8) {
            an = *reinterpret_cast<const float4*>(aRow + (kc + 1) * 8);
            b0n = *reinterpret_cast<const float4*>(bCol + (kc + 1) * 2 * NW * 4);
            if (TWO) b1n = *reinterpret_cast<const float4*>(bCol + (kc + 1) * 2 * NW * 4 + 32 * 4);
        }
        __builtin_amdgcn_sched_barrier(0);                        // reads of chunk kc+1 stay above ...
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
        if (TWO) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);                        // ... the 8 MFMAs of chunk kc
        a = an; b0 = b0n; b1 = b1n;
    }
}

// ---- weight-gradient chunk loop: nk chunks of 8 rows, three taps (kw) per wave ----------------------------------------
// aCol / dCol: this lane's column of the halo image / the dY image ([row][ROW] floats); tap kw reads halo rows j + kw.
// Software-pipelined by hand: the ten fragment reads of chunk kk + 1 are issued BEFORE the twelve MFMAs of chunk kk
// (sched_barrier pins that; left alone the reads follow the MFMAs and every chunk waits out the LDS latency)
template <int ROW = 64>
__device__ __forceinline__ void wgrad_chunks(const float* aCol, const float* dCol, int nk, f32x16& acc0, f32x16& acc1, f32x16& acc2) {
    float fa[2][6], fb[2][4];
    auto read = [&](int s, int kk) {
        const float* ap = aCol + kk * 8 * ROW;
        const float* dp = dCol + kk * 8 * ROW;
        fb[s][0] = dp[0]; fb[s][1] = dp[ROW]; fb[s][2] = dp[2 * ROW]; fb[s][3] = dp[3 * ROW];
        fa[s][0] = ap[0]; fa[s][1] = ap[ROW]; fa[s][2] = ap[2 * ROW]; fa[s][3] = ap[3 * ROW];
        fa[s][4] = ap[4 * ROW]; fa[s][5] = ap[5 * ROW];
    };
    auto mfma = [&](int s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][j], fb[s][j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][j + 1], fb[s][j], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][j + 2], fb[s][j], acc2, 0, 0, 0);
        }
    };
    int kk = 0;
    if (nk > 0) read(0, 0);
    for (; kk + 1 < nk; kk += 2) {
        read(1, kk + 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma(0);
        __builtin_amdgcn_sched_barrier(0);
        if (kk + 2 < nk) read(0, kk + 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma(1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (kk < nk) mfma(0);
}

}  // namespace
}  // namespace lisec
#endif
