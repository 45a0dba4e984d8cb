// Inference-only forward implicit GEMM on the bf16 matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16): the kernel behind
// the 'mixed_bfloat16' policy (lisec_amd/mixed_precision.py).
//
// Same buffers as igemm.hip: `in` and `out` are fp32 in HBM in the layouts the fp32 kernels use, and only the MFMA
// operands are bf16.  A gathered fp32 value gets the producing layer's folded BatchNormalization affine (+ReLU) in fp32
// (one fmaf, as k_igemm), is rounded to bf16 to nearest-even (v_cvt_pk_bf16_f32) and staged to LDS; the accumulators are
// fp32 and so are bias, LISEC_CONV_OUT_RELU and the stores.  The layers in front of and behind a call cannot tell which
// kernel ran.  No BatchNormalization statistics, no sink, no output gate, no row list: mode 0, dense rows.
//
// Tiling (256 threads = 4 waves, one per SIMD): 128 output positions x 64 output channels, every wave 32 x 64 = two 32x32
// accumulators.  Per (tap, 64-channel slab):
//   A slab 128 x 64 bf16 -> LDS rows of 128 B padded to 144 B: the ds_read_b128 fragment reads (lane l: row l & 31,
//     k = 8 (l >> 5) .. + 7) of a 16-lane conflict group fall on 16 rows that are distinct mod 16, i.e. 36 r mod 64 =
//     16 different 4-bank slots: conflict-free
//   W slab  64 x 64 bf16 -> LDS in the packed [k / 8][n][8] order (linear 16-byte copy; a fragment read is 512
//     contiguous bytes per lane half)
//   8 MFMAs per wave (256 SIMD cycles; the fp32 form spends 4096 on the same slab).
// With the MFMA time gone a step is the gather's latency, so the loop keeps the fp32 kernel's shape -- the next slab is
// loaded into registers while this one is multiplied and written to LDS between two barriers -- but with 26.6 KB of LDS
// and < 128 registers FOUR workgroups share a CU and cover each other's loads.
// Layers of few tiles (the RPN maps of 5 000 and 1 250 positions) are cut into K slices that meet in slice order inside
// the kernel (splitk_arrive, splitk.h): deterministic, no combine launch.
#include "conv.h"
#include "splitk.h"

namespace lisec {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int kThreads = 256;
constexpr int kRowBytes = 144;                      // 64 bf16 + 16 B of padding
constexpr int kABytes = BM * kRowBytes;             // 18 432
constexpr int kBBytes = (BK / 8) * BN * 16;         // 8 192
constexpr int kMaxSlices = 12;

__device__ __forceinline__ bf16x4 to_bf16(float4 v) {     // round to nearest even: two v_cvt_pk_bf16_f32
    f32x4 f = {v.x, v.y, v.z, v.w};
    return __builtin_convertvector(f, bf16x4);
}

template <bool XF>
__global__ void __launch_bounds__(kThreads, 4)
k_igemm_bf16(ConvGeom g, const float* __restrict__ in, const uint4* __restrict__ wp, const float* __restrict__ bias,
             const float* __restrict__ in_bn, int flags, float* __restrict__ out, int nsplit, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;
    unsigned char* sB = smem + kABytes;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mb = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = mb * BM;
    const int n0 = blockIdx.y * BN;
    const int HW = g.Ho * g.Wo;

    // ---- rows this thread stages: r = p*16 + tid/16, channels 4 * (tid % 16) .. + 3 of the slab ----------------------
    const int piece = tid & 15;
    RowGather rows[8];
    {
        int2* shared_rows = reinterpret_cast<int2*>(smem);      // one descriptor per row, computed once (as igemm_tile)
        if (tid < BM) {
            const RowGather r = row_gather(g, m0 + tid, 0, 0);
            shared_rows[tid] = make_int2(r.off, r.mask);
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int2 v = shared_rows[p * 16 + (tid >> 4)];
            rows[p].off = v.x + piece * 4;
            rows[p].mask = v.y;
        }
        __syncthreads();
    }
    // depth taps that no row of the tile has (a tile inside one depth plane at the edge of a padded Conv3D) are skipped
    const int mlast = (m0 + BM - 1 < g.M ? m0 + BM - 1 : g.M - 1);
    const int d_first = m0 / HW, d_last = mlast / HW;
    int dmask = 0xf;
    if (d_first == d_last) {
        int tmp;
        dmask = axis_mask(d_first, g.KD, g.ls_d, g.pd, g.Di, 0, tmp);
    }

    const int ncc = (g.Cin + BK - 1) / BK;
    const int nsteps = g.KD * g.KH * g.KW * ncc;
    const int KpG = ncc * (BK / 8);                  // packed groups of 8 k per tap

    struct TStep { int s, kd, kh, kw, cc; };
    const int s_end = nsplit > 1 ? (int)(((long long)(blockIdx.z + 1) * nsteps) / nsplit) : nsteps;
    const int s_begin = nsplit > 1 ? (int)(((long long)blockIdx.z * nsteps) / nsplit) : 0;
    auto next_tap = [&](TStep& t) {
        if (++t.kw == g.KW) {
            t.kw = 0;
            if (++t.kh == g.KH) { t.kh = 0; ++t.kd; }
        }
    };
    auto settle = [&](TStep t) -> TStep {            // the first live step at or after t; nsteps when the slice has none
        while (t.s < s_end && !((dmask >> t.kd) & 1)) {
            t.s += ncc - t.cc; t.cc = 0;
            next_tap(t);
        }
        if (t.s >= s_end) t.s = nsteps;
        return t;
    };
    auto next_of = [&](TStep t) -> TStep {
        ++t.s;
        if (++t.cc < ncc) {
            if (t.s >= s_end) t.s = nsteps;
            return t;
        }
        t.cc = 0;
        next_tap(t);
        return settle(t);
    };

    float4 ra[8];
    uint4 rb0, rb1;
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    unsigned valid_mask = 0;
    auto issue_loads = [&](const TStep& t) {
        const int tap = (t.kd * g.KH + t.kh) * g.KW + t.kw;
        const int c = t.cc * BK + piece * 4;
        const bool cok = c < g.Cin;
        const int soff = tap_delta(g, t.kd, t.kh, t.kw, 0) + t.cc * BK;
        const int tbits = cok ? tap_bits(t.kd, t.kh, t.kw) : 0x7fffffff;     // channels beyond Cin: nothing valid
        valid_mask = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const bool ok = (rows[p].mask & tbits) == tbits;
            const int off = ok ? rows[p].off + soff : 0;                       // branch-free: invalid rows read element 0
            ra[p] = *reinterpret_cast<const float4*>(in + off);
            valid_mask |= ok ? (1u << p) : 0u;
        }
        if (XF) {
            const int cs = cok ? c : 0;
            tsc = *reinterpret_cast<const float4*>(in_bn + cs);
            tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cs);
        }
        // W slab: 8 groups of 8 k x 64 columns, 16 B each -> two per thread
        const uint4* wl = wp + (size_t)(tap * KpG + t.cc * (BK / 8) + (tid >> 6)) * g.CoutP + n0 + (tid & 63);
        rb0 = wl[0];
        rb1 = wl[(size_t)4 * g.CoutP];
    };
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    auto store_lds = [&]() {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            float4 v = ra[p];
            const bool ok = (valid_mask >> p) & 1;
            if (XF) {
                v.x = ok ? fmaxf(fmaf(v.x, tsc.x, tsh.x), relu_lo) : 0.f;
                v.y = ok ? fmaxf(fmaf(v.y, tsc.y, tsh.y), relu_lo) : 0.f;
                v.z = ok ? fmaxf(fmaf(v.z, tsc.z, tsh.z), relu_lo) : 0.f;
                v.w = ok ? fmaxf(fmaf(v.w, tsc.w, tsh.w), relu_lo) : 0.f;
            } else {
                v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            }
            *reinterpret_cast<bf16x4*>(sA + (p * 16 + (tid >> 4)) * kRowBytes + piece * 8) = to_bf16(v);
        }
        uint4* bl = reinterpret_cast<uint4*>(sB) + tid;
        bl[0] = rb0;
        bl[4 * BN] = rb1;
    };

    f32x16 acc0 = {0}, acc1 = {0};
    // fragment of k step ks (16 k): A row (wave * 32 + lane & 31), bytes 32 ks + 16 (lane >> 5); B group 2 ks + (lane >> 5)
    const unsigned char* aRow = sA + (wave * 32 + (lane & 31)) * kRowBytes + 16 * (lane >> 5);
    const unsigned char* bCol = sB + ((lane >> 5) * BN + (lane & 31)) * 16;

    TStep cur;
    {
        const int tap = s_begin / ncc, hw = tap / g.KW;
        cur.s = s_begin; cur.cc = s_begin - tap * ncc; cur.kw = tap - hw * g.KW; cur.kd = hw / g.KH; cur.kh = hw - cur.kd * g.KH;
        cur = settle(cur);
    }
    if (cur.s < nsteps) {
        issue_loads(cur);
        store_lds();
    }
    __syncthreads();
    while (cur.s < nsteps) {
        const TStep nxt = next_of(cur);
        if (nxt.s < nsteps) issue_loads(nxt);
        // fragments of two k steps at a time (24 registers): all four at once spill under the 128-register budget
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            bf16x8 a[2], b0[2], b1[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ks = kh * 2 + k;
                a[k] = *reinterpret_cast<const bf16x8*>(aRow + ks * 32);
                b0[k] = *reinterpret_cast<const bf16x8*>(bCol + ks * 2 * BN * 16);
                b1[k] = *reinterpret_cast<const bf16x8*>(bCol + ks * 2 * BN * 16 + 32 * 16);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[k], b0[k], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[k], b1[k], acc1, 0, 0, 0);
            }
        }
        __syncthreads();
        if (nxt.s < nsteps) store_lds();
        __syncthreads();
        cur = nxt;
    }
    if (nsplit > 1 &&
        !splitk_arrive<false>(acc0, acc1, partial, nsplit, blockIdx.x * gridDim.y + blockIdx.y, gridDim.x * gridDim.y, wave, lane))
        return;
    // ---- epilogue: C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -------------
    const int col = lane & 31;
    const int nA = n0 + col, nB = n0 + 32 + col;
    const float biasA = (bias && nA < g.Cout) ? bias[nA] : 0.f;
    const float biasB = (bias && nB < g.Cout) ? bias[nB] : 0.f;
    const bool orelu = (flags & LISEC_CONV_OUT_RELU) != 0;
    const int mw = m0 + wave * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M) continue;
        float* o = out + (size_t)m * g.out_stride;
        float va = acc0[r] + biasA, vb = acc1[r] + biasB;
        if (orelu) { va = fmaxf(va, 0.f); vb = fmaxf(vb, 0.f); }
        if (nA < g.Cout) o[nA] = va;
        if (nB < g.Cout) o[nB] = vb;
    }
}

// dst[tap][k / 8][n][k % 8] bf16 (K and N zero padded to 64), RNE from an arbitrarily strided fp32 source
__global__ void k_pack_weights_bf16(const float* __restrict__ src, int ntaps, int K, int N, long long tap_stride,
                                    long long k_stride, long long n_stride, int Kp, int Np, bf16x8* __restrict__ dst) {
    const long long total = (long long)ntaps * (Kp / 8) * Np;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long t = i;
        const int n = (int)(t % Np);
        t /= Np;
        const int kg = (int)(t % (Kp / 8));
        const int tap = (int)(t / (Kp / 8));
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = kg * 8 + j;
            v[j] = (__bf16)((k < K && n < N) ? src[tap * tap_stride + k * k_stride + n * n_stride] : 0.f);
        }
        dst[i] = v;
    }
}

struct Bf16Plan {
    ConvGeom g;
    int ntiles, nnb, nsplit;
    size_t ws_bytes;
};

// K slices: a layer with fewer than one workgroup per CU is cut until ~3 workgroups per CU exist, no slice shorter than
// three steps; the workspace on offer caps the count (a smaller workspace only means fewer slices, never another path)
int plan_bf16(const lisec_conv_geom* c, size_t workspace_bytes, bool sizing, Bf16Plan* p) {
    ConvGeom& g = p->g;
    if (int rc = conv_geom_check(c, &g)) return rc;
    LISEC_CHECK_ARG(c->mode == 0, "the bf16 kernel is forward only (mode 0)");
    LISEC_CHECK_ARG(!c->ps, "the bf16 kernel has no pixel-shuffle store");
    p->ntiles = cdiv(g.M, BM);
    p->nnb = g.CoutP / BN;
    p->nsplit = 1;
    p->ws_bytes = 0;
    const int nsteps = g.KD * g.KH * g.KW * cdiv(g.Cin, BK);
    const long long blocks = (long long)p->ntiles * p->nnb;
    const int cus = cu_count();
    if (blocks >= cus || blocks > kSplitCounters) return 0;
    int ns = (int)(3LL * cus / blocks);
    if (ns > nsteps / 3) ns = nsteps / 3;
    if (ns > kMaxSlices) ns = kMaxSlices;
    auto bytes = [&](int n) { return align_up(sizeof(int) * kSplitCounters + sizeof(float) * (size_t)n * blocks * BM * BN, 256); };
    if (!sizing)
        while (ns >= 2 && bytes(ns) > workspace_bytes) --ns;
    if (ns < 2) return 0;
    p->nsplit = ns;
    p->ws_bytes = bytes(ns);
    return 0;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_conv_packed_bf16_bytes(int ntaps, int K, int N) {
    if (ntaps <= 0 || K <= 0 || N <= 0) return 0;
    return (size_t)ntaps * align_up(K, 64) * align_up(N, 64) * 2;
}

extern "C" int lisec_conv_pack_weights_bf16(const float* src, int ntaps, int K, int N, long long tap_stride,
                                            long long k_stride, long long n_stride, void* dst, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(src && dst && ntaps > 0 && K > 0 && N > 0, "bad pack arguments");
    LISEC_CHECK_ARG(((uintptr_t)dst & 15) == 0, "packed bf16 weights must be 16-byte aligned");
    const int Kp = (int)align_up(K, 64), Np = (int)align_up(N, 64);
    const long long total = (long long)ntaps * (Kp / 8) * Np;
    int gb = cdiv(total, 256);
    if (gb > 8192) gb = 8192;
    LISEC_LAUNCH(k_pack_weights_bf16, dim3(gb), dim3(256), 0, static_cast<hipStream_t>(stream_), src, ntaps, K, N,
                 tap_stride, k_stride, n_stride, Kp, Np, static_cast<bf16x8*>(dst));
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" size_t lisec_conv_forward_bf16_workspace_bytes(const lisec_conv_geom* c) {
    Bf16Plan p;
    if (plan_bf16(c, 0, true, &p)) return 0;
    return p.ws_bytes;
}

extern "C" int lisec_conv_forward_bf16(const lisec_conv_geom* c, const float* in, const void* packed_bf16, float* out,
                                       const float* bias, const float* in_bnstate, int flags, void* workspace,
                                       size_t workspace_bytes, lisec_stream_t stream_) {
    Bf16Plan p;
    if (int rc = plan_bf16(c, workspace ? workspace_bytes : 0, false, &p)) return rc;
    const ConvGeom& g = p.g;
    LISEC_CHECK_ARG(in && packed_bf16 && out, "NULL tensor pointer");
    LISEC_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)packed_bf16 & 15) == 0, "in/weights must be 16-byte aligned");
    LISEC_CHECK_ARG((flags & ~(LISEC_CONV_IN_RELU | LISEC_CONV_OUT_RELU)) == 0,
                    "the bf16 kernel takes LISEC_CONV_IN_RELU and LISEC_CONV_OUT_RELU only");
    LISEC_CHECK_ARG(!in_bnstate || ((uintptr_t)in_bnstate & 15) == 0, "in_bnstate must be 16-byte aligned");
    LISEC_CHECK_ARG(!(flags & LISEC_CONV_IN_RELU) || in_bnstate, "LISEC_CONV_IN_RELU needs the producing layer's in_bnstate");
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(p.ntiles, p.nnb, p.nsplit);
    const size_t lds = kABytes + kBBytes;
    const uint4* w = static_cast<const uint4*>(packed_bf16);
    float* partial = p.nsplit > 1 ? static_cast<float*>(workspace) : nullptr;
    if (in_bnstate)
        LISEC_LAUNCH(k_igemm_bf16<true>, grid, dim3(kThreads), lds, st, g, in, w, bias, in_bnstate, flags, out, p.nsplit, partial);
    else
        LISEC_LAUNCH(k_igemm_bf16<false>, grid, dim3(kThreads), lds, st, g, in, w, bias, in_bnstate, flags, out, p.nsplit, partial);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
