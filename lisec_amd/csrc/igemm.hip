// Implicit-GEMM convolution on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
// One kernel family serves every dense contraction of the network
//   Conv3D  (model_training.py:193)     Conv2D (:203)      Conv2DTranspose (:246,:249,:252)
//   Dense on the last axis (:184,:195)  1x1 heads (:254-255)
// and their data gradients, as   out[m, n] = sum_tap sum_c  A_tap[m, c] * W[tap][c][n]  (+ bias)
// with A_tap[m, :] = f(in[src(m, tap), :]) gathered on the fly (never an im2col buffer):
//   mode 0 (conv):            src = o*stride - pad + k          (ZeroPadding + 'valid')
//   mode 1 (transposed conv): src = (o + pad - k) / stride      when divisible and in range
// f is an optional per-channel affine (+ReLU): the BatchNormalization(+ReLU) of the PRODUCING
// layer is applied while the tile is staged, so normalised activations are never written to HBM.
//
// Tiling (per 256-thread workgroup = 4 waves, one per SIMD): 128 output positions x 64 output
// channels; every wave owns 32 x 64 = two 32x32 MFMA accumulators.  Per (tap, 64-channel slab):
//   A slab 128 x 64 fp32 -> LDS rows padded to 68 floats (conflict-free ds_read_b128 fragments)
//   W slab  64 x 64 fp32 -> LDS in the packed [k/4][n][4] order (linear copy, conflict-free)
//   64 MFMAs per wave (4096 SIMD cycles at the 64-cycle issue rate of the f32 MFMA).
// The next slab is prefetched into registers while the MFMAs run and written to LDS between two
// barriers (single LDS buffer, 51 KB => 3 workgroups per CU cover each other's staging).
// The tile height is a template parameter TM of igemm_tile / halo_tile / store_tile: 128 as above, or 64 (k_igemm_small, below)
// for the K-sliced layers of few tiles -- one 32 x 32 accumulator per wave, two double-buffered workgroups per CU.
// fp32 in / fp32 accumulate: bit-for-bit an fmaf chain, so parity with the fp32 oracle holds to
// summation-order noise (no reduced precision anywhere).
// Where the pieces live: this file holds the kernels' step walkers, staging maps, the epilogue (store_tile) and the host
// side (plan_conv and the launch list); tile_parts.h the on-load transforms of a staged float4 (affine_relu, bn_fold), the
// W-slab copy (wslab_load / wslab_store) and the 64-deep MFMA step (mfma_step64), shared with wgrad.hip; splitk.h the
// meeting of the K slices (slab_store, slice_ticket, slab_sum; splitk_arrive for a tile); conv.h the gather geometry.
#include "conv.h"
#include "tile_parts.h"


namespace lisec {
namespace {

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int LDA = 68;                          // padded A row (floats)
constexpr int kThreads = 256;
constexpr int A_FLOATS = BM * LDA;               // 8704
constexpr int B_FLOATS = BK * BN;                // 4096

// diagnostic (tools/igemm_stamps.py): 100 MHz s_memrealtime stamps of thread 0 of every workgroup of k_igemm_halo at its
// phase boundaries; nullptr (the default) = no stamp executes
__device__ unsigned long long* g_igemm_stamps = nullptr;
#define IGEMM_STAMP(K_)                                                                                    \
    do {                                                                                                   \
        if (stamps && threadIdx.x == 0 && stamp_wg < 8192) {                                               \
            stamps[(size_t)stamp_wg * 8 + (K_)] = __builtin_amdgcn_s_memrealtime();                        \
            if ((K_) == 0)   /* where the workgroup runs: HW_ID (wave, simd, cu, sh, se) | XCC_ID << 32 */  \
                stamps[(size_t)stamp_wg * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | \
                                                   ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
        }                                                                                                  \
    } while (0)

// Epilogue shared by the igemm kernels: bias (+accumulate, output gate, ReLU) store with the per-tile BatchNormalization
// partial sums.  C layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
// mw: first of the 32 rows this wave holds; storer: false for a wave that holds no rows of its own -- it only takes part
// in the statistics reduction, with zeros.
// TM = 64 (the 64 x 64 tile): wave w holds ONE accumulator, rows mw = m0 + (w & 1) * 32 .. and columns n0 + (w >> 1) * 32 ..;
// acc1 is not read.  The fp32 partial per 32-row group is what it is for TM = 128; the fp64 sum above it adds the two row
// halves of a column block -- and, under a sink, the two 64-row tiles of one 128-row tile MEET (pair_ws: the workspace whose
// head holds the counters, pair_buf: 256 floats per workgroup) so that the sink receives the addend the 128-row tile would
// have sent, ((r0 + r1) + r2) + r3 in fp64 over its four 32-row groups: the fixed-point sink rounds every addend to 2^-40,
// and a gradient's sums are small enough for two addends to round differently from one.  The first tile of a pair to finish
// leaves its two fp32 partials per column (sc1 stores, wait, barrier, one agent-scope add: the hand-off of splitk_arrive), the
// second one reads them (sc1), sums in row order and adds; both take their sink ticket.  A tile without a partner (the
// last 64 rows of an odd count) adds alone: the missing groups are the zeros of the 128-row tile's rows beyond M.
constexpr int kPairCounter0 = 2048;              // pair counters: the upper half of the workspace's kSplitCounters
template <int TM = 128>
__device__ __forceinline__ void store_tile(const ConvGeom& g, const f32x16& acc0, const f32x16& acc1, float* smem,
                                           int mw, int n0, int mb, int mlimit, int wave, int lane, int tid,
                                           const float* __restrict__ bias, int flags, float* __restrict__ out,
                                           double* __restrict__ stats, bool storer = true, bool half = false,
                                           int phase = 0, float* lds_tile = nullptr, float* pair_ws = nullptr,
                                           float* pair_buf = nullptr) {
    // phase (calls with g.tail_w): 1 = the gated first output, no statistics, the stored values also go to lds_tile
    // ([128][LDA], the A operand of the tail contraction); 2 = the tail's output: no gate, the backward statistics
    // half: the workgroup computed a 32-column slab (acc1 is unused): the second 32 columns are treated as outside Cout
    const int col = lane & 31;
    const int nA = n0 + (TM == 64 ? (wave >> 1) * 32 : 0) + col, nB = half || TM == 64 ? g.Cout : n0 + 32 + col;
    // pixel-shuffle store (kernel == stride transposed conv): the 64-column slab lies inside one tap
    const int ps_tap = g.ps ? n0 / g.ps_channels : 0;
    const int ps_kh = g.ps ? ps_tap / g.ps : 0, ps_kw = g.ps ? ps_tap - ps_kh * g.ps : 0;
    const int ncA = g.ps ? nA - ps_tap * g.ps_channels : nA, ncB = g.ps ? nB - ps_tap * g.ps_channels : nB;
    // parity-class order: decode the wave's first row once
    int pc_c = 0, pc_q = 0, pc_i = 0, pc_j = 0;
    if (g.pc_span) {
        pc_c = mw / g.pc_span;
        pc_q = mw - pc_c * g.pc_span;
        pc_i = pc_q / (g.Wo >> 1);
        pc_j = pc_q - pc_i * (g.Wo >> 1);
    }
    // BatchNormalization-backward statistics: per-column constants of the layer the gradient belongs to
    float ysA = 1.f, yhA = 0.f, ymA = 0.f, yiA = 0.f, ysB = 1.f, yhB = 0.f, ymB = 0.f, yiB = 0.f;
    const float* bwd_y = phase == 1 ? nullptr : g.bwd_y;
    const float* omask = phase == 2 ? nullptr : g.out_mask;
    if (bwd_y) {
        if (nA < g.Cout) { ysA = g.bwd_bn[nA]; yhA = g.bwd_bn[g.Cout + nA]; ymA = g.bwd_bn[2 * g.Cout + nA]; yiA = g.bwd_bn[3 * g.Cout + nA]; }
        if (nB < g.Cout) { ysB = g.bwd_bn[nB]; yhB = g.bwd_bn[g.Cout + nB]; ymB = g.bwd_bn[2 * g.Cout + nB]; yiB = g.bwd_bn[3 * g.Cout + nB]; }
    }
    const float biasA = (bias && nA < g.Cout) ? bias[ncA] : 0.f;
    const float biasB = (bias && nB < g.Cout) ? bias[ncB] : 0.f;
    const bool orelu = (flags & LISEC_CONV_OUT_RELU) != 0, accum = (flags & LISEC_CONV_ACCUMULATE) != 0;
    float sumA = 0.f, sqA = 0.f, sumB = 0.f, sqB = 0.f;
    // Backward statistics on a plain row order: the rows of y this wave needs are requested BEFORE the first store.  Read
    // inside the store loop each of them waited behind the stores in front of it (`out` may alias y for all the compiler
    // knows, and the memory pipeline returns in order): 16 dependent round trips per tile
    const bool y_ahead = bwd_y && !g.pc_span && !g.ps;
    float yA[16], yB[16];
    if (y_ahead) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const float* yr = bwd_y + (size_t)(m < mlimit ? m : 0) * g.Cout;
            yA[r] = nA < g.Cout ? yr[nA] : 0.f;
            yB[r] = nB < g.Cout ? yr[nB] : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int m = mw + row;
        bool live_row = storer && m < mlimit;
        size_t orow = (size_t)m;
        if (g.pc_span && live_row) {
            // parity-class order: q = q0 + row with q0 decoded once per wave (row < 32 <= Wo/2: at most one line wrap)
            int j = pc_j + row, i = pc_i;
            if (j >= (g.Wo >> 1)) { j -= g.Wo >> 1; ++i; }
            live_row = pc_q + row < g.pc_rows;
            orow = (size_t)(2 * i + (pc_c >> 1)) * g.Wo + 2 * j + (pc_c & 1);
        }
        if (live_row) {
            if (g.ps) {
                const int h = m / g.Wo, w = m - h * g.Wo;
                orow = (size_t)(h * g.ps + ps_kh) * (g.Wo * g.ps) + (w * g.ps + ps_kw);
            }
            float* o = out + orow * g.out_stride;
            float va = acc0[r] + biasA, vb = acc1[r] + biasB;
            if (accum) {
                if (nA < g.Cout) va += o[ncA];
                if (nB < g.Cout) vb += o[ncB];
            }
            if (omask) {
                const float* mk = omask + orow * g.out_stride;
                if (nA < g.Cout && !(mk[ncA] > 0.f)) va = 0.f;
                if (nB < g.Cout && !(mk[ncB] > 0.f)) vb = 0.f;
            }
            if (orelu) { va = fmaxf(va, 0.f); vb = fmaxf(vb, 0.f); }
            if (nA < g.Cout) o[ncA] = va;
            if (nB < g.Cout) o[ncB] = vb;
            if (lds_tile) { lds_tile[(wave * 32 + row) * LDA + col] = va; lds_tile[(wave * 32 + row) * LDA + 32 + col] = vb; }
            if (bwd_y) {
                // (sum dz, sum dz * yhat) of the gradient just stored, for the BatchNormalization it is about to cross
                const float* yr = bwd_y + orow * g.Cout;
                const float ya = y_ahead ? yA[r] : (nA < g.Cout ? yr[nA] : 0.f), yb = y_ahead ? yB[r] : (nB < g.Cout ? yr[nB] : 0.f);
                const float da = (g.bwd_relu && !(fmaf(ya, ysA, yhA) > 0.f)) || nA >= g.Cout ? 0.f : va;
                const float db = (g.bwd_relu && !(fmaf(yb, ysB, yhB) > 0.f)) || nB >= g.Cout ? 0.f : vb;
                sumA += da; sqA = fmaf(da, (ya - ymA) * yiA, sqA);
                sumB += db; sqB = fmaf(db, (yb - ymB) * yiB, sqB);
            } else {
                sumA += va; sqA = fmaf(va, va, sqA);
                sumB += vb; sqB = fmaf(vb, vb, sqB);
            }
        } else if (lds_tile) {
            lds_tile[(wave * 32 + row) * LDA + col] = 0.f; lds_tile[(wave * 32 + row) * LDA + 32 + col] = 0.f;
        }
    }
    if (phase != 1 && (stats || g.sink.acc)) {
        // per-channel partial sums of this 128-row tile (BatchNormalization batch statistics)
        __syncthreads();
        float* red = smem;                       // [4 waves][4][32]
        sumA += __shfl_xor(sumA, 32, 64); sqA += __shfl_xor(sqA, 32, 64);
        sumB += __shfl_xor(sumB, 32, 64); sqB += __shfl_xor(sqB, 32, 64);
        if (lane < 32) {
            red[(wave * 4 + 0) * 32 + lane] = sumA; red[(wave * 4 + 1) * 32 + lane] = sqA;
            red[(wave * 4 + 2) * 32 + lane] = sumB; red[(wave * 4 + 3) * 32 + lane] = sqB;
        }
        __syncthreads();
        if (TM == 64) {
            const int q = tid >> 5, c = tid & 31;            // (tid < 128) q: 0 sum, 1 sq of columns 0-31; 2, 3 of columns 32-63
            const int w0 = q & 2;                            // column block q >> 1 is held by waves (q & 2) and (q & 2) + 1
            float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;    // the two 32-row groups of this tile / of the other half of its 128 rows
            const int hf = mb & 1;
            if (tid < 128) { a0 = red[(w0 * 4 + (q & 1)) * 32 + c]; a1 = red[((w0 + 1) * 4 + (q & 1)) * 32 + c]; }
            bool add = true;
            if (g.sink.acc && pair_ws && (mb ^ 1) * 64 < g.M) {          // (workgroup-uniform)
                __shared__ int pair_second;
                const int slot = (mb >> 1) * gridDim.y + blockIdx.y;
                int* counter = reinterpret_cast<int*>(pair_ws) + kPairCounter0 + slot;
                float* mine = pair_buf + ((size_t)slot * 2 + hf) * 256;
                const float* theirs = pair_buf + ((size_t)slot * 2 + (hf ^ 1)) * 256;
                if (tid < 128) {
                    __hip_atomic_store(mine + tid, a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(mine + 128 + tid, a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) pair_second = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __syncthreads();
                add = pair_second == 1;
                if (add) {
                    if (tid == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (tid < 128) {
                        b0 = __hip_atomic_load(theirs + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        b1 = __hip_atomic_load(theirs + 128 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            if (add && tid < 128) {
                double v = 0.0;                              // row order, as the 128-row tile sums its four groups
                v += (double)(hf ? b0 : a0); v += (double)(hf ? b1 : a1); v += (double)(hf ? a0 : b0); v += (double)(hf ? a1 : b1);
                const int n = n0 + (q >> 1) * 32 + c;
                if (n < g.Cout) {
                    if (g.sink.acc) sink_add(g.sink, q & 1, n, v);
                    else stats[((size_t)mb * 2 + (q & 1)) * g.Cout + n] = v;
                }
            }
        } else if (tid < 128) {
            const int q = tid >> 5, c = tid & 31;            // q: 0 sumA, 1 sqA, 2 sumB, 3 sqB
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += (double)red[(k * 4 + q) * 32 + c];
            const int n = (half && q >= 2) ? g.Cout : n0 + (q >> 1) * 32 + c;
            if (n < g.Cout) {
                if (g.sink.acc) sink_add(g.sink, q & 1, n, v);
                else stats[((size_t)mb * 2 + (q & 1)) * g.Cout + n] = v;
            }
        }
        if (g.sink.acc) sink_finish(g.sink);
    }
}

// NW: columns per workgroup, 64 or 32.  32 (one accumulator per wave, half a W slab) is what a layer of 160-380 tiles
// runs instead of two K slices + a combine launch: twice the workgroups, every one over the whole K.
// DB: two LDS images (A tile + W slab each, 102 KB together: one workgroup per CU).  The loads of step s + 2 are in flight
// and the image of step s + 1 is written while the MFMAs of step s read the other image: ONE barrier per step and nothing
// between the MFMA runs but the stores' issue slots.  For launches of at most one workgroup per CU (the K-sliced 1 250- and
// 5 000-position RPN maps), where no second workgroup covers the store -> barrier -> fragment-read sequence of the
// single-image loop (2.65-2.9 us per step against 1.7 us of MFMA time, tools/rpn_stamps.py).
// FOLD: the gathered operand is a gradient about to cross a BatchNormalization(+ReLU) backwards: the apply pass of that
// backward -- dy = scale (gate(y) g - mean(dz) - yhat mean(dz yhat)), k_bn_bwd_apply -- runs on load, from g (`in`), the
// layer's raw output y (g.in_y, same layout) and the per-channel constants (g.fold_bn = its bnstate, g.fold_coef = the
// backward sink's means): the chain of data gradients of the RPN no longer stops for a launch between every two of them.
template <int MODE, bool XF, int NW = 64, bool DB = false, bool FOLD = false, int TM = BM>
__device__ __forceinline__ void
igemm_tile(const ConvGeom& g, const float* __restrict__ in, const float* __restrict__ wp,
           const float* __restrict__ bias, const float* __restrict__ in_bn, int flags,
           float* __restrict__ out, double* __restrict__ stats, int nsplit, float* __restrict__ partial, int tile0,
           int mb, float* smem, unsigned long long* stamps, unsigned stamp_wg) {
    static_assert(TM == 128 || (TM == 64 && NW == 64), "tile height");
    constexpr int TA_FLOATS = TM * LDA, NP = TM / 16;          // A image; staged rows per thread
    constexpr bool TWO = NW == 64 && TM == 128;                // two accumulators per wave
    float* sA = smem;
    float* sB = smem + TA_FLOATS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = mb * TM;
    const int n0 = blockIdx.y * NW;
    const int mlimit = row_limit(g);
    if (m0 >= mlimit) return;                     // row list shorter than its capacity (whole workgroup)
    const int HW = g.Ho * g.Wo;

    // ---- rows this thread stages: r = p*16 + tid/16, 16-byte piece tid%16 ----------------------
    const int piece = tid & 15;
    RowGather rows[NP];
    int tile_mask = 0;
    {
        // each gather descriptor is computed ONCE (thread r < 128 owns row r: two integer divisions + three axis masks) and
        // handed to the 16 threads that stage that row through LDS, instead of 8 descriptors per thread
        int2* shared_rows = reinterpret_cast<int2*>(smem);
        int* tile_or = reinterpret_cast<int*>(shared_rows + TM);     // OR of the rows' validity bits
        if (g.row_coords) {                                          // (wave-uniform branch)
            if (tid == 0) *tile_or = 0;
            __syncthreads();
        }
        if (tid < TM) {
            const RowGather r = row_gather(g, m0 + tid, MODE, 0);
            shared_rows[tid] = make_int2(r.off, r.mask);
            if (g.row_coords && r.mask) atomicOr(tile_or, r.mask);
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int2 v = shared_rows[p * 16 + (tid >> 4)];
            rows[p].off = v.x + piece * 4;
            rows[p].mask = v.y;
        }
        if (g.row_coords) tile_mask = *tile_or;
        __syncthreads();
    }
    // tile-uniform depth range for whole-tap skipping
    const int mlast = (m0 + TM - 1 < g.M ? m0 + TM - 1 : g.M - 1);
    const int d_first = g.pc_span ? 0 : m0 / HW, d_last = g.pc_span ? 0 : mlast / HW;
    int dmask_first;
    {
        int tmp;
        dmask_first = axis_mask(d_first, g.KD, g.ls_d, g.pd, g.Di, MODE, tmp);
    }

    const int ncc = (g.Cin + BK - 1) / BK;
    const int ntaps = g.KD * g.KH * g.KW;
    const int nsteps = ntaps * ncc;
    const int KpQ = ncc * (BK / 4);              // packed K quads per tap

    const int pclass = g.pc_span ? m0 / g.pc_span : 0;           // tile-uniform parity class (h & 1) * 2 + (w & 1)
    // A K step is (tap, channel slab); the walk over the step list is kept as (kd, kh, kw, cc) counters that advance by
    // increments -- a lone wave per SIMD pays every scalar instruction of a step in full, and the integer divisions of a
    // step number (no hardware divide: ~25 instructions each) were half of the non-MFMA work of a step.
    struct TStep { int s, kd, kh, kw, cc; };
    auto tap_live = [&](const TStep& t) -> bool {
        if (g.pc_span)                                           // stride 2 along h and w: only taps of the right parity divide
            return (((pclass >> 1) + g.ph - t.kh) & 1) == 0 && (((pclass & 1) + g.pw - t.kw) & 1) == 0;
        if (g.row_coords) {
            // row list (voxels sorted by cell, so a tile mostly shares z and its parity): a tap none of whose axis bits
            // is set in ANY row of the tile reads nothing -- conservative (per-axis OR), never skips a live tap
            const int tb = tap_bits(t.kd, t.kh, t.kw);
            return (tile_mask & tb) == tb;
        }
        if (d_first != d_last) return true;
        return (dmask_first >> t.kd) & 1;
    };

    float4 ra[NP];
    float4 ry[FOLD ? NP : 1];
    float4 fmu = make_float4(0, 0, 0, 0), fis = fmu, fm1 = fmu, fm2 = fmu;     // FOLD: mean, 1/std, mean(dz), mean(dz yhat)
    float4 rb0, rb1, rb2, rb3;
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    unsigned valid_mask = 0;

    auto issue_loads = [&](const TStep& t) {
        const int kd = t.kd, kh = t.kh, kw = t.kw, cc = t.cc;
        const int tap = (kd * g.KH + kh) * g.KW + kw;
        const int c = cc * BK + piece * 4;
        const bool cok = c < g.Cin;
        const int soff = tap_delta(g, kd, kh, kw, MODE) + cc * BK;     // wave-uniform
        const int tbits = cok ? tap_bits(kd, kh, kw) : 0x7fffffff;      // channel slab beyond Cin: nothing valid
        valid_mask = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool ok = (rows[p].mask & tbits) == tbits;
            const int off = ok ? rows[p].off + soff : 0;                // branch-free: invalid rows read element 0
            ra[p] = *reinterpret_cast<const float4*>(in + off);
            if (FOLD) ry[p] = *reinterpret_cast<const float4*>(g.in_y + off);
            valid_mask |= ok ? (1u << p) : 0u;
        }
        if (FOLD) {
            const int cs = cok ? c : 0;
            tsc = *reinterpret_cast<const float4*>(g.fold_bn + cs);
            tsh = *reinterpret_cast<const float4*>(g.fold_bn + g.Cin + cs);
            fmu = *reinterpret_cast<const float4*>(g.fold_bn + 2 * g.Cin + cs);
            fis = *reinterpret_cast<const float4*>(g.fold_bn + 3 * g.Cin + cs);
            fm1 = *reinterpret_cast<const float4*>(g.fold_coef + cs);
            fm2 = *reinterpret_cast<const float4*>(g.fold_coef + g.Cin + cs);
        }
        if (XF) {
            // unconditional (in_bn is never NULL here, see lisec_conv_forward_ex): with these two loads under a branch the
            // compiler sizes its s_waitcnt for the shorter path and every step waits for its first A loads before the MFMAs
            const int cs = cok ? c : 0;
            tsc = *reinterpret_cast<const float4*>(in_bn + cs);
            tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cs);
        }
        const float* wb = wp + ((size_t)(tap * KpQ + cc * (BK / 4)) * g.CoutP + n0) * 4;
        wslab_load<NW>(wb, g.CoutP, tid, rb0, rb1, rb2, rb3);
    };
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    auto store_lds = [&]() {
        // branch-free: without an affine tsc = 1, tsh = 0 (x*1 + 0 is exact); padding stays 0
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float4 v = ra[p];
            const bool ok = (valid_mask >> p) & 1;
            if (FOLD) bn_fold(v, ry[p], tsc, tsh, fmu, fis, fm1, fm2, g.fold_relu, ok);
            else if (XF) affine_relu(v, tsc, tsh, relu_lo, ok);
            else masked(v, ok);
            *reinterpret_cast<float4*>(sA + (p * 16 + (tid >> 4)) * LDA + piece * 4) = v;
        }
        wslab_store<NW>(sB, tid, rb0, rb1, rb2, rb3);
    };

    f32x16 acc0 = {0}, acc1 = {0};
    // TM = 64: wave w owns rows (w & 1) * 32 .. and columns (w >> 1) * 32 .. of the 64-column W slab
    const int aoff = ((TM == 64 ? wave & 1 : wave) * 32 + (lane & 31)) * LDA + 4 * (lane >> 5);
    const int boff = ((lane >> 5) * NW + (TM == 64 ? (wave >> 1) * 32 : 0) + (lane & 31)) * 4;
    const float* aRow = sA + aoff;
    const float* bCol = sB + boff;

    // split-K: slice z of the (tap, channel-slab) step list; slices write raw partial tiles
    const int s_end = nsplit > 1 ? (int)(((long long)(blockIdx.z + 1) * nsteps) / nsplit) : nsteps;
    const int s_begin = nsplit > 1 ? (int)(((long long)blockIdx.z * nsteps) / nsplit) : 0;
    auto next_tap = [&](TStep& t) {
        if (++t.kw == g.KW) {
            t.kw = 0;
            if (++t.kh == g.KH) { t.kh = 0; ++t.kd; }
        }
    };
    auto settle = [&](TStep t) -> TStep {           // the first live step at or after t, nsteps when the slice has none left
        while (t.s < s_end && !tap_live(t)) {        // a dead tap goes with all its channel slabs
            t.s += ncc - t.cc; t.cc = 0;
            next_tap(t);
        }
        if (t.s >= s_end) t.s = nsteps;
        return t;
    };
    auto next_of = [&](TStep t) -> TStep {
        ++t.s;
        if (++t.cc < ncc) {                          // same tap: live
            if (t.s >= s_end) t.s = nsteps;
            return t;
        }
        t.cc = 0;
        next_tap(t);
        return settle(t);
    };
    TStep cur;
    {
        const int tap = s_begin / ncc, hw = tap / g.KW;          // the only divisions of a step number: once per tile
        cur.s = s_begin; cur.cc = s_begin - tap * ncc; cur.kw = tap - hw * g.KW; cur.kd = hw / g.KH; cur.kh = hw - cur.kd * g.KH;
        cur = settle(cur);
    }
    IGEMM_STAMP(1);
    TStep nxt = cur;
    nxt.s = nsteps;
    if (cur.s < nsteps) {
        issue_loads(cur);
        store_lds();
        if (DB) {
            nxt = next_of(cur);
            if (nxt.s < nsteps) issue_loads(nxt);
        }
    }
    __syncthreads();
    IGEMM_STAMP(2);
    int stamp_steps = 0, img = 0;
    constexpr int IMG = TA_FLOATS + B_FLOATS;
    while (cur.s < nsteps) {
        ++stamp_steps;
        if (DB) {
            // image of step nxt -> the OTHER image (its loads went out a step ago); then the loads of the step after it
            sA = smem + (img ^ 1) * IMG; sB = sA + TA_FLOATS;
            TStep nn = nxt;
            if (nxt.s < nsteps) {
                store_lds();
                nn = next_of(nxt);
                if (nn.s < nsteps) issue_loads(nn);
            }
            aRow = smem + img * IMG + aoff; bCol = smem + img * IMG + TA_FLOATS + boff;
            img ^= 1;
            cur = nxt; nxt = nn;
        } else {
            nxt = next_of(cur);
            if (nxt.s < nsteps) issue_loads(nxt);
        }
        mfma_step64<TWO, NW>(aRow, bCol, acc0, acc1);
        __syncthreads();
        if (!DB) {
            if (nxt.s < nsteps) store_lds();
            __syncthreads();
            cur = nxt;
        }
    }
    IGEMM_STAMP(3);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)stamp_steps;
    if (nsplit > 1) {
        const bool last = splitk_arrive<DB, TM == 64 ? 4 : 8>(acc0, acc1, partial, nsplit, (mb - tile0) * gridDim.y + blockIdx.y,
                                        gridDim.x * gridDim.y, wave, lane);
        IGEMM_STAMP(7);
        if (!last) { IGEMM_STAMP(4); return; }
    }
    store_tile<TM>(g, acc0, acc1, smem, m0 + (TM == 64 ? wave & 1 : wave) * 32, n0, mb, mlimit, wave, lane, tid, bias, flags, out, stats,
                   true, NW == 32, 0, nullptr, TM == 64 ? partial : nullptr,
                   TM == 64 && partial ? partial + kSplitCounters + (nsplit > 1 ? (size_t)nsplit * gridDim.x * gridDim.y * (64 * 64) : 0) : nullptr);
    IGEMM_STAMP(4);
}

// TAG only changes the symbol name: bench.py launches a layer through k_igemm<.., 1> so that its row in a rocprofv3
// --stats summary is that layer alone (same code as TAG 0).
// k_igemm_queue (row lists over a big capacity, g.queue): 768 resident workgroups that DRAW their tiles from a counter
// instead of owning one each.  The tiles of a row list run 0 / 9 / 18 steps (rows beyond the device-side count, depth
// parity of the voxels) and the dispatcher waits for the CU whose turn it is, so one workgroup per tile kept 3/4 of the
// slots empty (84 000 voxels: starts spread over 183 us, 278 us for 82 us of work).  queue[0] = next tile, queue[1] =
// workgroups that have drawn past the end; the last of those leaves both zero for the next call.
template <int MODE, bool XF, int TAG = 0, int NW = 64, bool DB = false, bool FOLD = false>
__global__ void __launch_bounds__(kThreads)
k_igemm(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp,
        const float* __restrict__ bias, const float* __restrict__ in_bn, int flags,
        float* __restrict__ out, double* __restrict__ stats, int nsplit, float* __restrict__ partial, int tile0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long* stamps = g_igemm_stamps;
    const unsigned stamp_wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    IGEMM_STAMP(0);
    // XCD-aware tile order: consecutive M tiles (which share halo rows) stay on one XCD's L2
    igemm_tile<MODE, XF, NW, DB, FOLD>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial, tile0,
                                 tile0 + xcd_remap(blockIdx.x, gridDim.x), smem, stamps, stamp_wg);
}

// The same tiles DRAWN from a counter by 768 resident workgroups (a kernel of its own: wrapped in the loop the tile code
// needs 60 more registers and drops to two waves per SIMD, which the one-tile-per-workgroup launches must not pay).
template <int MODE, bool XF>
__global__ void __launch_bounds__(kThreads)
k_igemm_queue(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp,
              const float* __restrict__ bias, const float* __restrict__ in_bn, int flags, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int drawn;
    unsigned long long* stamps = g_igemm_stamps;
    const unsigned stamp_wg = blockIdx.x;
    IGEMM_STAMP(0);
    const int ntiles = (row_limit(g) + BM - 1) / BM;              // tiles that hold rows (device-side count)
    for (;;) {
        if (threadIdx.x == 0) drawn = atomicAdd(g.queue, 1);
        __syncthreads();
        const int tile = drawn;
        __syncthreads();                                           // (`drawn` is rewritten by the next draw)
        if (tile >= ntiles) break;
        igemm_tile<MODE, XF>(g, in, wp, bias, in_bn, flags, out, nullptr, 1, nullptr, 0, tile, smem, stamps, stamp_wg);
        __syncthreads();                                           // the epilogue's scratch is the next tile's staging area
    }
    if (threadIdx.x == 0 && atomicAdd(g.queue + 1, 1) == (int)gridDim.x - 1) {
        // every workgroup has drawn its last (out-of-range) index: nobody draws again
        __hip_atomic_store(g.queue, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(g.queue + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// w-halo variant for 3-tap, stride-1, pad-1 contractions along w (Conv3D / Conv2D 3x3 'same' layers and their data
// gradients, Wo >= 126).  The three kw taps of one (kd, kh) pair read the SAME input line shifted by one position, so
// the A tile is staged once per (kd, kh, channel slab) as the tile's line segment(s) plus one halo column on each
// side, and tap kw only moves the fragment base by one LDS row: a third of the global loads, LDS writes and
// BatchNormalization-on-load work of k_igemm per MFMA.  A 128-row tile touches at most NSEG output lines (NSEG = 2 for
// Wo >= 126, 3 for Wo >= 64; narrower maps measured no gain and stay on k_igemm):
//     halo row j <  a + 2 : line L0,     w_in = w0 - 1 + j              (a = rows of the tile on line L0)
//     halo row j >= a + 2 : line L0 + k, w_in = (j - (a + 2)) % (Wo + 2) - 1,   k = 1 + (j - (a + 2)) / (Wo + 2)
// and output row r (on segment k) reads halo row  r + 2k + f(kw),  f = kw (mode 0) or 2 - kw (mode 1).  Zero padding
// in w is simply a zero halo row; the (kd, kh) validity is per line, i.e. wave-uniform.  K slices are whole A tiles.
constexpr int halo_rows(int nseg, int tm = BM) { return tm + 2 * nseg; }     // segments + two halo columns each
constexpr size_t halo_lds_bytes(int nseg, int tm = BM) { return (size_t)(halo_rows(nseg, tm) * LDA + B_FLOATS) * sizeof(float); }   // <= 52 832 B: 3 per CU

template <int MODE, bool XF, int NSEG, int NW = 64, bool DB = false, bool TAIL = false, bool FOLD = false, int TM = BM>
__device__ __forceinline__ void
halo_tile(const ConvGeom& g, const float* __restrict__ in, const float* __restrict__ wp,
          const float* __restrict__ bias, const float* __restrict__ in_bn, int flags,
          float* __restrict__ out, double* __restrict__ stats, int nsplit, float* __restrict__ partial, int tile0,
          int mb, float* smem, unsigned long long* stamps, unsigned stamp_wg) {
    static_assert(TM == 128 || (TM == 64 && NW == 64 && NSEG == 2 && !TAIL), "tile height");
    constexpr int HALO_MAX_ROWS = halo_rows(NSEG, TM);
    constexpr int NP = (HALO_MAX_ROWS + 15) / 16;              // staged halo rows per thread
    constexpr bool TWO = NW == 64 && TM == 128;                // two accumulators per wave
    float* sA = smem;
    float* sB = smem + HALO_MAX_ROWS * LDA;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = mb * TM;
    const int n0 = blockIdx.y * NW;
    const int mlimit = g.M;

    // ---- the (at most NSEG) output lines of this tile ----------------------------------------------
    const int L0 = m0 / g.Wo, w0 = m0 - L0 * g.Wo;
    const int a = g.Wo - w0 < TM ? g.Wo - w0 : TM;               // rows on line L0
    const int nlines = g.Do * g.Ho;
    const int nseg = a < TM ? 1 + (TM - a + g.Wo - 1) / g.Wo : 1;
    const int nrows = TM + 2 * nseg;                             // staged halo rows

    // ---- staging map of this thread: halo row j = p*16 + tid/16, 16-byte piece tid%16 ----------------
    const int piece = tid & 15;
    int woff[NP];                                                 // w_in * in_stride + piece*4, < 0: never valid
    unsigned segbits = 0;                                        // 2 bits per p: the segment of row p
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int j = p * 16 + (tid >> 4);
        int sg = 0, w_in = w0 - 1 + j;
        if (j >= a + 2) {
            const int jj = j - (a + 2);
            sg = 1 + jj / (g.Wo + 2);
            w_in = jj - (sg - 1) * (g.Wo + 2) - 1;
        }
        const bool ok = j < nrows && w_in >= 0 && w_in < g.Wi;
        woff[p] = ok ? w_in * g.in_stride + piece * 4 : -1;
        segbits |= (unsigned)(sg & 3) << (2 * p);
    }

    const int ncc = (g.Cin + BK - 1) / BK;
    const int ngroups = g.KD * g.KH;
    const int nsteps = ngroups * ncc * 3;
    const int KpQ = ncc * (BK / 4);

    // (kd, kh) -> element offset of the source line of each of the two lines, or -1 (outside / not divisible)
    auto line_base = [&](int d, int h, int kd, int kh, bool exists) -> int {
        bool ok = exists;
        const int din = src_coord(d, kd, g.ls_d, g.pd, g.Di, MODE, ok);
        const int hin = src_coord(h, kh, g.ls_h, g.ph, g.Hi, MODE, ok);
        return ok ? ((din * g.Hi + hin) * g.Wi) * g.in_stride : -1;
    };
    // the lines of the tile, once (a line number -> (d, h) is a division)
    int seg_d[NSEG], seg_h[NSEG];
    bool seg_ok[NSEG];
#pragma unroll
    for (int k = 0; k < NSEG; ++k) {
        const int L = L0 + k;
        seg_d[k] = L / g.Ho; seg_h[k] = L - seg_d[k] * g.Ho;
        seg_ok[k] = k < nseg && L < nlines;
    }
    auto seg_base = [&](int k, int kd, int kh) -> int {          // source line of segment k, or -1
        return line_base(seg_d[k], seg_h[k], kd, kh, seg_ok[k]);
    };
    // A K step is (kd, kh, channel slab, kw); the walk keeps those four as counters (see igemm_tile)
    struct HStep { int s, kd, kh, cc, kw; };
    auto group_live = [&](const HStep& t) -> bool {
        bool any = false;
#pragma unroll
        for (int k = 0; k < NSEG; ++k) any = any || seg_base(k, t.kd, t.kh) >= 0;
        return any;
    };

    float4 ra[NP];
    float4 ry[FOLD ? NP : 1];
    float4 fmu = make_float4(0, 0, 0, 0), fis = fmu, fm1 = fmu, fm2 = fmu;     // FOLD (see igemm_tile)
    float4 rb0, rb1, rb2, rb3;
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    unsigned valid_mask = 0;
    bool staged_a = false;

    auto issue_loads = [&](const HStep& t) {
        const int kd = t.kd, kh = t.kh, cc = t.cc, kw = t.kw;
        staged_a = kw == 0;
        if (staged_a) {
            const int c = cc * BK + piece * 4;
            const bool cok = c < g.Cin;
            const int sb0 = seg_base(0, kd, kh), sb1 = seg_base(1, kd, kh), sb2 = NSEG > 2 ? seg_base(2, kd, kh) : -1;
            valid_mask = 0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const unsigned sg = (segbits >> (2 * p)) & 3u;
                const int lb = sg == 0 ? sb0 : (sg == 1 || NSEG == 2 ? sb1 : sb2);
                const bool ok = cok && woff[p] >= 0 && lb >= 0;
                const int off = ok ? lb + woff[p] + cc * BK : 0;        // branch-free: invalid pieces read element 0
                ra[p] = *reinterpret_cast<const float4*>(in + off);
                if (FOLD) ry[p] = *reinterpret_cast<const float4*>(g.in_y + off);
                valid_mask |= ok ? (1u << p) : 0u;
            }
            if (FOLD) {
                const int cs = cok ? c : 0;
                tsc = *reinterpret_cast<const float4*>(g.fold_bn + cs);
                tsh = *reinterpret_cast<const float4*>(g.fold_bn + g.Cin + cs);
                fmu = *reinterpret_cast<const float4*>(g.fold_bn + 2 * g.Cin + cs);
                fis = *reinterpret_cast<const float4*>(g.fold_bn + 3 * g.Cin + cs);
                fm1 = *reinterpret_cast<const float4*>(g.fold_coef + cs);
                fm2 = *reinterpret_cast<const float4*>(g.fold_coef + g.Cin + cs);
            }
            if (XF) {
                const int cs = cok ? c : 0;                     // unconditional, see k_igemm
                tsc = *reinterpret_cast<const float4*>(in_bn + cs);
                tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cs);
            }
        }
        const int tap = (kd * g.KH + kh) * 3 + kw;
        const float* wb = wp + ((size_t)(tap * KpQ + cc * (BK / 4)) * g.CoutP + n0) * 4;
        wslab_load<NW>(wb, g.CoutP, tid, rb0, rb1, rb2, rb3);
    };
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    auto store_lds = [&]() {
        if (staged_a) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float4 v = ra[p];
                const bool ok = (valid_mask >> p) & 1;
                if (FOLD) bn_fold(v, ry[p], tsc, tsh, fmu, fis, fm1, fm2, g.fold_relu, ok);
                else if (XF) affine_relu(v, tsc, tsh, relu_lo, ok);
                else masked(v, ok);
                const int j = p * 16 + (tid >> 4);
                if (j < HALO_MAX_ROWS) *reinterpret_cast<float4*>(sA + j * LDA + piece * 4) = v;
            }
        }
        wslab_store<NW>(sB, tid, rb0, rb1, rb2, rb3);
    };

    f32x16 acc0 = {0}, acc1 = {0};
    const int r_lane = (TM == 64 ? wave & 1 : wave) * 32 + (lane & 31);      // TM = 64: see igemm_tile
    const int seg_lane = r_lane < a ? 0 : 1 + (r_lane - a) / g.Wo;
    const int aoff = (r_lane + 2 * seg_lane) * LDA + 4 * (lane >> 5), boff = ((lane >> 5) * NW + (TM == 64 ? (wave >> 1) * 32 : 0) + (lane & 31)) * 4;
    const float* aLane = sA + aoff;
    const float* bCol = sB + boff;

    // split-K: slice z of the (kd, kh, channel slab) list -- whole A tiles, three taps each
    const int nstage = ngroups * ncc;
    const int s_end = nsplit > 1 ? 3 * (int)(((long long)(blockIdx.z + 1) * nstage) / nsplit) : nsteps;
    const int s_begin = nsplit > 1 ? 3 * (int)(((long long)blockIdx.z * nstage) / nsplit) : 0;
    auto next_group = [&](HStep& t) {
        if (++t.kh == g.KH) { t.kh = 0; ++t.kd; }
    };
    auto settle = [&](HStep t) -> HStep {           // the first live step at or after t (t.kw == 0), nsteps when none is left
        while (t.s < s_end && !group_live(t)) {      // a dead (kd, kh) pair goes with all its slabs and taps
            t.s += 3 * (ncc - t.cc); t.cc = 0;
            next_group(t);
        }
        if (t.s >= s_end) t.s = nsteps;
        return t;
    };
    auto next_of = [&](HStep t) -> HStep {
        ++t.s;
        if (++t.kw < 3) return t;                    // same A tile (slices end on whole tiles)
        t.kw = 0;
        if (++t.cc < ncc) {                          // same (kd, kh): live
            if (t.s >= s_end) t.s = nsteps;
            return t;
        }
        t.cc = 0;
        next_group(t);
        return settle(t);
    };
    HStep cur;
    {
        const int st = s_begin / 3, gi = st / ncc;                // the only divisions of a step number: once per tile
        cur.s = s_begin; cur.kw = 0; cur.cc = st - gi * ncc; cur.kd = gi / g.KH; cur.kh = gi - cur.kd * g.KH;
        cur = settle(cur);
    }
    IGEMM_STAMP(1);
    HStep nxt = cur;
    nxt.s = nsteps;
    bool next_staged = false;                       // DB: the registers hold step nxt, and its A tile is among them
    if (cur.s < nsteps) {
        issue_loads(cur);
        store_lds();
        if (DB) {
            nxt = next_of(cur);
            if (nxt.s < nsteps) { issue_loads(nxt); next_staged = staged_a; }
        }
    }
    __syncthreads();
    IGEMM_STAMP(2);
    int stamp_steps = 0, imgA = 0, imgW = 0;        // DB: the image holding the current A tile / the current W slab
    constexpr int IMG = HALO_MAX_ROWS * LDA + B_FLOATS;
    while (cur.s < nsteps) {
        ++stamp_steps;
        const int kw = cur.kw;
        if (DB) {
            // step nxt goes to the other image: its W slab always, its A tile when it opens a new (kd, kh, slab) group
            // (an A tile serves three steps; the image it leaves was last read a group ago); then the loads of the step after
            sA = smem + (imgA ^ 1) * IMG; sB = smem + (imgW ^ 1) * IMG + HALO_MAX_ROWS * LDA;
            aLane = smem + imgA * IMG + aoff; bCol = smem + imgW * IMG + HALO_MAX_ROWS * LDA + boff;
            HStep nn = nxt;
            if (nxt.s < nsteps) {
                store_lds();
                imgW ^= 1;
                if (next_staged) imgA ^= 1;
                nn = next_of(nxt);
                if (nn.s < nsteps) { issue_loads(nn); next_staged = staged_a; }
            }
            cur = nxt; nxt = nn;                    // (only kw, taken above, is read below)
        } else {
            nxt = next_of(cur);
            if (nxt.s < nsteps) issue_loads(nxt);
        }
        mfma_step64<TWO, NW>(aLane + (MODE == 0 ? kw : 2 - kw) * LDA, bCol, acc0, acc1);
        __syncthreads();
        if (!DB) {
            if (nxt.s < nsteps) store_lds();
            __syncthreads();
            cur = nxt;
        }
    }
    IGEMM_STAMP(3);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)stamp_steps;
    if (nsplit > 1) {
        const bool last = splitk_arrive<DB, TM == 64 ? 4 : 8>(acc0, acc1, partial, nsplit, (mb - tile0) * gridDim.y + blockIdx.y,
                                        gridDim.x * gridDim.y, wave, lane);
        IGEMM_STAMP(7);
        if (!last) { IGEMM_STAMP(4); return; }
    }
    if (TAIL) {
        // Dense(64) backward riding on the tile (model_training.py:195: the gradient this call stores is the one w.r.t. a
        // middle block's Dense output, gated by its ReLU): dz = (gated tile) @ Wd^T goes to tail_out with the backward
        // statistics of the BatchNormalization under the Dense -- 64 more MFMAs per wave on top of the tile's 27 x 64
        // instead of a launch that re-reads the 82 MB gradient (k_dense64<false, true>: 148 us alone at 320 000 rows)
        float* tA = smem;                             // [128][LDA]; the halo image is dead (the loop ended on a barrier)
        float* tB = smem + HALO_MAX_ROWS * LDA;
        store_tile(g, acc0, acc1, smem, m0 + wave * 32, n0, mb, mlimit, wave, lane, tid, bias, flags, out, nullptr, true, false,
                   1, tA);
        {
            // (behind the store, not under it: with the accumulators still live the 16 registers of the kernel's copy
            // took the workgroup from 152 to 168 registers, and a 168-register wave no longer fits beside the three
            // 120-register waves of a weight-gradient workgroup)
            const float* wl = g.tail_w + (size_t)(tid >> 6) * BN * 4 + (tid & 63) * 4;
            float* bl = tB + ((tid >> 6) * BN + (tid & 63)) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<float4*>(bl + i * 4 * BN * 4) = *reinterpret_cast<const float4*>(wl + i * 4 * BN * 4);
        }
        __syncthreads();
        f32x16 t0 = {0}, t1 = {0};
        const float* aRow = tA + (wave * 32 + (lane & 31)) * LDA + 4 * (lane >> 5);
        const float* bC = tB + ((lane >> 5) * BN + (lane & 31)) * 4;
#pragma unroll
        for (int kc = 0; kc < BK / 8; ++kc) {
            const float4 a = *reinterpret_cast<const float4*>(aRow + kc * 8);
            const float4 b0 = *reinterpret_cast<const float4*>(bC + kc * 2 * BN * 4);
            const float4 b1 = *reinterpret_cast<const float4*>(bC + kc * 2 * BN * 4 + 32 * 4);
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, t1, 0, 0, 0);
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, t1, 0, 0, 0);
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, t1, 0, 0, 0);
            t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, t1, 0, 0, 0);
        }
        store_tile(g, t0, t1, smem, m0 + wave * 32, n0, mb, mlimit, wave, lane, tid, nullptr, 0, g.tail_out, stats, true, false, 2);
        IGEMM_STAMP(4);
        return;
    }
    store_tile<TM>(g, acc0, acc1, smem, m0 + (TM == 64 ? wave & 1 : wave) * 32, n0, mb, mlimit, wave, lane, tid, bias, flags, out, stats,
                   true, NW == 32, 0, nullptr, TM == 64 ? partial : nullptr,
                   TM == 64 && partial ? partial + kSplitCounters + (nsplit > 1 ? (size_t)nsplit * gridDim.x * gridDim.y * (64 * 64) : 0) : nullptr);
    IGEMM_STAMP(4);
}

// TAG only changes the symbol name (see k_igemm).  With g.plane_pair the workgroup runs TWO tiles: the same (h, w) place of
// depth planes 2q and 2q + 1.  The planes of a strided or transposed Conv3D run different numbers of taps (the data
// gradient of the second middle block: 9 / 18 / 18 / 9 of 27 per plane); the hardware hands workgroups to the CUs in a
// fixed rotation and waits for a slot on the CU whose turn it is, so a launch of mixed 9- and 18-step workgroups left
// 40 % of the slots empty (tools/igemm_stamps.py).  Paired, every workgroup runs 27 steps.
template <int MODE, bool XF, int TAG = 0, int NSEG = 2, int NW = 64, bool DB = false, bool TAIL = false, bool FOLD = false>
__global__ void __launch_bounds__(kThreads)
k_igemm_halo(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp,
             const float* __restrict__ bias, const float* __restrict__ in_bn, int flags,
             float* __restrict__ out, double* __restrict__ stats, int nsplit, float* __restrict__ partial, int tile0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long* stamps = g_igemm_stamps;
    const unsigned stamp_wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    IGEMM_STAMP(0);
    const int v = tile0 + xcd_remap(blockIdx.x, gridDim.x);
    if (DB || !g.plane_pair) {
        halo_tile<MODE, XF, NSEG, NW, DB, TAIL, FOLD>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial, tile0, v, smem,
                                                      stamps, stamp_wg);
        return;
    }
    const int q = v / g.plane_tiles, i = v - q * g.plane_tiles;
    halo_tile<MODE, XF, NSEG, NW, false, TAIL>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial, tile0,
                                               2 * q * g.plane_tiles + i, smem, stamps, stamp_wg);
    __syncthreads();                                  // the epilogue's statistics scratch is the next tile's staging area
    halo_tile<MODE, XF, NSEG, NW, false, TAIL>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial, tile0,
                                               (2 * q + 1) * g.plane_tiles + i, smem, stamps, stamp_wg);
}

// ---------------------------------------------------------------------------------------------------------------
// Small tile: 64 positions x 64 channels per workgroup on the two-image (DB) loop, for the K-sliced layers of few tiles
// (RPN blocks 2 and 3, 5 000 x 128 and 1 250 x 256: forward layers and stride-1 data gradients).  As 128-row tiles those run one workgroup per
// CU, one wave per SIMD, and nothing covers a workgroup's prologue, staging, slab store or combine.  With 64 rows the map
// gives twice the tiles at the SAME K slicing: two workgroups per CU (69 760 B of LDS each at most), a second wave on
// every SIMD, slabs of half the size.  Every wave holds one 32 x 32 accumulator (32 MFMAs per step).  Each element's fmaf
// chain and the slice-order sum are those of the 128-row tile: the output is bit for bit the same.
// NSEG = 0: igemm_tile; 2: halo_tile (Wo >= 64: a 64-row tile touches at most two lines).  A kernel of its own so that the
// launch bounds of k_igemm / k_igemm_halo stay what they are.
template <int MODE, bool XF, int NSEG>
__global__ void __launch_bounds__(kThreads, 2)          // two workgroups per CU = two waves per SIMD: <= 256 registers
k_igemm_small(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp,
              const float* __restrict__ bias, const float* __restrict__ in_bn, int flags,
              float* __restrict__ out, double* __restrict__ stats, int nsplit, float* __restrict__ partial, int tile0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long* stamps = g_igemm_stamps;
    const unsigned stamp_wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    IGEMM_STAMP(0);
    const int v = tile0 + xcd_remap(blockIdx.x, gridDim.x);
    if constexpr (NSEG != 0)
        halo_tile<MODE, XF, NSEG, 64, true, false, false, 64>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial,
                                                                         tile0, v, smem, stamps, stamp_wg);
    else
        igemm_tile<MODE, XF, 64, true, false, 64>(g, in, wp, bias, in_bn, flags, out, stats, nsplit, partial, tile0, v, smem,
                                                  stamps, stamp_wg);
}

// ---------------------------------------------------------------------------------------------------------------
// Wide tile (round 4): 128 positions x 128 channels per 512-thread workgroup, w-halo staging (two lines per tile).
// The 128-channel stride-1 layers of the first RPN block (model_training.py:203-206: 20 000 positions, 157 tiles) ran as 628
// workgroups of 128 x 32 -- the A tile was staged for 32 MFMAs per wave and step and the layer sat at ~4 us of staging
// latency per step (80 us for 5.9 GFLOP, 0.47).  Here eight waves share one A tile: wave (rg, ch) owns rows 32 rg .. and
// columns 64 ch .. (two accumulators, the inner loop of halo_tile), the W slab is 64 x 128, and two workgroups per CU
// (68 KB of LDS each) put four waves on every SIMD, so one wave's staging hides behind the others' MFMAs.  K is sliced by
// whole A tiles as in halo_tile; the slices meet through splitk_arrive with eight waves.
constexpr int kWideThreads = 512;
constexpr int WB_FLOATS = BK * 128;
constexpr int kWideSlabF4 = 8 * 8 * 64;          // float4 per (slice, tile): 8 waves x 8 x 64 lanes = 128 x 128 floats
constexpr size_t wide_lds_bytes() { return (size_t)(halo_rows(2) * LDA + WB_FLOATS) * sizeof(float); }   // 68 672 B: 2 per CU

template <int MODE, bool XF>
__global__ void __launch_bounds__(kWideThreads, 4)      // two workgroups per CU = four waves per SIMD: <= 128 registers
k_igemm_wide(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
             const float* __restrict__ in_bn, int flags, float* __restrict__ out, double* __restrict__ stats, int nsplit,
             float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long* stamps = g_igemm_stamps;
    const unsigned stamp_wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    IGEMM_STAMP(0);
    constexpr int HALO_MAX_ROWS = halo_rows(2);
    float* sA = smem;
    float* sB = smem + HALO_MAX_ROWS * LDA;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave & 3, ch = wave >> 2;                     // 32-row group, 64-column half
    const int mb = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = mb * BM;
    const int n0 = blockIdx.y * 128;
    const int mlimit = g.M;

    const int L0 = m0 / g.Wo, w0 = m0 - L0 * g.Wo;
    const int a = g.Wo - w0 < BM ? g.Wo - w0 : BM;               // rows on line L0
    const int nlines = g.Do * g.Ho;
    const int nseg = a < BM ? 2 : 1;                             // Wo >= 126: at most two lines per tile
    const int nrows = BM + 2 * nseg;

    // staging map: halo row j = p * 32 + tid / 16, 16-byte piece tid % 16
    const int piece = tid & 15;
    int woff[5];
    unsigned segbits = 0;
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        const int j = p * 32 + (tid >> 4);
        int sg = 0, w_in = w0 - 1 + j;
        if (j >= a + 2) { sg = 1; w_in = j - (a + 2) - 1; }
        const bool ok = j < nrows && w_in >= 0 && w_in < g.Wi;
        woff[p] = ok ? w_in * g.in_stride + piece * 4 : -1;
        segbits |= (unsigned)sg << p;
    }
    const int ncc = (g.Cin + BK - 1) / BK;
    const int ngroups = g.KD * g.KH;
    const int nsteps = ngroups * ncc * 3;
    const int KpQ = ncc * (BK / 4);
    int seg_d[2], seg_h[2];
    bool seg_ok[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int L = L0 + k;
        seg_d[k] = L / g.Ho; seg_h[k] = L - seg_d[k] * g.Ho;
        seg_ok[k] = k < nseg && L < nlines;
    }
    auto seg_base = [&](int k, int kd, int kh) -> int {          // source line of segment k, or -1
        bool ok = seg_ok[k];
        const int din = src_coord(seg_d[k], kd, g.ls_d, g.pd, g.Di, MODE, ok);
        const int hin = src_coord(seg_h[k], kh, g.ls_h, g.ph, g.Hi, MODE, ok);
        return ok ? ((din * g.Hi + hin) * g.Wi) * g.in_stride : -1;
    };
    struct HStep { int s, kd, kh, cc, kw; };
    auto group_live = [&](const HStep& t) -> bool { return seg_base(0, t.kd, t.kh) >= 0 || seg_base(1, t.kd, t.kh) >= 0; };

    float4 ra[5];
    float4 rb[4];
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    unsigned valid_mask = 0;
    bool staged_a = false;
    auto issue_loads = [&](const HStep& t) {
        const int kd = t.kd, kh = t.kh, cc = t.cc, kw = t.kw;
        staged_a = kw == 0;
        if (staged_a) {
            const int c = cc * BK + piece * 4;
            const bool cok = c < g.Cin;
            const int sb0 = seg_base(0, kd, kh), sb1 = seg_base(1, kd, kh);
            valid_mask = 0;
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                const int lb = (segbits >> p) & 1 ? sb1 : sb0;
                const bool ok = cok && woff[p] >= 0 && lb >= 0;
                const int off = ok ? lb + woff[p] + cc * BK : 0;
                ra[p] = *reinterpret_cast<const float4*>(in + off);
                valid_mask |= ok ? (1u << p) : 0u;
            }
            if (XF) {
                const int cs = cok ? c : 0;
                tsc = *reinterpret_cast<const float4*>(in_bn + cs);
                tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cs);
            }
        }
        // W slab: 16 k-quads x 128 columns of float4, four per thread
        const int tap = (kd * g.KH + kh) * 3 + kw;
        const float* wb = wp + ((size_t)(tap * KpQ + cc * (BK / 4)) * g.CoutP + n0) * 4;
        const float* wl = wb + (size_t)(tid >> 7) * g.CoutP * 4 + (tid & 127) * 4;
        const size_t wstep = (size_t)4 * g.CoutP * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) rb[i] = *reinterpret_cast<const float4*>(wl + i * wstep);
    };
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    auto store_lds = [&]() {
        if (staged_a) {
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                float4 v = ra[p];
                const bool ok = (valid_mask >> p) & 1;
                if (XF) affine_relu(v, tsc, tsh, relu_lo, ok);
                else masked(v, ok);
                const int j = p * 32 + (tid >> 4);
                if (j < HALO_MAX_ROWS) *reinterpret_cast<float4*>(sA + j * LDA + piece * 4) = v;
            }
        }
        float* bl = sB + ((tid >> 7) * 128 + (tid & 127)) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(bl + i * 4 * 128 * 4) = rb[i];
    };

    f32x16 acc0 = {0}, acc1 = {0};
    const int r_lane = rg * 32 + (lane & 31);
    const int seg_lane = r_lane < a ? 0 : 1;
    const float* aLane = sA + (r_lane + 2 * seg_lane) * LDA + 4 * (lane >> 5);
    const float* bCol = sB + ((lane >> 5) * 128 + ch * 64 + (lane & 31)) * 4;

    const int nstage = ngroups * ncc;
    const int s_end = nsplit > 1 ? 3 * (int)(((long long)(blockIdx.z + 1) * nstage) / nsplit) : nsteps;
    const int s_begin = nsplit > 1 ? 3 * (int)(((long long)blockIdx.z * nstage) / nsplit) : 0;
    auto next_group = [&](HStep& t) { if (++t.kh == g.KH) { t.kh = 0; ++t.kd; } };
    auto settle = [&](HStep t) -> HStep {
        while (t.s < s_end && !group_live(t)) {
            t.s += 3 * (ncc - t.cc); t.cc = 0;
            next_group(t);
        }
        if (t.s >= s_end) t.s = nsteps;
        return t;
    };
    auto next_of = [&](HStep t) -> HStep {
        ++t.s;
        if (++t.kw < 3) return t;
        t.kw = 0;
        if (++t.cc < ncc) {
            if (t.s >= s_end) t.s = nsteps;
            return t;
        }
        t.cc = 0;
        next_group(t);
        return settle(t);
    };
    HStep cur;
    {
        const int st = s_begin / 3, gi = st / ncc;
        cur.s = s_begin; cur.kw = 0; cur.cc = st - gi * ncc; cur.kd = gi / g.KH; cur.kh = gi - cur.kd * g.KH;
        cur = settle(cur);
    }
    IGEMM_STAMP(1);
    if (cur.s < nsteps) { issue_loads(cur); store_lds(); }
    __syncthreads();
    IGEMM_STAMP(2);
    int stamp_steps = 0;
    while (cur.s < nsteps) {
        ++stamp_steps;
        const int kw = cur.kw;
        const HStep nxt = next_of(cur);
        if (nxt.s < nsteps) issue_loads(nxt);
        mfma_step64<true, 128>(aLane + (MODE == 0 ? kw : 2 - kw) * LDA, bCol, acc0, acc1);
        __syncthreads();
        if (nxt.s < nsteps) store_lds();
        __syncthreads();
        cur = nxt;
    }
    IGEMM_STAMP(3);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)stamp_steps;
    if (nsplit > 1) {
        const bool last = splitk_arrive<false, 8, 8>(acc0, acc1, partial, nsplit, mb * gridDim.y + blockIdx.y, gridDim.x * gridDim.y, wave, lane);
        IGEMM_STAMP(7);
        if (!last) { IGEMM_STAMP(4); return; }
    }
    // each column half is a 4-wave tile of its own for the store and the statistics; the halves use separate scratch and the
    // workgroup makes ONE sink arrival for both (g.sink.total counts workgroups)
    store_tile(g, acc0, acc1, smem + ch * 512, m0 + rg * 32, n0 + ch * 64, mb, mlimit, rg, lane, tid & 255, bias, flags, out, stats);
    IGEMM_STAMP(4);
}

// ---------------------------------------------------------------------------------------------------------------
// Dense(64) on the last axis (model_training.py:195) and its data gradient: 1x1x1, 64 -> 64, row m reads position m.
// One K step per tile, so k_igemm spends its time in phases (2500 workgroups load, then multiply, then store: 2.6 TB/s
// on a layer that moves 164 / 246 MB).  Here 768 workgroups stay resident and walk the tiles: the weights sit in LDS for
// the whole launch, the next tile's rows are requested before the current tile's MFMAs and stores, and the
// BatchNormalization-backward sums of the data gradient stay in registers until the workgroup is done (ONE sink arrival
// per workgroup instead of one per tile).
//   XF:  BatchNormalization of the producer applied on load (forward: Dense reads BN(conv)), bias + optional ReLU on store
//   BWD: (sum dz, sum dz * yhat) of the stored gradient for the BatchNormalization it is about to cross -> g.sink
//   DW:  (with BWD) the weight gradient of the same Dense beside its data gradient: the tile's rows of the gradient are in
//        LDS (the A operand) and its rows of y in registers (the statistics), which are the two operands of
//        dW[i][j] = sum_m bn(y)[m, i] * g[m, j] -- 64 more MFMAs per wave and tile under a kernel that waits for HBM, instead of
//        a second pass over both maps (k_wgrad: 35 / 46 / 67 us alone for the three middle blocks).  The accumulators stay in
//        registers for the whole launch; one 64 x 64 slab per workgroup, summed by k_dense_dw_reduce.
template <bool XF, bool BWD, bool DW = false>
__global__ void __launch_bounds__(kThreads, DW ? 2 : 3)     // three resident workgroups per CU (resident_slots): <= 168 registers;
k_dense64(ConvGeom g, const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
          const float* __restrict__ in_bn, int flags, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;
    float* sB = smem + A_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = (g.M + BM - 1) / BM;
    const int piece = tid & 15;
    // the whole 64 x 64 kernel: packed [k/4][n][4], copied once
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(sB + (i * 256 + tid) * 4) = *reinterpret_cast<const float4*>(wp + (i * 256 + tid) * 4);
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    if (XF) {
        tsc = *reinterpret_cast<const float4*>(in_bn + piece * 4);
        tsh = *reinterpret_cast<const float4*>(in_bn + 64 + piece * 4);
    }
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    const bool orelu = (flags & LISEC_CONV_OUT_RELU) != 0;
    const int col = lane & 31;
    const float biasA = bias ? bias[col] : 0.f, biasB = bias ? bias[32 + col] : 0.f;
    float ysA = 1.f, yhA = 0.f, ymA = 0.f, yiA = 0.f, ysB = 1.f, yhB = 0.f, ymB = 0.f, yiB = 0.f;
    if (BWD) {
        ysA = g.bwd_bn[col]; yhA = g.bwd_bn[64 + col]; ymA = g.bwd_bn[128 + col]; yiA = g.bwd_bn[192 + col];
        ysB = g.bwd_bn[32 + col]; yhB = g.bwd_bn[96 + col]; ymB = g.bwd_bn[160 + col]; yiB = g.bwd_bn[224 + col];
    }
    float sumA = 0.f, sqA = 0.f, sumB = 0.f, sqB = 0.f;
    f32x16 dw00 = {0}, dw01 = {0}, dw10 = {0}, dw11 = {0};      // DW: blocks (i half, j half) of this wave's share of dW

    // Every global access goes through a buffer descriptor over the layer's rows: one 32-bit lane offset per tile instead of a
    // 64-bit address, a clamp and a branch per row -- rows beyond the layer read zeros and their stores are dropped
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int nbytes = g.M * 256;
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, nbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(out, 0, nbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(BWD ? g.bwd_y : in), 0, nbytes, 0x00020000);
    const int a_voff = (tid >> 4) * 256 + piece * 16;                         // row tid >> 4 of a 16-row group, 16 bytes of it
    const int c_voff = (wave * 32 + 4 * (lane >> 5)) * 256 + col * 4;         // C layout: the wave's rows, this lane's column

    u32x4 ra[8];
    auto issue = [&](int tile) {
        const int vo = tile * (BM * 256) + a_voff;
#pragma unroll
        for (int p = 0; p < 8; ++p) ra[p] = __builtin_amdgcn_raw_buffer_load_b128(irs, vo + p * 4096, 0, 0);
    };
    auto stage = [&]() {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            float4 v = make_float4(__uint_as_float(ra[p].x), __uint_as_float(ra[p].y), __uint_as_float(ra[p].z), __uint_as_float(ra[p].w));
            if (XF) affine_relu(v, tsc, tsh, relu_lo, true);
            *reinterpret_cast<float4*>(sA + (p * 16 + (tid >> 4)) * LDA + piece * 4) = v;
        }
    };
    const float* aRow = sA + (wave * 32 + (lane & 31)) * LDA + 4 * (lane >> 5);
    const float* bCol = sB + ((lane >> 5) * BN + (lane & 31)) * 4;

    int tile = blockIdx.x;
    if (tile < ntiles) issue(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                                          // the previous tile's fragments have been read
        stage();
        __syncthreads();
        const int next = tile + gridDim.x;
        if (next < ntiles) issue(next);
        const int mw = tile * BM + wave * 32;
        const int cvo = tile * (BM * 256) + c_voff;               // accumulator row r is cvo + ((r & 3) + 8 * (r >> 2)) * 256
        // BWD: the tile's rows of y are requested HERE, before the MFMAs.  Read one by one inside the store loop they were
        // serialised behind the stores (the compiler cannot rule out that `out` aliases g.bwd_y): 16 dependent round trips
        // per tile, 15 us per tile and CU -- the kernel moved 246 MB in 148 us (1.7 TB/s)
        float yA[BWD ? 16 : 1], yB[BWD ? 16 : 1];
        if (BWD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = ((r & 3) + 8 * (r >> 2)) * 256;
                yA[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yrs, cvo + ro, 0, 0));
                yB[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yrs, cvo + ro + 128, 0, 0));
            }
        }
        f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
        for (int kc = 0; kc < BK / 8; ++kc) {
            const float4 a = *reinterpret_cast<const float4*>(aRow + kc * 8);
            const float4 b0 = *reinterpret_cast<const float4*>(bCol + kc * 2 * BN * 4);
            const float4 b1 = *reinterpret_cast<const float4*>(bCol + kc * 2 * BN * 4 + 32 * 4);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
        }
        if (DW) {
            // C-layout registers of y ARE an A operand: lanes 0-31 hold row m_r (k = 0), lanes 32-63 row m_r + 4 (k = 1), lane & 31
            // the channel i; the B operand is the same two rows of the gradient tile in LDS, lane & 31 the column j.  Rows beyond
            // the layer: the gradient rows are zeros (descriptor), so whatever bn(0) is, the product is zero
            const float* gRow = sA + (wave * 32 + 4 * (lane >> 5)) * LDA + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (r & 3) + 8 * (r >> 2);
                float xa = fmaf(yA[r], ysA, yhA), xb = fmaf(yB[r], ysB, yhB);
                if (g.bwd_relu) { xa = fmaxf(xa, 0.f); xb = fmaxf(xb, 0.f); }
                const float g0 = gRow[ml * LDA], g1 = gRow[ml * LDA + 32];
                dw00 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, g0, dw00, 0, 0, 0);
                dw01 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, g1, dw01, 0, 0, 0);
                dw10 = __builtin_amdgcn_mfma_f32_32x32x2f32(xb, g0, dw10, 0, 0, 0);
                dw11 = __builtin_amdgcn_mfma_f32_32x32x2f32(xb, g1, dw11, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ml = (r & 3) + 8 * (r >> 2);
            float va = acc0[r] + biasA, vb = acc1[r] + biasB;
            if (orelu) { va = fmaxf(va, 0.f); vb = fmaxf(vb, 0.f); }
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(va), ors, cvo + ml * 256, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vb), ors, cvo + ml * 256 + 128, 0, 0);
            if (BWD) {
                const bool ok = mw + ml + 4 * (lane >> 5) < g.M;
                const float ya = yA[r], yb = yB[r];
                const float da = (!ok || (g.bwd_relu && !(fmaf(ya, ysA, yhA) > 0.f))) ? 0.f : va;
                const float db = (!ok || (g.bwd_relu && !(fmaf(yb, ysB, yhB) > 0.f))) ? 0.f : vb;
                sumA += da; sqA = fmaf(da, (ya - ymA) * yiA, sqA);
                sumB += db; sqB = fmaf(db, (yb - ymB) * yiB, sqB);
            }
        }
    }
    if (DW) {
        // the four waves' shares, added in wave order (deterministic), then the workgroup's slab
        float* dsum = smem;                                       // [64][64]
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float* d0 = dsum + i * 64 + col;
                    float* d1 = dsum + (32 + i) * 64 + col;
                    if (w == 0) { d0[0] = dw00[r]; d0[32] = dw01[r]; d1[0] = dw10[r]; d1[32] = dw11[r]; }
                    else        { d0[0] += dw00[r]; d0[32] += dw01[r]; d1[0] += dw10[r]; d1[32] += dw11[r]; }
                }
            }
        }
        __syncthreads();
        float* slab = g.dw_slabs + (size_t)blockIdx.x * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(slab + (i * 256 + tid) * 4) = *reinterpret_cast<const float4*>(dsum + (i * 256 + tid) * 4);
    }
    if (BWD) {
        __syncthreads();
        float* red = smem;                                        // [4 waves][4][32]
        sumA += __shfl_xor(sumA, 32, 64); sqA += __shfl_xor(sqA, 32, 64);
        sumB += __shfl_xor(sumB, 32, 64); sqB += __shfl_xor(sqB, 32, 64);
        if (lane < 32) {
            red[(wave * 4 + 0) * 32 + lane] = sumA; red[(wave * 4 + 1) * 32 + lane] = sqA;
            red[(wave * 4 + 2) * 32 + lane] = sumB; red[(wave * 4 + 3) * 32 + lane] = sqB;
        }
        __syncthreads();
        if (tid < 128) {
            const int q = tid >> 5, c = tid & 31;                // q: 0 sumA, 1 sqA, 2 sumB, 3 sqB
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += (double)red[(k * 4 + q) * 32 + c];
            sink_add(g.sink, q & 1, (q >> 1) * 32 + c, v);
        }
        sink_finish(g.sink);
    }
}

// dW[e] = sum over the workgroups' slabs.  256 workgroups of 16 elements; thread (group = tid >> 4, e = tid & 15) adds slabs
// group * n/16 ... in index order with eight loads in flight, the 16 group sums are then added in group order: a fixed tree,
// so the result does not depend on timing (one thread per element walking all 512 slabs took 70-96 us: 128 dependent round trips)
__global__ void __launch_bounds__(256) k_dense_dw_reduce(const float* __restrict__ slabs, int n, float* __restrict__ dW) {
    __shared__ float part[16][16];
    const int e = blockIdx.x * 16 + (threadIdx.x & 15), grp = threadIdx.x >> 4;
    const int per = (n + 15) / 16, z0 = grp * per, z1 = z0 + per < n ? z0 + per : n;
    float s = 0.f;
    int z = z0;
    for (; z + 8 <= z1; z += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = slabs[(size_t)(z + k) * 4096 + e];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; z < z1; ++z) s += slabs[(size_t)z * 4096 + e];
    part[grp][threadIdx.x & 15] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += part[k][threadIdx.x];
        dW[e] = t;
    }
}

// all layers of the network in ONE launch: table of descriptors in device memory, element index -> layer by
// a search over the running element offsets
__global__ void k_pack_weights_batched(const lisec_pack_desc* __restrict__ tab, int n, long long total) {
    // one float4 of the packed layout (four consecutive k of one column) per thread: 16-byte coalesced stores, and
    // for (K, N)-major sources (k_stride == N) four coalesced row reads per wave
    for (long long i4 = blockIdx.x * 256LL + threadIdx.x; i4 < (total >> 2); i4 += (long long)gridDim.x * 256) {
        const long long i = i4 << 2;
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid].start <= i) lo = mid; else hi = mid - 1;
        }
        const lisec_pack_desc d = tab[lo];
        long long t = (i - d.start) >> 2;
        const int nn = (int)(t % d.Np);
        t /= d.Np;
        const int kq = (int)(t % (d.Kp / 4));
        const int tap = (int)(t / (d.Kp / 4));
        const float* s0 = d.src + tap * d.tap_stride + (long long)(kq * 4) * d.k_stride + nn * d.n_stride;
        const bool nok = nn < d.N;
        float4 v;
        v.x = (nok && kq * 4 + 0 < d.K) ? s0[0] : 0.f;
        v.y = (nok && kq * 4 + 1 < d.K) ? s0[d.k_stride] : 0.f;
        v.z = (nok && kq * 4 + 2 < d.K) ? s0[2 * d.k_stride] : 0.f;
        v.w = (nok && kq * 4 + 3 < d.K) ? s0[3 * d.k_stride] : 0.f;
        *reinterpret_cast<float4*>(d.dst + (i - d.start)) = v;
    }
}

// dst[tap][k/4][n][k%4] (K padded to 64, N padded to 64, zero filled) from an arbitrary strided source
__global__ void k_pack_weights(const float* __restrict__ src, int ntaps, int K, int N, long long tap_stride,
                               long long k_stride, long long n_stride, int Kp, int Np, float* __restrict__ dst) {
    const long long total = (long long)ntaps * Kp * Np;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int j = (int)(i & 3);
        long long t = i >> 2;
        int n = (int)(t % Np);
        t /= Np;
        int kq = (int)(t % (Kp / 4));
        int tap = (int)(t / (Kp / 4));
        int k = kq * 4 + j;
        dst[i] = (k < K && n < N) ? src[tap * tap_stride + k * k_stride + n * n_stride] : 0.f;
    }
}

}  // namespace

int conv_geom_check(const lisec_conv_geom* c, ConvGeom* g) {
    LISEC_CHECK_ARG(c, "geom is NULL");
    LISEC_CHECK_ARG(c->mode == 0 || c->mode == 1, "mode must be 0 or 1");
    auto lg = [](int s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : -1; };
    int ld = lg(c->sd), lh = lg(c->sh), lw = lg(c->sw);
    LISEC_CHECK_ARG(ld >= 0 && lh >= 0 && lw >= 0, "strides must be 1, 2 or 4");
    LISEC_CHECK_ARG(c->Di > 0 && c->Hi > 0 && c->Wi > 0 && c->Do > 0 && c->Ho > 0 && c->Wo > 0, "bad dims");
    LISEC_CHECK_ARG(c->Do < 1024 && c->Ho < 1024 && c->Wo < 1024, "output dims must be < 1024");
    LISEC_CHECK_ARG(c->KD >= 1 && c->KH >= 1 && c->KW >= 1 && c->KD <= 4 && c->KH <= 4 && c->KW <= 4,
                    "kernel taps must be in [1,4] per axis");
    LISEC_CHECK_ARG((long long)c->Di * c->Hi * c->Wi * c->in_stride < (1LL << 31), "gathered tensor too large (int32 offsets)");
    LISEC_CHECK_ARG(c->Cin >= 4 && c->Cin % 4 == 0 && c->in_stride >= c->Cin && c->in_stride % 4 == 0,
                    "Cin/in_stride must be multiples of 4");
    if (c->ps) {
        LISEC_CHECK_ARG(c->ps >= 1 && c->ps <= 8 && c->ps_channels > 0 && c->ps_channels % 64 == 0 &&
                        c->Cout == c->ps * c->ps * c->ps_channels && c->out_stride >= c->ps_channels &&
                        c->Do == 1 && c->KD * c->KH * c->KW == 1,
                        "pixel-shuffle store needs a 2D 1x1 geometry with Cout = ps*ps*ps_channels, ps_channels % 64 == 0");
    } else {
        LISEC_CHECK_ARG(c->out_stride >= c->Cout, "bad out_stride");
    }
    LISEC_CHECK_ARG(c->Cout >= 1, "bad Cout");
    LISEC_CHECK_ARG((long long)c->Do * c->Ho * c->Wo < (1LL << 30), "too many output positions");
    g->Di = c->Di; g->Hi = c->Hi; g->Wi = c->Wi; g->Do = c->Do; g->Ho = c->Ho; g->Wo = c->Wo;
    g->KD = c->KD; g->KH = c->KH; g->KW = c->KW; g->ls_d = ld; g->ls_h = lh; g->ls_w = lw;
    g->pd = c->pd; g->ph = c->ph; g->pw = c->pw;
    g->Cin = c->Cin; g->in_stride = c->in_stride; g->Cout = c->Cout; g->out_stride = c->out_stride;
    g->CoutP = (int)align_up(c->Cout, 64);
    g->M = c->Do * c->Ho * c->Wo;
    g->ps = c->ps; g->ps_channels = c->ps_channels;
    g->row_coords = nullptr; g->row_count = nullptr; g->out_mask = nullptr;
    g->pc_span = 0; g->pc_rows = 0;
    g->bwd_y = nullptr; g->bwd_bn = nullptr; g->bwd_relu = 0;
    g->sink.acc = nullptr;
    g->plane_tiles = 0; g->plane_pair = 0; g->queue = nullptr;
    g->tail_w = nullptr; g->tail_out = nullptr;
    g->in_y = nullptr; g->fold_bn = nullptr; g->fold_coef = nullptr; g->fold_relu = 0;
    g->dw_slabs = nullptr;
    g->pointwise = c->KD * c->KH * c->KW == 1 && ld == 0 && lh == 0 && lw == 0 && c->pd == 0 && c->ph == 0 && c->pw == 0 &&
                   c->Di == c->Do && c->Hi == c->Ho && c->Wi == c->Wo;
    return 0;
}

}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_conv_packed_floats(int ntaps, int K, int N) {
    if (ntaps <= 0 || K <= 0 || N <= 0) return 0;
    return (size_t)ntaps * align_up(K, 64) * align_up(N, 64);
}

extern "C" int lisec_conv_pack_weights(const float* src, int ntaps, int K, int N, long long tap_stride,
                                       long long k_stride, long long n_stride, float* dst,
                                       lisec_stream_t stream_) {
    LISEC_CHECK_ARG(src && dst && ntaps > 0 && K > 0 && N > 0, "bad pack arguments");
    int Kp = (int)align_up(K, 64), Np = (int)align_up(N, 64);
    long long total = (long long)ntaps * Kp * Np;
    int gb = cdiv(total, 256);
    if (gb > 8192) gb = 8192;
    LISEC_LAUNCH(k_pack_weights, dim3(gb), dim3(256), 0, static_cast<hipStream_t>(stream_), src, ntaps,
                       K, N, tap_stride, k_stride, n_stride, Kp, Np, dst);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_conv_pack_weights_batched(const lisec_pack_desc* device_table, int n, long long total,
                                               lisec_stream_t stream_) {
    LISEC_CHECK_ARG(device_table && n > 0 && total > 0, "bad batched pack arguments");
    LISEC_CHECK_ARG(total % 4 == 0, "packed sizes are multiples of 4");
    int gb = cdiv(total / 4, 256);
    if (gb > 8192) gb = 8192;
    LISEC_LAUNCH(k_pack_weights_batched, dim3(gb), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       device_table, n, total);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_conv_num_mblocks(const lisec_conv_geom* c) {
    ConvGeom g;
    if (conv_geom_check(c, &g)) return -1;
    return cdiv(g.M, BM);
}

namespace { void parity_order(const lisec_conv_geom* c, ConvGeom* g); }

extern "C" int lisec_conv_num_mblocks_bwd(const lisec_conv_geom* c) {
    ConvGeom g;
    if (conv_geom_check(c, &g)) return -1;
    parity_order(c, &g);                              // the row order a backward-statistics call uses
    return cdiv(g.M, BM);
}

namespace {
int resident_slots() {
    return 3 * cu_count();       // 51 KB LDS per workgroup -> 3 per CU
}

// k_dense64 with the Dense weight gradient beside the data gradient holds 64 more accumulators: two workgroups per CU
int dense_dw_slots() { return 2 * (resident_slots() / 3); }

// Switches `g` to the parity-class row order (conv.h) when the geometry is a 2D transposed gather with stride 2 along
// h and w over an even map.
void parity_order(const lisec_conv_geom* c, ConvGeom* g) {
    if (c->mode == 1 && g->ls_h == 1 && g->ls_w == 1 && g->Do == 1 && g->KD == 1 && !c->ps && g->Ho % 2 == 0 &&
        g->Wo % 2 == 0 && g->Wo >= 64) {
        g->pc_rows = (g->Ho / 2) * (g->Wo / 2);
        g->pc_span = cdiv(g->pc_rows, BM) * BM;
        g->M = 4 * g->pc_span;
    }
}

// (scale = 1, shift = 0) for any channel count up to kIdentityMax, part of the code object (no allocation, never written):
// the on-load affine of a call that only asked for LISEC_CONV_IN_RELU.  The kernels read scale at in_bn[c] and shift at
// in_bn[Cin + c]: the table is kIdentityMax ones followed by kIdentityMax zeros, entered Cin floats before the zeros.
constexpr int kIdentityMax = 4096;
__device__ const float4 g_identity_bn[2 * kIdentityMax / 4] = {
#define LISEC_ONE4 {1.f, 1.f, 1.f, 1.f}
#define LISEC_ONE64 LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, \
                    LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4, LISEC_ONE4
#define LISEC_ONE1024 LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, \
                      LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64, LISEC_ONE64
    LISEC_ONE1024, LISEC_ONE1024, LISEC_ONE1024, LISEC_ONE1024          // the zeros follow (rest of the initialiser)
#undef LISEC_ONE1024
#undef LISEC_ONE64
#undef LISEC_ONE4
};
const float* identity_bnstate(int C) {
    if (C > kIdentityMax || C % 4) return nullptr;
    void* base = nullptr;
    if (hipGetSymbolAddress(&base, HIP_SYMBOL(g_identity_bn)) != hipSuccess) return nullptr;
    return static_cast<const float*>(base) + (kIdentityMax - C);
}

// Everything lisec_conv_forward_ex decides before it launches, in one place -- so that lisec_conv_plan_query reports the
// plan a call WILL run, not a restatement of it.
//
// K slicing: layers with few tiles are cut into K slices so that they fill the 256 CUs; layers with many tiles run whole
// rounds unsplit and only the LAST, partially filled round is K-sliced (otherwise e.g. mid1's 2500 tiles take 4 rounds of
// 768 resident workgroups for 3.25 rounds of work).  The slices of a tile are combined inside the kernel by the last one
// to arrive (splitk_arrive): the workspace holds kSplitCounters arrival counters (zero between calls) and the slabs.
//
// plan_conv ends by writing the launches the call consists of (at most two: the whole rounds and the K-sliced tail) into
// ConvCall::launch.  lisec_conv_forward_ex issues that list and lisec_conv_plan_query adds it up; neither decides anything.
using TileKernel = decltype(&k_igemm<0, false>);            // k_igemm / k_igemm_halo
using ResidentKernel = decltype(&k_igemm_queue<0, false>);  // k_igemm_queue / k_dense64
using WideKernel = decltype(&k_igemm_wide<0, false>);

struct ConvLaunch {
    enum Kind { TILE, RESIDENT, WIDE } kind;     // the signature, i.e. which pointer is live
    union { TileKernel tile; ResidentKernel resident; WideKernel wide; };
    dim3 grid, block;
    size_t lds;
    int nsplit, tile0;
    bool partial;                // the workspace is passed as `partial` (nullptr otherwise)
};

struct ConvCall {
    ConvGeom g;
    int ntiles, nnb;
    int tile0_tail, nsplit;      // first tile of the K-sliced tail (== ntiles: none); slices
    size_t ws_bytes;
    bool xf;
    bool db;                     // the K-sliced launch runs the two-image (double-buffered) kernels, one workgroup per CU
    int tm;                      // rows per tile: BM, or 64 (k_igemm_small; ntiles then counts 64-row tiles)
    int kernel, cols;            // LISEC_KERNEL_*; output channels per workgroup
    double* stats;               // per-tile table (or the dummy that keeps the statistics paths on under a sink)
    ConvLaunch launch[2];
    int nlaunch;

    ConvLaunch& add(ConvLaunch::Kind kind, dim3 grid, int threads, size_t lds) {
        ConvLaunch& l = launch[nlaunch++];
        l.kind = kind; l.grid = grid; l.block = dim3(threads); l.lds = lds;
        l.nsplit = 1; l.tile0 = 0; l.partial = false;
        return l;
    }
};

// ---- the instantiations of the family.  These helpers name every kernel the library compiles and no other: a variant
// that is not listed here does not exist, and plan_conv never asks for one.
// Calls f(M, X) with the gather mode and the transform-on-load switch as integral constants.
template <typename F>
auto with_mode_xf(int mode, bool xf, F f) {
    using M0 = std::integral_constant<int, 0>;
    using M1 = std::integral_constant<int, 1>;
    if (mode == 0) return xf ? f(M0{}, std::true_type{}) : f(M0{}, std::false_type{});
    return xf ? f(M1{}, std::true_type{}) : f(M1{}, std::false_type{});
}

struct TileVariant {
    int mode;
    bool xf;
    int nseg;                    // 0: k_igemm; 2 / 3: k_igemm_halo with that many lines per tile
    int cols = 64;               // 32: half-N workgroups (never sliced, so never double-buffered)
    bool db = false;             // two LDS images
    bool tail = false;           // second contraction on the stored tile (two-line halo, 64 columns)
    bool fold = false;           // BatchNormalization backward on load (mode 1, no XF)
    bool roofline = false;       // the TAG = 1 symbols (no XF; halo with two lines only)
    int tm = BM;                 // 64: k_igemm_small (two images, 64 columns, nseg 0 or 2, none of the switches above)
};

template <int M, bool X>
TileKernel plain_kernel(int cols, bool db) {
    if (db) return k_igemm<M, X, 0, 64, true>;
    if (cols == 32) return k_igemm<M, X, 0, 32>;
    return k_igemm<M, X>;
}
template <int M, bool X, int NSEG>
TileKernel halo_kernel(int cols, bool db) {
    if (db) return k_igemm_halo<M, X, 0, NSEG, 64, true>;
    if (cols == 32) return k_igemm_halo<M, X, 0, NSEG, 32>;
    return k_igemm_halo<M, X, 0, NSEG>;
}
template <int NSEG>
TileKernel fold_halo_kernel(int cols, bool db) {
    if (db) return k_igemm_halo<1, false, 0, NSEG, 64, true, false, true>;
    if (cols == 32) return k_igemm_halo<1, false, 0, NSEG, 32, false, false, true>;
    return k_igemm_halo<1, false, 0, NSEG, 64, false, false, true>;
}
TileKernel fold_kernel(int nseg, int cols, bool db) {
    switch (nseg) {
    case 2: return fold_halo_kernel<2>(cols, db);
    case 3: return fold_halo_kernel<3>(cols, db);
    }
    if (db) return k_igemm<1, false, 0, 64, true, true>;
    if (cols == 32) return k_igemm<1, false, 0, 32, false, true>;
    return k_igemm<1, false, 0, 64, false, true>;
}
TileKernel roofline_kernel(int mode, int nseg) {
    if (nseg) return mode == 0 ? k_igemm_halo<0, false, 1, 2> : k_igemm_halo<1, false, 1, 2>;
    return mode == 0 ? k_igemm<0, false, 1> : k_igemm<1, false, 1>;
}
TileKernel small_kernel(int mode, bool xf, int nseg) {
    return with_mode_xf(mode, xf, [&](auto m, auto x) -> TileKernel {
        constexpr int M = decltype(m)::value;
        constexpr bool X = decltype(x)::value;
        return nseg ? k_igemm_small<M, X, 2> : k_igemm_small<M, X, 0>;
    });
}
TileKernel tile_kernel(const TileVariant& v) {
    if (v.tm == 64) return small_kernel(v.mode, v.xf, v.nseg);
    if (v.roofline) return roofline_kernel(v.mode, v.nseg);
    if (v.fold) return fold_kernel(v.nseg, v.cols, v.db);
    return with_mode_xf(v.mode, v.xf, [&](auto m, auto x) -> TileKernel {
        constexpr int M = decltype(m)::value;
        constexpr bool X = decltype(x)::value;
        if (v.tail) return k_igemm_halo<M, X, 0, 2, 64, false, true>;
        switch (v.nseg) {
        case 2: return halo_kernel<M, X, 2>(v.cols, v.db);
        case 3: return halo_kernel<M, X, 3>(v.cols, v.db);
        }
        return plain_kernel<M, X>(v.cols, v.db);
    });
}
ResidentKernel queue_kernel(int mode, bool xf) {
    return with_mode_xf(mode, xf, [](auto m, auto x) -> ResidentKernel { return k_igemm_queue<decltype(m)::value, decltype(x)::value>; });
}
WideKernel wide_kernel(int mode, bool xf) {
    return with_mode_xf(mode, xf, [](auto m, auto x) -> WideKernel { return k_igemm_wide<decltype(m)::value, decltype(x)::value>; });
}
ResidentKernel dense64_kernel(bool xf, bool bwd, bool dw) {
    if (dw) return k_dense64<false, true, true>;
    if (bwd) return xf ? k_dense64<true, true> : k_dense64<false, true>;
    return xf ? k_dense64<true, false> : k_dense64<false, false>;
}
constexpr size_t tile_lds_bytes(int nseg, int tm = BM) {
    return nseg ? halo_lds_bytes(nseg, tm) : (size_t)(tm * LDA + B_FLOATS) * sizeof(float);
}

void plan_slices(const ConvGeom& g, ConvCall* p) {
    const lisec_tuning& tn = tuning();
    const int ntiles = cdiv(g.M, BM), nnb = g.CoutP / BN;
    p->tile0_tail = ntiles; p->nsplit = 1; p->ws_bytes = 0; p->db = false; p->tm = BM;
    const int nsteps = g.KD * g.KH * g.KW * cdiv(g.Cin, BK);
    if (g.ps || g.Cout % 4 != 0 || g.out_stride % 4 != 0 || nsteps < 6) return;
    const int slots = resident_slots();
    const long long blocks = (long long)ntiles * nnb;
    int tail_tiles;
    if (blocks < slots / 4) {                       // small layer: slice all of it
        tail_tiles = ntiles;
    } else {
        const int tiles_per_round = slots / nnb > 0 ? slots / nnb : 1;
        tail_tiles = ntiles % tiles_per_round;
        if (ntiles < tiles_per_round) tail_tiles = ntiles;
    }
    const long long tail_blocks = (long long)tail_tiles * nnb;
    if (tail_blocks == 0 || tail_blocks * 10 > (long long)slots * 7) return;   // tail round >= 70 % full already
    if (blocks > 2LL * slots) return;       // >= 3 rounds: the short last round costs less than a sliced launch
    if (tail_blocks > kSplitCounters) return;
    int ns = (int)(slots / tail_blocks);
    if (ns > nsteps / tn.splitk_min_steps) ns = nsteps / tn.splitk_min_steps;
    if (ns > tn.max_splitk) ns = tn.max_splitk;
    if (tn.force_splitk > 0) ns = tn.force_splitk < nsteps ? tn.force_splitk : nsteps;     // measurement aid
    if (tn.lone_db && tail_tiles == ntiles && blocks < slots / 4 && !g.row_coords) {
        // a small layer, sliced as a whole: ONE workgroup per CU on the two-image kernels instead of two or three per CU on
        // the single-image ones -- half the slices (and slabs) for the same number of MFMA steps per CU
        int nd = (int)((slots / 3) / tail_blocks);
        if (nd > nsteps / tn.splitk_min_steps) nd = nsteps / tn.splitk_min_steps;
        if (nd > tn.max_splitk) nd = tn.max_splitk;
        if (tn.force_splitk > 0) nd = ns;           // measurement aid: holds for the lone form too
        if (nd >= 2) { ns = nd; p->db = true; }
        // 64-row tiles (k_igemm_small) for such a layer: the SAME slices -- so every element keeps its sum order -- over
        // twice the tiles, two workgroups per CU.  A candidate here; plan_conv keeps it for the calls the kernel serves
        if (tn.small_tile && g.Cout % BN == 0 && !g.pc_span) p->tm = 64;
    }
    // a 64-row candidate: room for whichever tile height plan_conv settles on, and 256 floats per 64-row workgroup where the
    // two halves of a 128-row tile meet for the statistics sink (store_tile)
    const size_t pair_floats = p->tm == 64 ? (size_t)cdiv(g.M, 64) * nnb * 256 : 0;
    if (ns < 2 || ns < tn.min_splitk) {
        p->db = false;
        if (p->tm == 64) p->ws_bytes = align_up(sizeof(int) * kSplitCounters + sizeof(float) * pair_floats, 256);
        return;
    }
    p->tile0_tail = ntiles - tail_tiles;
    p->nsplit = ns;
    const size_t rows = p->tm == 64 && cdiv(g.M, 64) * 64 > tail_tiles * BM ? (size_t)cdiv(g.M, 64) * 64 : (size_t)tail_tiles * BM;
    p->ws_bytes = align_up(sizeof(int) * kSplitCounters + sizeof(float) * ((size_t)ns * rows * nnb * BN + pair_floats), 256);
}

// The 128 x 128 tile (k_igemm_wide): layers of 128 (256, ...) output channels on the two-line w-halo geometry whose 128-row
// tiles leave the chip under-filled (the stride-1 layers of the first RPN block and their data gradients: 157 tiles).  Two
// workgroups per CU; K sliced by whole A tiles so that the launch is one round of them.
bool plan_wide(const ConvGeom& g, int* nsplit, size_t* ws_bytes) {
    if (!tuning().wide_tile || g.row_coords || g.ps || g.pc_span || g.queue || g.tail_w) return false;
    if (!(g.ls_w == 0 && g.KW == 3 && g.pw == 1 && g.Wi == g.Wo && g.Wo >= BM - 2 && g.in_stride % 4 == 0)) return false;
    if (g.CoutP % 128 != 0 || g.Cout % 4 != 0 || g.out_stride % 4 != 0) return false;
    const long long blocks = (long long)cdiv(g.M, BM) * (g.CoutP / 128);
    const int slots = 2 * (resident_slots() / 3);                       // two workgroups per CU
    if (blocks > 2LL * slots || blocks > kSplitCounters) return false;  // big layers fill the chip with 128 x 64 tiles
    const int nstage = g.KD * g.KH * cdiv(g.Cin, BK);
    int ns = (int)(slots / blocks);
    if (ns > nstage) ns = nstage;
    if (ns > tuning().max_splitk) ns = tuning().max_splitk;
    if (ns < 1) ns = 1;
    *nsplit = ns;
    *ws_bytes = ns > 1 ? align_up(sizeof(int) * kSplitCounters + (size_t)ns * blocks * kWideSlabF4 * 16, 256) : 0;
    return true;
}

int plan_conv(const lisec_conv_geom* c, bool has_in_bn, int flags, const lisec_conv_extras* extras, double* stats_partials,
              const void* workspace, size_t workspace_bytes, const int32_t* row_coords, const int32_t* row_count,
              int row_capacity, ConvCall* p) {
    ConvGeom& g = p->g;
    if (int rc = conv_geom_check(c, &g)) return rc;
    p->nlaunch = 0; p->cols = 64;
    const lisec_tuning& tn = tuning();
    const float* out_mask = extras ? extras->out_mask : nullptr;
    LISEC_CHECK_ARG(!out_mask || (!c->ps && ((uintptr_t)out_mask & 15) == 0),
                    "out_mask: 16-byte aligned, not with a pixel-shuffle store");
    g.out_mask = out_mask;
    const bool bwd_stats = extras && extras->bwd_y;
    const lisec_bn_sink* sk = extras ? extras->sink : nullptr;
    const bool table_stats = stats_partials != nullptr && !sk;     // per-tile partial table (laid out for 128-row tiles)
    if (sk) {
        LISEC_CHECK_ARG(sk->acc && sk->n_rows > 0 && !row_coords && !c->ps, "bn sink: accumulators, row count, dense rows");
        LISEC_CHECK_ARG((sk->kind == LISEC_SINK_FORWARD && !bwd_stats && sk->gamma && sk->beta && sk->bnstate &&
                         (sk->moving_mean == nullptr) == (sk->moving_var == nullptr)) ||
                        (sk->kind == LISEC_SINK_BACKWARD && bwd_stats && sk->dgamma && sk->dbeta && sk->coef),
                        "bn sink: kind 1 needs gamma/beta/bnstate and no bwd_y, kind 2 needs bwd_y and dgamma/dbeta/coef");
        // a dummy non-NULL partial table keeps the statistics code paths on; the sink takes precedence in the kernels
        if (!stats_partials) stats_partials = reinterpret_cast<double*>(sk->acc);
    }
    if (bwd_stats) {
        LISEC_CHECK_ARG(extras->bwd_bnstate && stats_partials && !c->ps && !row_coords && c->Cout % 4 == 0 &&
                        ((uintptr_t)extras->bwd_y & 15) == 0 && ((uintptr_t)extras->bwd_bnstate & 15) == 0,
                        "backward statistics need y, its bnstate, a partials buffer, dense rows and Cout % 4 == 0");
        g.bwd_y = extras->bwd_y; g.bwd_bn = extras->bwd_bnstate; g.bwd_relu = extras->bwd_relu ? 1 : 0;
    }
    if (extras && extras->dense_dw) {
        LISEC_CHECK_ARG(bwd_stats && sk && !has_in_bn && !out_mask && !extras->in_y && !extras->tail_w && !table_stats &&
                        !(flags & (LISEC_CONV_ACCUMULATE | LISEC_CONV_TAG_ROOFLINE | LISEC_CONV_IN_RELU)) && g.pointwise &&
                        g.Cin == 64 && g.Cout == 64 && g.in_stride == 64 && g.out_stride == 64 && tn.dense64 &&
                        cdiv(g.M, BM) >= dense_dw_slots() && g.M < (1 << 23) && ((uintptr_t)extras->dense_dw & 15) == 0,
                        "dense_dw: the data gradient of a Dense(64) (1x1x1, 64 -> 64, packed rows) with bwd_y and a backward sink, "
                        "at least lisec_dense_dw_slabs() tiles of 128 rows, 16-byte aligned slabs");
        g.dw_slabs = extras->dense_dw;
    }
    if (extras && extras->in_y) {
        LISEC_CHECK_ARG(extras->in_fold_bnstate && extras->in_fold_coef && c->mode == 1 && !has_in_bn && !(flags & LISEC_CONV_IN_RELU) &&
                        !row_coords && c->Cin % 4 == 0 && ((uintptr_t)extras->in_y & 15) == 0 &&
                        ((uintptr_t)extras->in_fold_bnstate & 15) == 0 && ((uintptr_t)extras->in_fold_coef & 15) == 0,
                        "in_y (BatchNormalization backward on load): a transposed gather (mode 1) without in_bnstate / IN_RELU, "
                        "with the layer's bnstate and the backward sink's coefficients, 16-byte aligned");
        g.in_y = extras->in_y; g.fold_bn = extras->in_fold_bnstate; g.fold_coef = extras->in_fold_coef;
        g.fold_relu = extras->in_fold_relu ? 1 : 0;
    }
    p->stats = stats_partials;
    // stride 2 along h and w, transposed gather (data gradient of a stride-2 Conv2D): rows are visited in parity
    // classes so that a tile only runs the taps that divide -- 9/4 of the 9 taps on average
    if (!row_coords && (!stats_partials || bwd_stats)) parity_order(c, &g);
    if (row_coords) {
        LISEC_CHECK_ARG(row_count && row_capacity > 0 && !stats_partials && !c->ps,
                        "row list needs a device count, a capacity, and no stats / pixel-shuffle");
        g.row_coords = row_coords; g.row_count = row_count; g.M = row_capacity; g.pointwise = 0;
        // K slicing is planned for the capacity; workgroups past the device-side row count exit at once
    }
    plan_slices(g, p);
    const int ntiles = p->ntiles = cdiv(g.M, BM), nnb = p->nnb = g.CoutP / BN;
    const auto unsliced = [&] { p->tile0_tail = ntiles; p->nsplit = 1; p->db = false; };
    const bool ws_ok = workspace && workspace_bytes >= p->ws_bytes;
    if (!ws_ok) unsliced();
    const bool roofline = (flags & LISEC_CONV_TAG_ROOFLINE) != 0;
    // 64-row tiles: asked for by the caller (LISEC_CONV_SMALL_TILE), a candidate of plan_slices, and none of what
    // k_igemm_small does not serve: the per-tile statistics table (laid out for 128-row tiles), BatchNormalization backward
    // on load, the tail contraction, row lists, parity classes, pixel-shuffle stores, the roofline symbols
    const bool small = (flags & LISEC_CONV_SMALL_TILE) && p->tm == 64 && !table_stats && !g.in_y && !(extras && extras->tail_w) &&
                       !row_coords && !g.pc_span && !g.ps && !roofline && (!sk || ws_ok);   // (a sink: the tile pairs meet in the workspace)
    p->tm = BM;
    if (row_coords && !g.in_y && extras && extras->queue && nnb == 1 && ntiles >= resident_slots() && !stats_partials && !g.out_mask &&
        !roofline) {
        g.queue = extras->queue;                     // one un-sliced launch of resident workgroups drawing tiles
        unsliced();
    }
    if (sk) {
        g.sink.acc = static_cast<long long*>(sk->acc);
        g.sink.kind = sk->kind; g.sink.C = g.Cout; g.sink.unbiased = sk->unbiased_moving;
        g.sink.total = (unsigned)ntiles * (unsigned)nnb;          // every (tile, channel slab) stores exactly once
        g.sink.N = sk->n_rows;
        g.sink.gamma = sk->gamma; g.sink.beta = sk->beta; g.sink.mmean = sk->moving_mean; g.sink.mvar = sk->moving_var;
        g.sink.bnstate = sk->bnstate; g.sink.dgamma = sk->dgamma; g.sink.dbeta = sk->dbeta; g.sink.coef = sk->coef;
    }
    p->xf = has_in_bn || (flags & LISEC_CONV_IN_RELU);
    // 3-tap stride-1 pad-1 contraction along w over full lines: the w-halo kernel (one A tile per (kd, kh) pair)
    const bool halo_geom = !g.row_coords && !g.ps && g.ls_w == 0 && g.KW == 3 && g.pw == 1 && g.Wi == g.Wo &&
                           g.Wo >= 64 && g.in_stride % 4 == 0;       // <= 3 lines per 128-row tile
    const bool halo3 = g.Wo < BM - 2;                                // more than two lines per tile possible
    // planes that run different numbers of depth taps: one workgroup per PAIR of planes (see k_igemm_halo) when the layer
    // runs as one launch of the halo kernel and the pairs still fill the chip
    if (tn.plane_pair && !g.in_y && halo_geom && g.Do % 2 == 0 && (g.Ho * g.Wo) % BM == 0 && !g.pc_span &&
        (p->tile0_tail == ntiles || roofline) && (long long)(ntiles / 2) * nnb >= resident_slots()) {
        int lo = 1 << 30, hi = 0;
        for (int d = 0; d < g.Do; ++d) {
            int live = 0;
            for (int kd = 0; kd < g.KD; ++kd) {
                if (c->mode == 0) { const int sd = (d << g.ls_d) - g.pd + kd; live += sd >= 0 && sd < g.Di; }
                else { const int t = d + g.pd - kd; live += t >= 0 && (t & ((1 << g.ls_d) - 1)) == 0 && (t >> g.ls_d) < g.Di; }
            }
            lo = live < lo ? live : lo; hi = live > hi ? live : hi;
        }
        if (lo != hi) { g.plane_tiles = g.Ho * g.Wo / BM; g.plane_pair = 1; }
    }
    // a launch of the tile family over every tile (half as many workgroups with plane_pair), or over the tiles from `tile0`
    TileVariant v{c->mode, p->xf, 0};
    const auto add_tile = [&](dim3 grid, int nsplit = 1, int tile0 = 0) {
        ConvLaunch& l = p->add(ConvLaunch::TILE, grid, kThreads, (v.db ? 2 : 1) * tile_lds_bytes(v.nseg, v.tm));
        l.tile = tile_kernel(v);
        l.nsplit = nsplit; l.tile0 = tile0; l.partial = nsplit > 1;
    };
    if (roofline && !p->xf && !g.in_y) {             // one launch, every tile, under its own symbol
        v.roofline = true;
        v.nseg = halo_geom && !halo3 ? 2 : 0;
        if (!v.nseg) g.plane_pair = 0;
        unsliced();
        p->kernel = v.nseg ? LISEC_KERNEL_HALO2 : LISEC_KERNEL_IGEMM;
        add_tile(dim3(g.plane_pair ? ntiles / 2 : ntiles, nnb, 1));
        return LISEC_OK;
    }
    if (extras && extras->tail_w) {
        LISEC_CHECK_ARG(!g.in_y, "tail: not together with in_y");
        // second contraction on the stored tile: one un-sliced launch of the two-line halo kernel over 64 columns
        LISEC_CHECK_ARG(extras->tail_out && ((uintptr_t)extras->tail_w & 15) == 0 && ((uintptr_t)extras->tail_out & 15) == 0,
                        "tail: packed 64 x 64 kernel and an output, 16-byte aligned");
        LISEC_CHECK_ARG(halo_geom && !halo3 && g.Cout == 64 && g.out_stride == 64 && !g.pc_span && !table_stats &&
                        !(flags & (LISEC_CONV_ACCUMULATE | LISEC_CONV_OUT_RELU)) && (!bwd_stats || sk),
                        "tail: needs the two-line w-halo kernel, Cout = out_stride = 64, no accumulate / ReLU, statistics through a sink");
        g.tail_w = extras->tail_w; g.tail_out = extras->tail_out;
        unsliced();
        p->kernel = LISEC_KERNEL_HALO2;
        v.nseg = 2; v.tail = true;
        add_tile(dim3(g.plane_pair ? ntiles / 2 : ntiles, 1, 1));
        return LISEC_OK;
    }
    {
        int wns = 1;
        size_t wws = 0;
        if (!table_stats && !g.out_mask && !g.in_y && plan_wide(g, &wns, &wws) && (wns == 1 || (workspace && workspace_bytes >= wws))) {
            p->kernel = LISEC_KERNEL_WIDE; p->cols = 128;
            p->nsplit = wns; p->tile0_tail = wns > 1 ? 0 : ntiles; p->ws_bytes = wws; p->db = false;
            g.plane_pair = 0;
            if (sk) g.sink.total = (unsigned)ntiles * (unsigned)(g.CoutP / 128);
            ConvLaunch& l = p->add(ConvLaunch::WIDE, dim3(ntiles, g.CoutP / 128, wns), kWideThreads, wide_lds_bytes());
            l.wide = wide_kernel(c->mode, p->xf);
            l.nsplit = wns; l.partial = true;       // (the kernel does not read it when nsplit == 1)
            return LISEC_OK;
        }
    }
    // Dense(64) and its data gradient: the resident-workgroup kernel
    if (tn.dense64 && !g.in_y && g.pointwise && g.Cin == 64 && g.Cout == 64 && g.in_stride == 64 && g.out_stride == 64 && !g.row_coords &&
        g.M < (1 << 23) &&      // rows x 256 bytes fit a buffer descriptor
        !g.out_mask && !(flags & (LISEC_CONV_ACCUMULATE | LISEC_CONV_TAG_ROOFLINE)) && !table_stats &&
        (!sk || (sk->kind == LISEC_SINK_BACKWARD && bwd_stats)) && !(bwd_stats && !sk) &&
        ntiles >= (g.dw_slabs ? dense_dw_slots() : resident_slots())) {
        p->kernel = LISEC_KERNEL_DENSE64;
        unsliced(); g.plane_pair = 0;
        const int wgs = g.dw_slabs ? dense_dw_slots() : resident_slots();
        if (sk) g.sink.total = (unsigned)wgs;
        p->add(ConvLaunch::RESIDENT, dim3(wgs), kThreads, tile_lds_bytes(0)).resident = dense64_kernel(p->xf, bwd_stats, g.dw_slabs != nullptr);
        return LISEC_OK;
    }
    LISEC_CHECK_ARG(!g.dw_slabs, "dense_dw: not served by this call");
    // the halo kernel slices K by whole A tiles: (kd, kh, channel slab) entries
    const int nstage = g.KD * g.KH * cdiv(g.Cin, BK);
    v.nseg = halo_geom && p->nsplit <= nstage ? (halo3 ? 3 : 2) : 0;
    v.fold = g.in_y != nullptr;                      // (FOLD instantiations: the same launch shapes as the plain ones)
    if (!v.nseg) g.plane_pair = 0;
    if (g.queue) {
        p->kernel = LISEC_KERNEL_QUEUE;
        p->add(ConvLaunch::RESIDENT, dim3(resident_slots()), kThreads, tile_lds_bytes(0)).resident = queue_kernel(c->mode, p->xf);
        return LISEC_OK;
    }
    if (small) {
        // one launch of every 64-row tile on the two-image loop, K sliced as the 128-row plan would be (or not at all)
        const int nt64 = cdiv(g.M, 64);
        p->tm = 64; p->ntiles = nt64; p->db = true;
        p->tile0_tail = p->nsplit > 1 ? 0 : nt64;
        g.plane_pair = 0;
        if (sk) g.sink.total = (unsigned)nt64 * (unsigned)nnb;
        v.tm = 64; v.db = true; v.fold = false;
        v.nseg = v.nseg ? 2 : 0;                     // Wo >= 64: at most two lines per 64-row tile
        p->kernel = v.nseg ? LISEC_KERNEL_HALO2 : LISEC_KERNEL_IGEMM;
        add_tile(dim3(nt64, nnb, p->nsplit), p->nsplit, 0);
        if (sk) p->launch[p->nlaunch - 1].partial = true;
        return LISEC_OK;
    }
    p->kernel = v.nseg == 3 ? LISEC_KERNEL_HALO3 : (v.nseg ? LISEC_KERNEL_HALO2 : LISEC_KERNEL_IGEMM);
    // a layer that would run as two K slices (160-380 tiles): 32-column workgroups over the whole K instead -- as many
    // workgroups, no slabs
    if (tn.half_n && p->nsplit == 2 && p->tile0_tail == 0 && !p->db) {
        unsliced();
        v.cols = p->cols = 32;
        if (sk) g.sink.total = (unsigned)ntiles * (unsigned)cdiv(g.Cout, 32);
        add_tile(dim3(ntiles, cdiv(g.Cout, 32), 1));  // (no workgroups for column blocks beyond Cout: the 16-column heads)
        return LISEC_OK;
    }
    if (p->tile0_tail > 0)                           // whole rounds, single pass
        add_tile(dim3(g.plane_pair ? ntiles / 2 : p->tile0_tail, nnb, 1));
    if (p->tile0_tail < ntiles) {                    // K-sliced tail (or the whole small layer), combined inside the kernel
        v.db = p->db;                                // two LDS images per workgroup (one workgroup per CU)
        add_tile(dim3(ntiles - p->tile0_tail, nnb, p->nsplit), p->nsplit, p->tile0_tail);
    }
    return LISEC_OK;
}
}  // namespace

extern "C" size_t lisec_conv_forward_workspace_bytes(const lisec_conv_geom* c) {
    ConvCall p;
    if (conv_geom_check(c, &p.g)) return 0;
    plan_slices(p.g, &p);
    const size_t plain = p.ws_bytes;
    parity_order(c, &p.g);                            // the order a statistics-free call would use
    plan_slices(p.g, &p);
    size_t w = plain > p.ws_bytes ? plain : p.ws_bytes;
    ConvGeom gw;
    int wns = 1;
    size_t wws = 0;
    if (!conv_geom_check(c, &gw) && plan_wide(gw, &wns, &wws) && wws > w) w = wws;
    return w;
}

extern "C" size_t lisec_conv_forward_rows_workspace_bytes(const lisec_conv_geom* c, int row_capacity) {
    ConvCall p;
    if (conv_geom_check(c, &p.g) || row_capacity <= 0) return 0;
    p.g.M = row_capacity;
    plan_slices(p.g, &p);
    return p.ws_bytes;
}

extern "C" int lisec_conv_plan_query(const lisec_conv_geom* c, int has_in_bnstate, int flags, const lisec_conv_extras* extras,
                                     int has_stats_table, size_t workspace_bytes, int has_row_list, int row_capacity,
                                     lisec_conv_plan* out) {
    LISEC_CHECK_ARG(out, "NULL plan");
    ConvCall p;
    static double dummy_stats;
    static int32_t dummy_rows[4];
    if (int rc = plan_conv(c, has_in_bnstate != 0, flags, extras, has_stats_table ? &dummy_stats : nullptr,
                           workspace_bytes ? &dummy_stats : nullptr, workspace_bytes, has_row_list ? dummy_rows : nullptr,
                           has_row_list ? dummy_rows + 3 : nullptr, row_capacity, &p))
        return rc;
    out->kernel = p.kernel;
    out->cols = p.cols;
    out->tiles = p.ntiles;
    out->tail_tile0 = p.tile0_tail;
    out->k_slices = p.nsplit;
    out->plane_pair = p.g.plane_pair;
    out->parity_classes = p.g.pc_span ? 1 : 0;
    out->double_buffered = p.db ? 1 : 0;
    out->tile_rows = p.tm;
    out->workgroups = 0;
    for (int i = 0; i < p.nlaunch; ++i) out->workgroups += (int)(p.launch[i].grid.x * p.launch[i].grid.y * p.launch[i].grid.z);
    out->launches = p.nlaunch;
    return LISEC_OK;
}

extern "C" int lisec_conv_forward(const lisec_conv_geom* c, const float* in, const float* packed_w,
                                  const float* bias, const float* in_bnstate, int flags, float* out,
                                  double* stats_partials, void* workspace, size_t workspace_bytes,
                                  const int32_t* row_coords, const int32_t* row_count, int row_capacity,
                                  lisec_stream_t stream_) {
    return lisec_conv_forward_masked(c, in, packed_w, bias, in_bnstate, flags, out, nullptr, stats_partials, workspace,
                                     workspace_bytes, row_coords, row_count, row_capacity, stream_);
}

extern "C" int lisec_conv_forward_masked(const lisec_conv_geom* c, const float* in, const float* packed_w,
                                         const float* bias, const float* in_bnstate, int flags, float* out,
                                         const float* out_mask, double* stats_partials, void* workspace,
                                         size_t workspace_bytes, const int32_t* row_coords,
                                         const int32_t* row_count, int row_capacity, lisec_stream_t stream_) {
    lisec_conv_extras ex = {out_mask, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return lisec_conv_forward_ex(c, in, packed_w, bias, in_bnstate, flags, out, &ex, stats_partials, workspace,
                                 workspace_bytes, row_coords, row_count, row_capacity, stream_);
}

extern "C" int lisec_dense_dw_slabs(void) { return dense_dw_slots(); }

extern "C" int lisec_dense_dw_reduce(const float* slabs, float* dW, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(slabs && dW, "NULL tensor pointer");
    LISEC_LAUNCH(k_dense_dw_reduce, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream_), slabs, dense_dw_slots(), dW);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_conv_forward_ex(const lisec_conv_geom* c, const float* in, const float* packed_w,
                                     const float* bias, const float* in_bnstate, int flags, float* out,
                                     const lisec_conv_extras* extras, double* stats_partials, void* workspace,
                                     size_t workspace_bytes, const int32_t* row_coords,
                                     const int32_t* row_count, int row_capacity, lisec_stream_t stream_) {
    ConvCall p;
    if (int rc = plan_conv(c, in_bnstate != nullptr, flags, extras, stats_partials, workspace, workspace_bytes, row_coords,
                           row_count, row_capacity, &p))
        return rc;
    const ConvGeom& g = p.g;
    LISEC_CHECK_ARG(in && packed_w && out, "NULL tensor pointer");
    LISEC_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)packed_w & 15) == 0, "in/weights must be 16-byte aligned");
    LISEC_CHECK_ARG(p.nsplit == 1 || ((uintptr_t)workspace & 15) == 0, "split-K needs a 16-byte aligned workspace");
    if (p.xf && !in_bnstate) {
        // ReLU on load without a BatchNormalization: the kernels always read a (scale, shift) table -- hand them the identity
        in_bnstate = identity_bnstate(g.Cin);
        LISEC_CHECK_ARG(in_bnstate, "LISEC_CONV_IN_RELU without a bnstate supports Cin <= 4096");
    }
    hipStream_t st = static_cast<hipStream_t>(stream_);
    for (int i = 0; i < p.nlaunch; ++i) {
        const ConvLaunch& l = p.launch[i];
        float* partial = l.partial ? static_cast<float*>(workspace) : nullptr;
        switch (l.kind) {
        case ConvLaunch::TILE:
            LISEC_LAUNCH(l.tile, l.grid, l.block, l.lds, st, g, in, packed_w, bias, in_bnstate, flags, out, p.stats, l.nsplit,
                         partial, l.tile0);
            break;
        case ConvLaunch::RESIDENT:
            LISEC_LAUNCH(l.resident, l.grid, l.block, l.lds, st, g, in, packed_w, bias, in_bnstate, flags, out);
            break;
        case ConvLaunch::WIDE:
            LISEC_LAUNCH(l.wide, l.grid, l.block, l.lds, st, g, in, packed_w, bias, in_bnstate, flags, out, p.stats, l.nsplit,
                         partial);
            break;
        }
    }
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

// Diagnostic (not in lisec_hip.h): points k_igemm_halo's stamp buffer at `buf` (device, 8192*8 uint64) or NULL.
extern "C" int lisec_debug_igemm_stamps(unsigned long long* buf) {
    LISEC_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_igemm_stamps), &buf, sizeof(buf)));
    return LISEC_OK;
}
