// Weight gradients of every dense contraction on the fp32 matrix cores (gfx950).
//
//   dW[tap][c][n] = sum_m  A_tap[m][c] * dY[m][n]        (what Keras' fit() derives by autograd for
//   Conv3D / Conv2D / Conv2DTranspose / Dense kernels, model_training.py:184,193,203,246-255,:299)
// A_tap is the same on-the-fly gather (+ BatchNormalization/ReLU of the producing layer applied on
// load) as in igemm.hip; the contraction runs over output positions m, so the GEMM is
// (64 c) x (64 n) with K = M: tiny output, huge K.  Work split:
//   workgroup = (group of KW consecutive taps) x (64-channel c block) x (64-channel n block)
//               x (one of S ranges of 128-row M tiles)
// The dY tile is staged once per M tile and reused by the KW taps of the group; each wave keeps one
// 32x32 accumulator per tap for its whole M range and writes it once to a partial slab
// [S][tap][Cin][Cout]; a second kernel sums the S slabs in index order (deterministic, no atomics)
// into the Keras kernel layout.
// Host side (end of the file): plan_wgrad decides the kernel and its launches from the geometry and the flags alone,
// bind_wgrad puts the tensors and the workspace in, run_wgrad issues them; the plan query and the workspace sizes read
// the same plan.
#include "conv.h"
#include "tile_parts.h"


namespace lisec {
namespace {

constexpr int BMW = 128, BC = 64;                // rows per M tile, channel block
constexpr int kThreads = 256;
constexpr int TILE_FLOATS = BMW * BC;            // 8192 (32 KB)

// diagnostic (tools/wgrad_stamps.py): 100 MHz s_memrealtime stamps of thread 0 of every workgroup at its phase boundaries
// (0 entry, 1 first tile in LDS, 2 loop done, 3 slabs stored; 5 = tiles run, 6 = HW_ID | XCC_ID << 32; 4 / 7 = s_memtime
// shader cycles at 1 / 2: the in-kernel clock of the loop); nullptr = off
__device__ unsigned long long* g_wgrad_stamps = nullptr;
#define WGRAD_STAMP(K_)                                                                                    \
    do {                                                                                                   \
        if (stamps && threadIdx.x == 0 && stamp_wg < 8192) {                                               \
            stamps[(size_t)stamp_wg * 8 + (K_)] = __builtin_amdgcn_s_memrealtime();                        \
            if ((K_) == 1) stamps[(size_t)stamp_wg * 8 + 4] = __builtin_amdgcn_s_memtime();    /* shader cycles: 4, 7 */  \
            if ((K_) == 2) stamps[(size_t)stamp_wg * 8 + 7] = __builtin_amdgcn_s_memtime();                \
            if ((K_) == 0)                                                                                 \
                stamps[(size_t)stamp_wg * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | \
                                                   ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
        }                                                                                                  \
    } while (0)

// RL: row-list instantiation (tiles are tested for work by their decoded row masks, see first_live)
template <int MODE, int TG, bool RL = false>
__global__ void __launch_bounds__(kThreads)
k_wgrad(ConvGeom g, const float* __restrict__ in, const float* __restrict__ in_bn, int flags,
        const float* __restrict__ dy, const float* __restrict__ dy_bn, int nsplit, int tiles_per_split,
        float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned long long* stamps = g_wgrad_stamps;
    const unsigned stamp_wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    WGRAD_STAMP(0);
    float* sA = smem;
    float* sD = smem + TILE_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ngroups = g.KD * g.KH * (g.KW / TG);
    const int split = blockIdx.x / ngroups, group = blockIdx.x - split * ngroups;
    const int tap0 = group * TG;                 // taps tap0 .. tap0+TG-1 share (kd, kh)
    const int c0 = blockIdx.y * BC, n0 = blockIdx.z * BC;
    const int HW = g.Ho * g.Wo;
    const int mlimit = row_limit(g);
    const int ntiles = (mlimit + BMW - 1) / BMW;
    // dense rows: split s owns the tiles [s * tiles_per_split, ...).  Row lists: the launch is sized for the CAPACITY but
    // only the tiles below the device-side count hold rows, so split s takes tiles s, s + nsplit, s + 2 nsplit, ... --
    // every split gets its share of the live tiles whatever their number (84 000 of 200 000 rows: contiguous ranges left
    // 58 % of the workgroups without a row and 14 tiles to each of the others)
    const int ts = RL ? nsplit : 1;
    const int t_begin = RL ? split : split * tiles_per_split;
    const int t_end = RL ? ntiles : (t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles);
    const int kd = tap0 / (g.KH * g.KW), kh = (tap0 / g.KW) % g.KH, kw0 = tap0 % g.KW;

    const int piece = tid & 15;
    const int cA = c0 + piece * 4, cD = n0 + piece * 4;
    const bool cokA = cA < g.Cin, cokD = cD < g.Cout;
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    if (in_bn && cokA) {
        tsc = *reinterpret_cast<const float4*>(in_bn + cA);
        tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cA);
    }
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;
    float4 dsc = make_float4(1, 1, 1, 1), dsh = make_float4(0, 0, 0, 0);
    if (dy_bn && cokD) {
        dsc = *reinterpret_cast<const float4*>(dy_bn + cD);
        dsh = *reinterpret_cast<const float4*>(dy_bn + g.Cout + cD);
    }
    const float drelu_lo = (flags & LISEC_CONV_DY_RELU) ? 0.f : -INFINITY;
    unsigned dvalid = 0;

    f32x16 acc[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) acc[t] = (f32x16){0};

    float4 ra[8], rd[8];
    unsigned valid_mask = 0;
    RowGather rows[8];

    auto decode_rows = [&](int tile) {
#pragma unroll
        for (int p = 0; p < 8; ++p) rows[p] = row_gather(g, tile * BMW + p * 16 + (tid >> 4), MODE, cA);
    };
    auto tile_live = [&](int tile) -> bool {     // whole tile outside the valid depth range of this tap group
        if (g.row_coords) return true;
        int mfirst = tile * BMW, mlast = mfirst + BMW - 1 < g.M ? mfirst + BMW - 1 : g.M - 1;
        int df = mfirst / HW, dl = mlast / HW;
        if (df != dl) return true;
        int tmp;
        return (axis_mask(df, g.KD, g.ls_d, g.pd, g.Di, MODE, tmp) >> kd) & 1;
    };
    auto load_a = [&](int kw) {
        const int soff = tap_delta(g, kd, kh, kw, MODE);
        const int tbits = cokA ? tap_bits(kd, kh, kw) : 0x7fffffff;
        valid_mask = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const bool ok = (rows[p].mask & tbits) == tbits;
            const int off = ok ? rows[p].off + soff : 0;
            ra[p] = *reinterpret_cast<const float4*>(in + off);
            valid_mask |= ok ? (1u << p) : 0u;
        }
    };
    auto load_d = [&](int tile) {
        dvalid = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int m = tile * BMW + p * 16 + (tid >> 4);
            const bool ok = m < mlimit && cokD;                      // branch-free: rows beyond the layer read element 0
            rd[p] = *reinterpret_cast<const float4*>(dy + (ok ? (size_t)m * g.out_stride + cD : (size_t)0));
            dvalid |= ok ? (1u << p) : 0u;
        }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            float4 v = ra[p];
            const bool ok = (valid_mask >> p) & 1;
            affine_relu(v, tsc, tsh, relu_lo, ok);
            *reinterpret_cast<float4*>(sA + (p * 16 + (tid >> 4)) * BC + piece * 4) = v;
        }
    };
    auto store_d = [&]() {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            float4 v = rd[p];
            const bool ok = (dvalid >> p) & 1;
            affine_relu(v, dsc, dsh, drelu_lo, ok);
            *reinterpret_cast<float4*>(sD + (p * 16 + (tid >> 4)) * BC + piece * 4) = v;
        }
    };

    // MFMA 32x32x2: A operand lane(i = c, h) <- A_tap[m = 8*kk + 4h + j][c]; B operand lane(h, n) <- dY[m][n]
    const float* aCol = sA + (4 * (lane >> 5)) * BC + (wave >> 1) * 32 + (lane & 31);
    const float* dCol = sD + (4 * (lane >> 5)) * BC + (wave & 1) * 32 + (lane & 31);

    // step list: (tile, t) with t in [0, TG); dY is staged with t == 0
    // first tile >= `tile` with work for this tap group; its row descriptors are decoded on return.  Row lists: the
    // voxels are sorted by cell, so most tiles share one depth (parity) and whole (kd, kh) groups fall away
    const int gbits = (1 << kd) | (16 << kh);
    auto first_live = [&](int tile) -> int {
        if (!RL) {
            while (tile < t_end && !tile_live(tile)) ++tile;
            if (tile < t_end) decode_rows(tile);
            return tile;
        }
        for (; tile < t_end; tile += ts) {
            decode_rows(tile);
            int pred = 0;
#pragma unroll
            for (int p = 0; p < 8; ++p) pred |= (rows[p].mask & gbits) == gbits;
            if (__syncthreads_or(pred)) break;
        }
        return tile;
    };
    int tile = first_live(t_begin);
    int t = 0;
    if (tile < t_end) {
        load_a(kw0);
        load_d(tile);
        store_a();
        store_d();
    }
    __syncthreads();
    WGRAD_STAMP(1);
    int stamp_tiles = 0;
    while (tile < t_end) {
        stamp_tiles += t == 0;
        // next step
        int ntile = tile, nt = t + 1;
        if (nt == TG) {
            nt = 0;
            ntile = first_live(ntile + ts);
        }
        const bool more = ntile < t_end;
        if (more) {
            if (nt == 0) load_d(ntile);
            load_a(kw0 + nt);
        }
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) {
            if (tt == t) {
#pragma unroll 4
                for (int kk = 0; kk < BMW / 8; ++kk) {
                    const float* ap = aCol + kk * 8 * BC;
                    const float* dp = dCol + kk * 8 * BC;
                    const float a0 = ap[0], a1 = ap[BC], a2 = ap[2 * BC], a3 = ap[3 * BC];
                    const float b0 = dp[0], b1 = dp[BC], b2 = dp[2 * BC], b3 = dp[3 * BC];
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[tt], 0, 0, 0);
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[tt], 0, 0, 0);
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, acc[tt], 0, 0, 0);
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc[tt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        if (more) {
            store_a();
            if (nt == 0) store_d();
        }
        __syncthreads();
        tile = ntile;
        t = nt;
    }

    WGRAD_STAMP(2);
    // partial slab [split][tap][Cin][Cout]; C layout: col = lane&31 (n), row = (r&3)+8*(r>>2)+4*(lane>>5) (c)
    const int ntaps = g.KD * g.KH * g.KW;
#pragma unroll
    for (int tt = 0; tt < TG; ++tt) {
        float* base = partial + ((size_t)split * ntaps + tap0 + tt) * g.Cin * g.Cout;
        const int n = n0 + (wave & 1) * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + (wave >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (c < g.Cin && n < g.Cout) base[(size_t)c * g.Cout + n] = acc[tt][r];
        }
    }
    WGRAD_STAMP(3);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)stamp_tiles;
}


// ---- halo variant: stride-1 (along w) 3-tap convolutions, dense positions -------------------------------------
// A tile is a run of up to 128 consecutive w' inside ONE output line (d',h'); for the workgroup's (kd,kh) the
// three kw taps read the same source line shifted by one position, so the source rows w0-pw .. w0-pw+len+1 are
// staged ONCE (zero outside the map) and tap kw reads LDS rows j+kw: half the global->LDS traffic of the generic
// kernel, no per-row address arithmetic, and 3x longer MFMA runs between barriers.  The contraction runs over the
// rows; the tiles of a line are made equal (W' = 400 -> 4 x 100 rows) so that no short tail tile pays a full staging round.

// The (kd, kh) groups a launch runs: groups no output line can read (depth stride 2 over a two-plane input: a third of
// them) get no workgroups at all.
struct LiveGroups { int n; unsigned char id[16]; };

// One weight-gradient contraction as the halo kernel sees it: single launches pass one, batched launches a table of them.
struct WgradItem {
    ConvGeom g;
    const float* in; const float* in_bn; const float* dy;
    float* partial;          // slabs (combine: in the accumulator register layout, behind the arrival counters)
    float* dW;               // combine: the finished kernel gradient is written by the last slice to arrive
    int* counters;           // combine: one arrival counter per (group, c block, n block), zero between calls
    int flags, nsplit, tiles_per_split, flip, LT, transpose, combine;
    int gx, gy, gz;          // grid of this item: gx = nsplit * groups
    LiveGroups live;
};

// Slab of one (slice, cell) in the register layout: [wave 4][q 12 = 3 taps x 4 float4][lane 64] float4 = 48 KB.
constexpr int kWSlabF4 = 4 * 12 * 64;
constexpr int kWgradCounters = 4096;

// NP: staging passes of 16 rows.  7 (tiles of <= 104 rows: the 400-wide middle layers run 4 x 100) needs 12 registers
// fewer than 9 and, with the fragment reads software-pipelined by hand, fits three workgroups per CU.  The bound is on DR,
// not on LT: the last 8-row chunk reads the A image up to row DR + 1, so the passes must cover DR + 2 <= NP * 16 rows
// (LT = 105 .. 110 has DR = 112: rows 112 and 113 lie beyond seven passes and would be read as stale LDS).
template <bool XF, int NP>
__device__ __forceinline__ void
wgrad_halo_body(const WgradItem& it, const int bx, const int by, const int bz, float* smem, unsigned long long* stamps,
                const unsigned stamp_wg) {
    constexpr int PA = NP, PD = NP == 7 ? 7 : 8;
    const ConvGeom& g = it.g;
    const float* __restrict__ in = it.in;
    const float* __restrict__ in_bn = it.in_bn;
    const float* __restrict__ dy = it.dy;
    float* __restrict__ partial = it.partial;
    const int flags = it.flags, nsplit = it.nsplit, tiles_per_split = it.tiles_per_split, flip = it.flip, LT = it.LT;
    const LiveGroups& live = it.live;
    (void)nsplit;
    // LT <= 128: rows per tile, chosen by the host so that the tiles of one line are equal (W' = 400 -> 4 x 100) and,
    // with DR = LT rounded up to 8, the workgroup's LDS is (2 DR + 2) x 256 B: 53 760 B at LT = 100, three per CU
    WGRAD_STAMP(0);
    const int DR = (LT + 7) & ~7;
    float* sA = smem;                                  // [DR + 2][64]: halo rows, zero beyond len + 2
    float* sD = smem + (DR + 2) * BC;                  // [DR][64]: dY rows, zero beyond len
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ngroups = live.n;
    const int split = bx / ngroups, gslot = bx - split * ngroups, group = live.id[gslot];
    const int kd = group / g.KH, kh = group - kd * g.KH;
    const int c0 = by * BC, n0 = bz * BC;
    const int tpl = (g.Wo + LT - 1) / LT;              // tiles per output line
    const int ntiles = g.Do * g.Ho * tpl;
    const int t_begin = split * tiles_per_split;
    const int t_end = t_begin + tiles_per_split < ntiles ? t_begin + tiles_per_split : ntiles;

    const int piece = tid & 15, rsub = tid >> 4;       // 16 rows x 16 pieces per pass
    const int cA = c0 + piece * 4, cD = n0 + piece * 4;
    const bool cokA = cA < g.Cin, cokD = cD < g.Cout;
    float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
    if (XF && in_bn && cokA) {
        tsc = *reinterpret_cast<const float4*>(in_bn + cA);
        tsh = *reinterpret_cast<const float4*>(in_bn + g.Cin + cA);
    }
    const float relu_lo = (flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;

    f32x16 acc0 = {0}, acc1 = {0}, acc2 = {0};
    float4 ra[PA], rd[PD];
    unsigned amask = 0, dmask = 0;
    int cur_len = 0, nxt_len = 0;

    // tile -> (output line, w0, len, source line offset or -1)
    auto tile_info = [&](int tile, int& w0, int& len, long long& src_line, long long& dy_line) -> bool {
        const int line = tile / tpl;
        w0 = (tile - line * tpl) * LT;
        len = g.Wo - w0 < LT ? g.Wo - w0 : LT;
        const int d = line / g.Ho, h = line - d * g.Ho;
        const int sd = (d << g.ls_d) - g.pd + kd, sh = (h << g.ls_h) - g.ph + kh;
        dy_line = (long long)line * g.Wo;
        src_line = ((long long)sd * g.Hi + sh) * g.Wi;
        return sd >= 0 && sd < g.Di && sh >= 0 && sh < g.Hi;
    };
    auto next_live = [&](int tile) -> int {
        int w0, len; long long a, b;
        while (tile < t_end && !tile_info(tile, w0, len, a, b)) ++tile;
        return tile;
    };
    auto issue = [&](int tile) {
        int w0, len; long long src_line, dy_line;
        (void)tile_info(tile, w0, len, src_line, dy_line);
        nxt_len = len;
        amask = 0;
        dmask = 0;
#pragma unroll
        for (int p = 0; p < PA; ++p) {                 // halo rows: slot s <-> source w = w0 - pw + s
            const int s_ = p * 16 + rsub;
            const int sw = w0 - g.pw + s_;
            const bool ok = cokA && s_ < len + 2 && sw >= 0 && sw < g.Wi;
            const long long off = ok ? (src_line + sw) * g.in_stride + cA : 0;
            ra[p] = *reinterpret_cast<const float4*>(in + off);
            amask |= ok ? (1u << p) : 0u;
        }
#pragma unroll
        for (int p = 0; p < PD; ++p) {
            const int j = p * 16 + rsub;
            const bool ok = cokD && j < len;
            const long long off = ok ? (dy_line + w0 + j) * g.out_stride + cD : 0;
            rd[p] = *reinterpret_cast<const float4*>(dy + off);      // (zeroed in store(): a select here would make the
            dmask |= ok ? (1u << p) : 0u;                            //  wave wait for the load before its MFMAs)
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int s_ = p * 16 + rsub;
            if (s_ < DR + 2) {
                float4 v = ra[p];
                const bool ok = (amask >> p) & 1;
                if (XF) affine_relu(v, tsc, tsh, relu_lo, ok);
                else masked(v, ok);
                *reinterpret_cast<float4*>(sA + s_ * BC + piece * 4) = v;
            }
        }
#pragma unroll
        for (int p = 0; p < PD; ++p)
            if (p * 16 + rsub < DR)
                *reinterpret_cast<float4*>(sD + (p * 16 + rsub) * BC + piece * 4) = (dmask >> p) & 1 ? rd[p] : make_float4(0, 0, 0, 0);
        cur_len = nxt_len;
    };

    const float* aCol = sA + (4 * (lane >> 5)) * BC + (wave >> 1) * 32 + (lane & 31);
    const float* dCol = sD + (4 * (lane >> 5)) * BC + (wave & 1) * 32 + (lane & 31);

    int tile = next_live(t_begin);
    if (tile < t_end) { issue(tile); store(); }
    __syncthreads();
    WGRAD_STAMP(1);
    int stamp_tiles = 0;
    while (tile < t_end) {
        ++stamp_tiles;
        const int ntile = next_live(tile + 1);
        if (ntile < t_end) issue(ntile);
        const int nk = (cur_len + 7) >> 3;             // rows beyond len are zero in sD: whole 8-row chunks only
        wgrad_chunks<BC>(aCol, dCol, nk, acc0, acc1, acc2);
        __syncthreads();
        if (ntile < t_end) store();
        __syncthreads();
        tile = ntile;
    }

    WGRAD_STAMP(2);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)stamp_tiles;
    const int ntaps = g.KD * g.KH * g.KW;
    const int tap0 = (kd * g.KH + kh) * g.KW;
    const int n = n0 + (wave & 1) * 32 + (lane & 31);
    float* out_base = partial;
    size_t out_split = (size_t)split;
    bool transpose = false;
    if (it.combine) {
        // The slices of a cell (group, c block, n block) meet here, as the K slices of a tile do in igemm.hip: slab stores in
        // the register layout (write-through), every wave waits for its stores, barrier, ONE lane's agent-scope ticket; the
        // last slice to arrive adds the slabs in slice order (deterministic) and writes the finished gradient -- no slab-sum
        // launch.  Used when a cell has few slices (the RPN maps); many slices (the middle layers) keep the slab-sum kernel.
        // (the "last" word in the dynamic LDS, free by now: a static word on top of LT = 100's 53 760 B rounds the allocation
        // past a third of the CU's 160 KB and the kernel drops from three to two workgroups per CU)
        const int ncell = ngroups * it.gy * it.gz, cell = (gslot * it.gy + by) * it.gz + bz;
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(partial, 0, (int)((size_t)it.nsplit * ncell * kWSlabF4 * 16),
                                                                      0x00020000);
        const unsigned lane_off = (unsigned)((wave * 12) * 64 + lane) * 16u;
        slab_store<12>(acc0, acc1, acc2, rs, (unsigned)(((size_t)split * ncell + cell) * kWSlabF4 * 16) + lane_off);
        if (!slice_ticket(it.counters + cell, it.nsplit, reinterpret_cast<int*>(smem))) { WGRAD_STAMP(3); return; }
        slab_sum<false, 12>(acc0, acc1, acc2, rs, (unsigned)((size_t)cell * kWSlabF4 * 16) + lane_off, (unsigned)((size_t)ncell * kWSlabF4 * 16), it.nsplit);
        out_base = it.dW; out_split = 0; transpose = it.transpose != 0;
    }
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
        // flip: a stride-1 transposed gather (o + p - k) run as the plain one (o - (K-1-p) + k') with k' = K-1-k
        const int tap = flip ? ((g.KD - 1 - kd) * g.KH + (g.KH - 1 - kh)) * g.KW + (2 - tt) : tap0 + tt;
        float* base = out_base + (out_split * ntaps + tap) * g.Cin * g.Cout;
        const f32x16& acc = tt == 0 ? acc0 : (tt == 1 ? acc1 : acc2);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + (wave >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (c < g.Cin && n < g.Cout) {
                if (transpose) base[(size_t)n * g.Cin + c] = acc[r];          // (taps, Cout, Cin): the Conv2DTranspose layout
                else base[(size_t)c * g.Cout + n] = acc[r];
            }
        }
    }
    WGRAD_STAMP(3);
}

template <bool XF, int NP>
__global__ void __launch_bounds__(kThreads, NP == 7 ? 3 : 2)
k_wgrad_halo(WgradItem it) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    wgrad_halo_body<XF, NP>(it, blockIdx.x, blockIdx.y, blockIdx.z, smem, g_wgrad_stamps,
                            (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// Several contractions in ONE launch (the stride-1 convolutions of an RPN block: up to five layers whose maps hold 1 250 -
// 20 000 positions and fill a fraction of the chip each): workgroup -> (item, block of that item's grid).
constexpr int kBatchMax = 6;
struct WgradBatch { int n; int first[kBatchMax + 1]; WgradItem item[kBatchMax]; };
template <bool XF, int NP>
__global__ void __launch_bounds__(kThreads, NP == 7 ? 3 : 2)
k_wgrad_halo_batch(WgradBatch b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.first[i + 1]) ++i;
    const WgradItem& it = b.item[i];
    const int local = blockIdx.x - b.first[i];
    const int bx = local % it.gx, by = (local / it.gx) % it.gy, bz = local / (it.gx * it.gy);
    wgrad_halo_body<XF, NP>(it, bx, by, bz, smem, g_wgrad_stamps, blockIdx.x);
}

// ---- ring variant (round 4): 3 x 3 taps in (h, w) at stride 1, dense positions ------------------------------------------
// The halo kernel gives every (kd, kh) group its own workgroups, so each of them re-reads x and dY: nine passes over both
// operands for a Conv3D (PMC: 573 MB per launch of the second middle block against 123 MB algorithmic), and each workgroup
// stages 202 rows for 3 taps.  Here ONE workgroup owns a run of consecutive output lines h0 .. h1 of one column
//   (cell = 64 c x 64 n block, kd, output plane d, w segment)
// and computes all NINE (kh, kw) taps: 12 waves = 3 kh x 4 quadrants of the 64 x 64 cell, three accumulators (kw) per wave --
// the inner loop of the halo kernel, unchanged.  Output line h reads the input lines h - ph + kh; moving to h + 1 needs ONE new
// line, so the three x lines live in a 3-slot LDS ring and every input line and every dY line is staged once per run:
// 202 rows per 9 taps.  LDS (3 (DR + 2) + DR) x 256 B = 108 032 B at 100-row tiles: one of these and one 52 KB workgroup
// of the data-gradient chain per CU (85 + 41 of the 128 granules).  Slabs are written in the accumulator register layout
// [slice][cell][wave 12][q 12][lane 64] float4 and summed in slice order: by the last slice to arrive when a cell has few
// slices (RPN maps), by k_wgrad_ring_reduce otherwise (the middle layers).
constexpr int kRingThreads = 768;
constexpr int kRSlabF4 = 12 * 12 * 64;             // float4 per (slice, cell): 147 456 B

struct RingGeom {
    int Di, Hi, Wi, Do, Ho, Wo, KD;
    int ls_d, pd, ph, pw;
    int Cin, in_stride, Cout, out_stride;
};

struct RingItem {
    RingGeom g;
    const float* in; const float* in_bn; const float* dy;
    float* slabs;            // behind the arrival counters of the workspace
    float* dW;
    int* counters;           // combine: one arrival counter per cell (kd, c block, n block), zero between calls
    int flags, flip, LT, transpose, combine;
    int R;                   // runs per column
    int tpl;                 // tiles (w segments) per output line
    int npairs;              // (kd, d) pairs whose input plane exists
    int gy, gz;              // c blocks, n blocks
    int nblocks;             // workgroups of this item = gy * gz * tpl * R * npairs
    int ncells;              // KD * gy * gz
    int kd_slices[4];        // slices per cell of depth tap kd = (planes d that kd reads) * tpl * R
    unsigned char pair_kd[16], pair_d[16], pair_rank[16];   // rank: index of d among the planes kd reads
};

// (wave, q, lane, j) of the register layout -> (tap, c, n) of the kernel gradient
__device__ __forceinline__ void ring_store_out(const RingItem& it, int kd, int c0, int n0, int wave, int q, int lane, float4 v) {
    const RingGeom& g = it.g;
    const int kh = wave >> 2, quad = wave & 3, tt = q >> 2, i = q & 3;
    const int tap = it.flip ? ((g.KD - 1 - kd) * 3 + (2 - kh)) * 3 + (2 - tt) : (kd * 3 + kh) * 3 + tt;
    const int c = c0 + (quad >> 1) * 32 + 8 * i + 4 * (lane >> 5);
    const int n = n0 + (quad & 1) * 32 + (lane & 31);
    if (n >= g.Cout || c >= g.Cin) return;
    const float e[4] = {v.x, v.y, v.z, v.w};
    if (it.transpose) {                              // (taps, Cout, Cin): the Conv2DTranspose layout
        float* o = it.dW + ((size_t)tap * g.Cout + n) * g.Cin + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c + j < g.Cin) o[j] = e[j];
    } else {
        float* o = it.dW + ((size_t)tap * g.Cin + c) * g.Cout + n;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c + j < g.Cin) o[(size_t)j * g.Cout] = e[j];
    }
}

template <bool XF, int NP>
__device__ __forceinline__ void
wgrad_ring_body(const RingItem& it, const int bx, float* smem, unsigned long long* stamps, const unsigned stamp_wg) {
    const RingGeom& g = it.g;
    const float* __restrict__ in = it.in;
    const float* __restrict__ dy = it.dy;
    WGRAD_STAMP(0);
    const int LT = it.LT, DR = (LT + 7) & ~7;
    const int SLOT = (DR + 2) * BC;                    // floats per x line slot
    float* sX = smem;                                  // [3][DR + 2][64]
    float* sD = smem + 3 * SLOT;                       // [DR][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = wave >> 2, quad = wave & 3;
    // workgroup -> (cell, w segment, run, (kd, d) pair); the pairs of one place are neighbours on one XCD: they share
    // the dY lines (same d) or the x planes
    int id = xcd_remap(bx, it.nblocks);
    const int pair = id % it.npairs; id /= it.npairs;
    const int run = id % it.R; id /= it.R;
    const int wseg = id % it.tpl; id /= it.tpl;
    const int bz = id % it.gz, by = id / it.gz;
    const int kd = it.pair_kd[pair], d = it.pair_d[pair];
    const int h0 = (int)((long long)run * g.Ho / it.R), h1 = (int)((long long)(run + 1) * g.Ho / it.R);
    const int sd = (d << g.ls_d) - g.pd + kd;          // exists: the host lists only such pairs
    const int w0 = wseg * LT;
    const int len = g.Wo - w0 < LT ? g.Wo - w0 : LT;
    const int c0 = by * BC, n0 = bz * BC;
    const int piece = tid & 15, rsub = tid >> 4;       // 48 rows x 16 pieces per pass
    const int cA = c0 + piece * 4, cD = n0 + piece * 4;
    const bool cokA = cA < g.Cin, cokD = cD < g.Cout;
    // the on-load affine of the x operand lives in LDS (behind the dY tile), not in eight registers per lane
    float* sT = sD + DR * BC;                          // [2][64]: scale, shift of this workgroup's 64 input channels
    if (XF && tid < 32) {
        const int cc = c0 + (tid & 15) * 4;
        const bool sh_ = tid >= 16;
        float4 v = sh_ ? make_float4(0, 0, 0, 0) : make_float4(1, 1, 1, 1);
        if (it.in_bn && cc < g.Cin) v = *reinterpret_cast<const float4*>(it.in_bn + (sh_ ? g.Cin : 0) + cc);
        *reinterpret_cast<float4*>(sT + (sh_ ? BC : 0) + (tid & 15) * 4) = v;
    }
    if (XF) __syncthreads();
    const float relu_lo = (it.flags & LISEC_CONV_IN_RELU) ? 0.f : -INFINITY;

    f32x16 acc0 = {0}, acc1 = {0}, acc2 = {0};
    // Staging: ONE register array for the two things a step brings in.  Pass p handles row p * 48 + rsub of the virtual
    // image [x line A: DR + 2 rows][second source: an x line (warm-up) or a dY line (DR rows)]: 5 float4 per thread at
    // 100-row tiles.  Buffer loads against a descriptor that covers exactly ONE line (x) / one tile (dY): rows before
    // the line (negative offset), beyond its end, beyond the tile's rows and channel pieces beyond Cin / Cout read as
    // zeros -- no predicates, no masks, no 64-bit lane addresses.
    u32x4 rr[NP];
    const int XR = DR + 2;
    const int strideX4 = g.in_stride * 4, strideD4 = g.out_stride * 4;                   // bytes per row
    const int voffX = cokA ? (w0 - g.pw + rsub) * strideX4 + cA * 4 : 0x40000000;        // (0x40000000: beyond any line)
    const int voffD = cokD ? rsub * strideD4 + cD * 4 : 0x40000000;
    const int recX = ((g.Wi - 1) * g.in_stride + g.Cin) * 4;
    const int recD = ((len - 1) * g.out_stride + g.Cout) * 4;
    auto x_rsrc = [&](int sh) {
        const bool lv = sh >= 0 && sh < g.Hi;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in) + ((long long)sd * g.Hi + (lv ? sh : 0)) * g.Wi * g.in_stride,
                                                 0, lv ? recX : 0, 0x00020000);
    };
    auto load2 = [&](int shA, bool second_is_x, int lineB) {          // lineB: input line (x) or output line h (dY)
        __amdgpu_buffer_rsrc_t rsA = x_rsrc(shA);
        __amdgpu_buffer_rsrc_t rsB = second_is_x
            ? x_rsrc(lineB)
            : __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy) + (((long long)d * g.Ho + lineB) * g.Wo + w0) * g.out_stride,
                                                0, recD, 0x00020000);
        const int voffB = second_is_x ? voffX : voffD, strideB4 = second_is_x ? strideX4 : strideD4;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (p * 48 + rsub < XR) rr[p] = __builtin_amdgcn_raw_buffer_load_b128(rsA, voffX + p * 48 * strideX4, 0, 0);
            else                    rr[p] = __builtin_amdgcn_raw_buffer_load_b128(rsB, voffB + (p * 48 - XR) * strideB4, 0, 0);
        }
    };
    auto store2 = [&](int shA, bool second_is_x, int lineB) {
        float4 tsc = make_float4(1, 1, 1, 1), tsh = make_float4(0, 0, 0, 0);
        if (XF) {
            tsc = *reinterpret_cast<const float4*>(sT + piece * 4);
            tsh = *reinterpret_cast<const float4*>(sT + BC + piece * 4);
        }
        float* dA = sX + ((shA + 3) % 3) * SLOT;
        float* dB = second_is_x ? sX + ((lineB + 3) % 3) * SLOT : sD;
        const int rowsB = second_is_x ? XR : DR;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = p * 48 + rsub;
            const bool first = row < XR;
            const int s_ = first ? row : row - XR;
            if (row < XR + rowsB) {
                float4 v = make_float4(__uint_as_float(rr[p].x), __uint_as_float(rr[p].y), __uint_as_float(rr[p].z),
                                       __uint_as_float(rr[p].w));
                if (XF && (first || second_is_x)) {
                    // the affine turns the zeros of the padding into max(shift, 0): the halo rows outside the map are
                    // zeroed again (rows beyond the tile only meet zero dY rows: any finite value does)
                    const int sw = w0 - g.pw + s_;
                    const bool keep = sw >= 0 && sw < g.Wi;
                    affine_relu(v, tsc, tsh, relu_lo, keep);
                }
                *reinterpret_cast<float4*>((first ? dA : dB) + s_ * BC + piece * 4) = v;
            }
        }
    };

    // warm-up: the two lines below the first output line's newest one, then the first tile
    load2(h0 - g.ph, true, h0 - g.ph + 1);
    store2(h0 - g.ph, true, h0 - g.ph + 1);
    load2(h0 - g.ph + 2, false, h0);
    store2(h0 - g.ph + 2, false, h0);
    __syncthreads();
    WGRAD_STAMP(1);

    const float* dCol = sD + (4 * (lane >> 5)) * BC + (quad & 1) * 32 + (lane & 31);
    const int aoff = (4 * (lane >> 5)) * BC + (quad >> 1) * 32 + (lane & 31);
    const int nk = (len + 7) >> 3;                     // rows beyond len are zero in sD: whole 8-row chunks only
    for (int h = h0; h < h1; ++h) {
        const bool more = h + 1 < h1;
        if (more) load2(h + 3 - g.ph, false, h + 1);
        const int sh = h - g.ph + kh;                  // this wave's input line (wave-uniform)
        if (sh >= 0 && sh < g.Hi) {
            const float* aCol = sX + ((sh + 3) % 3) * SLOT + aoff;
            wgrad_chunks<BC>(aCol, dCol, nk, acc0, acc1, acc2);
        }
        __syncthreads();
        if (more) store2(h + 3 - g.ph, false, h + 1);                // the slot of line h - ph: no tile reads it again
        __syncthreads();
    }
    WGRAD_STAMP(2);
    if (stamps && threadIdx.x == 0 && stamp_wg < 8192) stamps[(size_t)stamp_wg * 8 + 5] = (unsigned long long)(h1 - h0);

    // slab of this slice, register layout, write-through
    const int cell = (kd * it.gy + by) * it.gz + bz;
    const int slice = (it.pair_rank[pair] * it.tpl + wseg) * it.R + run;
    const int nsl = it.kd_slices[kd];
    int smax = it.kd_slices[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) smax = it.kd_slices[k] > smax ? it.kd_slices[k] : smax;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(it.slabs, 0, (int)((size_t)smax * it.ncells * kRSlabF4 * 16),
                                                                  0x00020000);
    const unsigned lane_off = (unsigned)((wave * 12) * 64 + lane) * 16u;
    slab_store<12>(acc0, acc1, acc2, rs, (unsigned)(((size_t)slice * it.ncells + cell) * kRSlabF4 * 16) + lane_off);
    if (!it.combine) { WGRAD_STAMP(3); return; }
    // few slices per cell: they meet here as the K slices of a tile do in igemm.hip; the last one to arrive adds the slabs
    // in slice order and writes the finished gradient (the "last" word: the dynamic LDS, free by now)
    if (!slice_ticket(it.counters + cell, nsl, reinterpret_cast<int*>(smem))) { WGRAD_STAMP(3); return; }
    slab_sum<false, 12>(acc0, acc1, acc2, rs, (unsigned)((size_t)cell * kRSlabF4 * 16) + lane_off, (unsigned)((size_t)it.ncells * kRSlabF4 * 16), nsl);
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const f32x16& a = q < 4 ? acc0 : (q < 8 ? acc1 : acc2);
        const int r = (q & 3) * 4;
        ring_store_out(it, kd, c0, n0, wave, q, lane, make_float4(a[r], a[r + 1], a[r + 2], a[r + 3]));
    }
    WGRAD_STAMP(3);
}

// <= 120 registers: three of these waves and one 148-register wave of the data-gradient chain share a SIMD's 512
template <bool XF, int NP>
__global__ void __launch_bounds__(kRingThreads) __attribute__((amdgpu_num_vgpr(120)))
k_wgrad_ring(RingItem it) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    wgrad_ring_body<XF, NP>(it, blockIdx.x, smem, g_wgrad_stamps, blockIdx.x);
}

struct RingBatch { int n; int first[kBatchMax + 1]; RingItem item[kBatchMax]; };
template <bool XF, int NP>
__global__ void __launch_bounds__(kRingThreads) __attribute__((amdgpu_num_vgpr(120)))
k_wgrad_ring_batch(RingBatch b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.first[i + 1]) ++i;
    wgrad_ring_body<XF, NP>(b.item[i], blockIdx.x - b.first[i], smem, g_wgrad_stamps, blockIdx.x);
}

// Slab sum of the ring kernel for cells with many slices (the middle layers: 60 - 80 slices of 147 KB per cell): one WAVE per
// 8 float4 of a cell's slab, lane = 8 * group + t sums the slices group, group + 8, ... of float4 t (four loads in
// flight), then the eight partial sums are added across lanes in a fixed tree; <= 56 registers, no LDS (k_wgrad_reduce_lanes
// says why).  A depth tap no plane reads (kd_slices == 0) gets zeros.
__global__ void __launch_bounds__(256, 8)
k_wgrad_ring_reduce(RingItem it) {
    const int lane = threadIdx.x & 63, tx = lane & 7, ty = lane >> 3;
    const long long i4 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + tx;
    const long long total = (long long)it.ncells * kRSlabF4;
    const long long ii = i4 < total ? i4 : 0;
    const int cell = (int)(ii / kRSlabF4), e = (int)(ii - (long long)cell * kRSlabF4);
    const int kd = cell / (it.gy * it.gz);
    const int nsl = it.kd_slices[kd];
    float4 s = make_float4(0, 0, 0, 0);
    if (i4 < total) {
        const float4* src = reinterpret_cast<const float4*>(it.slabs) + (size_t)cell * kRSlabF4 + e;
        const size_t zs = (size_t)it.ncells * kRSlabF4;
        int k = ty;
        for (; k + 3 * 8 < nsl; k += 4 * 8) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(k + 8 * u) * zs];
#pragma unroll
            for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        for (; k < nsl; k += 8) {
            const float4 v = src[(size_t)k * zs];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
        s.x += __shfl_down(s.x, o, 64); s.y += __shfl_down(s.y, o, 64);
        s.z += __shfl_down(s.z, o, 64); s.w += __shfl_down(s.w, o, 64);
    }
    if (ty != 0 || i4 >= total) return;
    const int rem = cell - kd * it.gy * it.gz;
    const int by = rem / it.gz, bz = rem - by * it.gz;
    ring_store_out(it, kd, by * BC, bz * BC, e / 768, (e >> 6) % 12, e & 63, s);
}

// dW = sum over splits (index order).  transpose: write [tap][n][c] (Conv2DTranspose kernels are (kh,kw,out,in)).
// One thread per float4 of the kernel; the S slab loads of a thread are independent (batched 8 at a time) and
// added in slab order, so the result does not depend on the launch geometry.
__global__ void __launch_bounds__(256)
k_wgrad_reduce(const float* __restrict__ partial, int nsplit, int ntaps, int Cin, int Cout,
               int transpose, float* __restrict__ dW, unsigned long long dead_taps) {
    const long long per = (long long)ntaps * Cin * Cout;          // Cout % 4 == 0
    const long long per4 = per >> 2;
    const long long tap4 = ((long long)Cin * Cout) >> 2;
    for (long long i4 = blockIdx.x * 256LL + threadIdx.x; i4 < per4; i4 += (long long)gridDim.x * 256) {
        const float4* src = reinterpret_cast<const float4*>(partial) + i4;
        float4 s = make_float4(0, 0, 0, 0);
        int k = (dead_taps >> (i4 / tap4)) & 1 ? nsplit : 0;      // a tap no workgroup ran: its slabs were never written
        for (; k + 4 <= nsplit; k += 4) {               // (four in flight: <= 56 registers, see k_wgrad_reduce_lanes)
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(k + u) * per4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        for (; k < nsplit; ++k) {
            const float4 v = src[(size_t)k * per4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const long long i = i4 << 2;
        if (!transpose) {
            reinterpret_cast<float4*>(dW)[i4] = s;
        } else {
            const int n = (int)(i % Cout);
            long long t = i / Cout;
            const int c = (int)(t % Cin);
            const int tap = (int)(t / Cin);
            float* o = dW + ((size_t)tap * Cout + n) * Cin + c;
            o[0] = s.x; o[Cin] = s.y; o[2 * (size_t)Cin] = s.z; o[3 * (size_t)Cin] = s.w;
        }
    }
}

// Many slabs over a small kernel (the 64x64 Dense layers: > 1000 slabs of 16 KB): 32 lanes stride over the slabs of
// 8 float4 outputs per block (loads batched 8 deep), combined in lane order through LDS.
__global__ void __launch_bounds__(256, 8)            // <= 56 registers
k_wgrad_reduce_lanes(const float* __restrict__ partial, int nsplit, int ntaps, int Cin, int Cout,
                     int transpose, float* __restrict__ dW, unsigned long long dead_taps) {
    // One WAVE per 8 outputs (float4 each): lane = 8 * g + t sums slabs g, g + 8, g + 16, ... of output t (eight loads in
    // flight), then the eight partial sums of an output are added across lanes in a fixed tree -- no LDS and no barrier:
    // the pass runs beside data-gradient kernels that hold all but a few KB of every CU's LDS, and with 4 KB of LDS per
    // workgroup only one of its workgroups fitted a CU at a time.  Registers for the same reason: three waves of a
    // 148-register contraction leave 56 registers per SIMD lane; at 64 this kernel's waves only found room when a
    // data-gradient workgroup ENDED (171-226 us in the step for the 47 MB of a middle layer, 12 us alone).
    const long long per4 = ((long long)ntaps * Cin * Cout) >> 2;
    const long long tap4 = ((long long)Cin * Cout) >> 2;
    const int lane = threadIdx.x & 63, tx = lane & 7, ty = lane >> 3;
    const long long i4 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + tx;
    float4 s = make_float4(0, 0, 0, 0);
    const bool live = i4 < per4 && !((dead_taps >> ((i4 < per4 ? i4 : 0) / tap4)) & 1);
    if (live) {
        const float4* src = reinterpret_cast<const float4*>(partial) + i4;
        int k = ty;
        for (; k + 3 * 8 < nsplit; k += 4 * 8) {                // (four in flight, not eight: see the register note below)
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(k + 8 * u) * per4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        for (; k < nsplit; k += 8) {
            const float4 v = src[(size_t)k * per4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {                 // groups g and g + o/8: ((0+1)+(2+3))+((4+5)+(6+7))
        s.x += __shfl_down(s.x, o, 64); s.y += __shfl_down(s.y, o, 64);
        s.z += __shfl_down(s.z, o, 64); s.w += __shfl_down(s.w, o, 64);
    }
    if (ty != 0 || i4 >= per4) return;
    const long long i = i4 << 2;
    if (!transpose) {
        reinterpret_cast<float4*>(dW)[i4] = s;
    } else {
        const int n = (int)(i % Cout);
        long long t = i / Cout;
        const int c = (int)(t % Cin);
        const int tap = (int)(t / Cin);
        float* o = dW + ((size_t)tap * Cout + n) * Cin + c;
        o[0] = s.x; o[Cin] = s.y; o[2 * (size_t)Cin] = s.z; o[3 * (size_t)Cin] = s.w;
    }
}

// ---- host side: plan, bind, run ---------------------------------------------------------------------------------------
// plan_wgrad decides everything a weight-gradient call does before a tensor is known: the kernel (ring, then w-halo, then
// plain), its argument struct, the launch and the slab sum that follows it.  bind_wgrad puts the tensors and the
// workspace placement into that plan and run_wgrad issues it.  lisec_conv_wgrad, the batched entry, the workspace sizes
// and lisec_conv_wgrad_plan_query all read the same WgradCall, so a query reports the plan a call WILL run.
using PlainKernel = decltype(&k_wgrad<0, 1, false>);
using HaloKernel = decltype(&k_wgrad_halo<false, 7>);
using HaloBatchKernel = decltype(&k_wgrad_halo_batch<false, 7>);
using RingKernel = decltype(&k_wgrad_ring<false, 3>);
using RingBatchKernel = decltype(&k_wgrad_ring_batch<false, 3>);

struct WgradCall {
    enum Kind { RING, HALO, PLAIN } kind;        // the order they are tried in
    enum Reduce { NONE, RING_SUM, LANE_SUM, SLAB_SUM };
    // the kernel's argument, pointers still empty: RING takes `ring`, HALO takes `it`, PLAIN takes it.g, the operands and
    // the slab split of `it`, and dy_bn, one by one
    RingItem ring;
    WgradItem it;
    const float* dy_bn;
    bool xf;                     // the instantiation: BatchNormalization / ReLU on load, ...
    int np;                      // ... staging passes (ring: 48 rows; halo: 16 rows; plain: its 8 passes of 16 rows)
    bool mirrored;               // a unit-stride transposed gather run as the plain one with mirrored taps and pads
    union { RingKernel ring_fn; HaloKernel halo_fn; PlainKernel plain_fn; };
    dim3 grid, block;
    size_t lds;
    Reduce reduce;               // the launch that sums the slabs (NONE: the kernel combines in place)
    dim3 reduce_grid;
    unsigned long long dead_taps;    // taps whose groups got no workgroups: the slab sum writes zeros
    int cells;                   // arrival counters used
    size_t slab_bytes, ws_bytes; // workspace = [kWgradCounters arrival counters][slabs]
    // what lisec_conv_wgrad_plan_query reports beside the launches (slabs / tiles_per_slab: the split of the M tiles)
    int taps_per_group, groups, tile_rows, tiles, slabs, tiles_per_slab, lines_per_run;
};

// ---- the instantiations.  These selectors name every kernel the file compiles and no other.
RingKernel ring_kernel(bool xf, int np) {
    switch (np) {
    case 3: return xf ? k_wgrad_ring<true, 3> : k_wgrad_ring<false, 3>;
    case 5: return xf ? k_wgrad_ring<true, 5> : k_wgrad_ring<false, 5>;
    }
    return xf ? k_wgrad_ring<true, 6> : k_wgrad_ring<false, 6>;
}
RingBatchKernel ring_kernel_batch(bool xf, int np) {
    switch (np) {
    case 3: return xf ? k_wgrad_ring_batch<true, 3> : k_wgrad_ring_batch<false, 3>;
    case 5: return xf ? k_wgrad_ring_batch<true, 5> : k_wgrad_ring_batch<false, 5>;
    }
    return xf ? k_wgrad_ring_batch<true, 6> : k_wgrad_ring_batch<false, 6>;
}
HaloKernel halo_kernel(bool xf, int np) {
    if (np == 7) return xf ? k_wgrad_halo<true, 7> : k_wgrad_halo<false, 7>;
    return xf ? k_wgrad_halo<true, 9> : k_wgrad_halo<false, 9>;
}
HaloBatchKernel halo_kernel_batch(bool xf, int np) {
    if (np == 7) return xf ? k_wgrad_halo_batch<true, 7> : k_wgrad_halo_batch<false, 7>;
    return xf ? k_wgrad_halo_batch<true, 9> : k_wgrad_halo_batch<false, 9>;
}
template <int MODE, bool RL>
PlainKernel plain_kernel_tg(int TG) {
    switch (TG) {
    case 1: return k_wgrad<MODE, 1, RL>;
    case 2: return k_wgrad<MODE, 2, RL>;
    case 3: return k_wgrad<MODE, 3, RL>;
    }
    return k_wgrad<MODE, 4, RL>;
}
PlainKernel plain_kernel(int mode, int TG, bool rows) {
    if (mode == 0) return rows ? plain_kernel_tg<0, true>(TG) : plain_kernel_tg<0, false>(TG);
    return rows ? plain_kernel_tg<1, true>(TG) : plain_kernel_tg<1, false>(TG);
}

int ring_slots() { return tuning().wgrad_ring_slots > 0 ? tuning().wgrad_ring_slots : cu_count(); }   // one ring workgroup per CU

// 3 taps along w at stride 1 on a line long enough: the shape the w-halo kernel serves (tiles follow the output lines)
bool halo_shape(const ConvGeom& g) { return g.KW == 3 && g.ls_w == 0 && g.Wo >= 8; }

// LDS of a halo workgroup.  At LT = 100 that is 53 760 B = 42 of the CU's 128 granules of 1 280 B, and three fit -- which
// starves the data-gradient chain running beside the weight gradients on the other stream of its 41 granules (measured
// in the step: 227.7 samples/s with three per CU against 232 with two; alone the three-per-CU launch is 5 % faster).
// tuning().wgrad_per_cu == 2 (default) therefore asks for 43 granules: two of these + one chain workgroup = 127 of 128.
size_t halo_lds(int LT) {
    const int DR = (LT + 7) & ~7;
    size_t lds = (size_t)(2 * DR + 2) * BC * sizeof(float);
    // just over a third of 160 KB and not more: LDS is handed out in 1 280-byte granules, 2 x 43 granules leave 53 760 B --
    // room for the 52 224 B of a data-gradient workgroup; a request of 55 637 B (44 granules) left 51 200 and locked the
    // chain out of every CU that held two of these
    const size_t third = 54700;
    if (tuning().wgrad_per_cu == 2 && lds < third) lds = third;
    return lds;
}

// The ring kernel's plan of the forward gather `g` over every position; false when the kernel does not serve it.
// slots: workgroups the call should fill (0: one per CU)
bool plan_ring(const ConvGeom& g, int slots, WgradCall* p) {
    if (!tuning().wgrad_ring || g.KW != 3 || g.KH != 3 || g.ls_w != 0 || g.ls_h != 0 || g.Wo < 8 || g.ph < 0 || g.ph > 2 ||
        g.out_stride % 4 || g.Cout % 4)
        return false;
    RingItem& it = p->ring;
    it.g = RingGeom{g.Di, g.Hi, g.Wi, g.Do, g.Ho, g.Wo, g.KD, g.ls_d, g.pd, g.ph, g.pw, g.Cin, g.in_stride, g.Cout, g.out_stride};
    it.LT = cdiv(g.Wo, cdiv(g.Wo, BMW));        // equal tiles per line
    it.tpl = cdiv(g.Wo, it.LT);
    it.gy = cdiv(g.Cin, BC); it.gz = cdiv(g.Cout, BC);
    it.ncells = g.KD * it.gy * it.gz;
    it.npairs = 0;
    int planes[4] = {0, 0, 0, 0};
    for (int kd = 0; kd < g.KD; ++kd)
        for (int d = 0; d < g.Do; ++d) {
            const int sd = (d << g.ls_d) - g.pd + kd;
            if (sd < 0 || sd >= g.Di) continue;
            if (it.npairs >= 16) return false;
            it.pair_kd[it.npairs] = (unsigned char)kd; it.pair_d[it.npairs] = (unsigned char)d;
            it.pair_rank[it.npairs] = (unsigned char)planes[kd]++;
            ++it.npairs;
        }
    if (it.npairs == 0) return false;
    for (int i = it.npairs; i < 16; ++i) it.pair_kd[i] = it.pair_d[i] = it.pair_rank[i] = 0;
    // runs per column: one round of workgroups where possible, the longest runs that balance (a run pays two warm-up
    // lines and one slab: ~ one tile)
    const int cols = it.gy * it.gz * it.tpl * it.npairs;
    if (slots <= 0) slots = ring_slots();
    int best_r = 1;
    long long best_cost = -1;
    for (int r = 1; r <= g.Ho; ++r) {
        const long long rounds = cdiv((long long)cols * r, slots);
        const long long cost = rounds * (cdiv(g.Ho, r) + 1);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_r = r; }
    }
    it.R = best_r;
    it.nblocks = cols * it.R;
    int smax = 0;
    bool dead = false;
    for (int kd = 0; kd < 4; ++kd) {
        it.kd_slices[kd] = kd < g.KD ? planes[kd] * it.tpl * it.R : 0;
        if (it.kd_slices[kd] > smax) smax = it.kd_slices[kd];
        if (kd < g.KD && planes[kd] == 0) dead = true;
    }
    it.combine = (!dead && smax <= tuning().wgrad_combine_max && it.ncells <= kWgradCounters) ? 1 : 0;
    p->slab_bytes = align_up((size_t)smax * it.ncells * kRSlabF4 * 16, 256);
    if (p->slab_bytes >= (1ull << 31)) return false;
    if ((long long)g.Do * g.Ho * g.Wo * g.out_stride >= (1LL << 31)) return false;   // int32 offsets into dy
    p->ws_bytes = sizeof(int) * kWgradCounters + p->slab_bytes;
    p->cells = it.ncells;
    const int DR = (it.LT + 7) & ~7;
    p->np = 2 * (DR + 2) <= 3 * 48 ? 3 : (2 * (DR + 2) <= 5 * 48 ? 5 : 6);   // 48-row passes over [x line][x line | dY line]
    p->ring_fn = ring_kernel(p->xf, p->np);
    p->grid = dim3(it.nblocks); p->block = dim3(kRingThreads);
    p->lds = (size_t)(3 * (DR + 2) + DR + 2) * BC * sizeof(float);           // x ring, dY tile, scale/shift
    p->reduce = it.combine ? WgradCall::NONE : WgradCall::RING_SUM;
    p->reduce_grid = dim3(cdiv((long long)it.ncells * kRSlabF4, 32));
    p->taps_per_group = 9;
    p->groups = it.npairs;                      // (kd, d) pairs that read an existing plane
    p->tile_rows = it.LT;
    p->tiles = g.Do * g.Ho * it.tpl;
    p->slabs = smax;
    p->tiles_per_slab = p->lines_per_run = cdiv(g.Ho, it.R);
    return true;
}

// The slab plan of the w-halo (`halo`) and plain kernels: tap groups, M tiles, the ranges of tiles that get a slab each,
// the workspace.  blocks_target: workgroups the call should fill (0: tuning().wgrad_blocks)
void plan_tiles(const ConvGeom& g, bool halo, int blocks_target, WgradCall* p) {
    WgradItem& it = p->it;
    it.g = g;
    it.gy = cdiv(g.Cin, BC); it.gz = cdiv(g.Cout, BC);
    p->taps_per_group = g.KW;                   // the (at most 4) taps of one (kd, kh) share a staged dY tile
    p->groups = g.KD * g.KH;
    p->tile_rows = BMW;
    p->tiles = cdiv(g.M, BMW);
    it.live.n = 0;
    if (halo) {
        it.LT = p->tile_rows = cdiv(g.Wo, cdiv(g.Wo, BMW));     // equal tiles per line
        p->tiles = g.Do * g.Ho * cdiv(g.Wo, it.LT);
        for (int kd = 0; kd < g.KD; ++kd) {
            bool dlive = false;
            for (int d = 0; d < g.Do && !dlive; ++d) { const int sd = (d << g.ls_d) - g.pd + kd; dlive = sd >= 0 && sd < g.Di; }
            for (int kh = 0; kh < g.KH; ++kh) {
                bool hlive = false;
                for (int h = 0; h < g.Ho && !hlive; ++h) { const int sh = (h << g.ls_h) - g.ph + kh; hlive = sh >= 0 && sh < g.Hi; }
                if (dlive && hlive && it.live.n < 16) it.live.id[it.live.n++] = (unsigned char)(kd * g.KH + kh);
            }
        }
        p->groups = it.live.n > 0 ? it.live.n : 1;
    }
    const int target = blocks_target > 0 ? blocks_target : tuning().wgrad_blocks;
    int want = cdiv(target, p->groups * it.gy * it.gz);     // 1024: ~2 rounds of the 512 resident workgroups (measured: 512-1024
                                                // blocks beat 1536+, whose extra slabs cost more in the reduce than they balance)
    if (want < 1) want = 1;
    if (want > p->tiles) want = p->tiles;
    p->tiles_per_slab = cdiv(p->tiles, want);
    p->slabs = cdiv(p->tiles, p->tiles_per_slab);
    // every plan keeps the head of the workspace (kWgradCounters arrival counters) free, so that the counters of the
    // combining plans stay zero whatever else shares the workspace; slab_bytes = what follows the head
    p->slab_bytes = align_up(sizeof(float) * (size_t)p->slabs * g.KD * g.KH * g.KW * g.Cin * g.Cout, 256);
    it.combine = 0;
    if (halo && p->slabs <= tuning().wgrad_combine_max && g.KD * g.KH <= 16 &&
        (long long)g.KD * g.KH * it.gy * it.gz <= kWgradCounters) {
        // few slices per cell: combined inside the kernel (every group gets workgroups: the cells of a group that reads
        // nothing must still be written, as zeros)
        it.combine = 1;
        it.live.n = g.KD * g.KH;
        for (int i = 0; i < it.live.n; ++i) it.live.id[i] = (unsigned char)i;
        p->groups = it.live.n;
        p->slab_bytes = align_up((size_t)p->slabs * p->groups * it.gy * it.gz * kWSlabF4 * 16, 256);
    }
    p->ws_bytes = sizeof(int) * kWgradCounters + p->slab_bytes;
    it.nsplit = p->slabs; it.tiles_per_split = p->tiles_per_slab;
    it.gx = p->slabs * p->groups;
}

// Plans the weight gradient of `c` from what a plan depends on and nothing else.  share: the part of the chip the call
// should fill -- workgroups of the halo and plain kernels, slots of the ring; 0: the whole chip.  first: where the order
// ring, w-halo, plain is entered (the batched entry asks for a launch of halo items after one of ring items failed).
int plan_wgrad(const lisec_conv_geom* c, int flags, bool has_in_bn, bool has_dy_bn, bool has_rows, int row_capacity,
               int share, WgradCall::Kind first, WgradCall* p) {
    *p = WgradCall{};
    ConvGeom g;
    if (int rc = conv_geom_check(c, &g)) return rc;
    LISEC_CHECK_ARG(!has_rows || row_capacity > 0, "row list needs a capacity");
    if (has_rows) { g.M = row_capacity; g.pointwise = 0; }
    p->xf = has_in_bn || (flags & LISEC_CONV_IN_RELU);
    // The ring and w-halo kernels gather forwards, over every position, with dy as it is.  A transposed gather with unit
    // strides is the forward one with mirrored taps and pads K-1-p (first deconv: kernel 3, stride 1, 'same'), so they
    // serve it too; the plain kernel gathers either way and gets the geometry as given.
    const bool dense = !has_rows && !has_dy_bn && !(flags & LISEC_CONV_DY_RELU);
    const bool flip = dense && c->mode == 1 && g.ls_d == 0 && g.ls_h == 0 && g.ls_w == 0 && g.KW == 3;
    const bool forward = dense && (c->mode == 0 || flip);
    ConvGeom m = g;
    if (flip) { m.pd = g.KD - 1 - g.pd; m.ph = g.KH - 1 - g.ph; m.pw = g.KW - 1 - g.pw; }
    if (forward && first == WgradCall::RING && plan_ring(m, share, p)) {
        p->kind = WgradCall::RING;
        p->ring.flags = flags; p->ring.flip = flip ? 1 : 0;
        p->mirrored = flip;
        return LISEC_OK;
    }
    const bool halo = forward && halo_shape(g);
    plan_tiles(halo ? m : g, halo, share, p);
    WgradItem& it = p->it;
    it.flags = flags;
    p->grid = dim3(it.gx, it.gy, it.gz); p->block = dim3(kThreads);
    if (halo) {
        p->kind = WgradCall::HALO;
        it.flip = flip ? 1 : 0;
        p->mirrored = flip;
        const int DR = (it.LT + 7) & ~7;
        p->np = DR + 2 <= 7 * 16 ? 7 : 9;                // the passes stage every row of the A image the chunks read
        p->halo_fn = halo_kernel(p->xf, p->np);
        p->lds = halo_lds(it.LT);
        p->cells = p->groups * it.gy * it.gz;
        unsigned ran = 0;
        for (int i = 0; i < it.live.n; ++i) ran |= 1u << it.live.id[i];
        for (int gi = 0; gi < g.KD * g.KH; ++gi) {
            if ((ran >> gi) & 1) continue;
            const int kd = gi / g.KH, kh = gi - kd * g.KH;
            for (int tt = 0; tt < 3; ++tt) {
                const int tap = flip ? ((g.KD - 1 - kd) * g.KH + (g.KH - 1 - kh)) * g.KW + (2 - tt) : gi * g.KW + tt;
                p->dead_taps |= 1ULL << tap;
            }
        }
    } else {
        p->kind = WgradCall::PLAIN;
        p->np = 8;
        p->plain_fn = plain_kernel(c->mode, p->taps_per_group, has_rows);
        p->lds = 2 * TILE_FLOATS * sizeof(float);
    }
    // many slabs: 32 lane groups per output sum slabs / 32 slabs each (one or two memory round trips instead of
    // slabs / 8 dependent ones -- the pass runs beside the data-gradient chain and every round trip costs microseconds
    // there: 22-151 us in the step for the 47 MB of a middle layer, 12 us alone)
    const long long per4 = (long long)g.KD * g.KH * g.KW * g.Cin * g.Cout / 4;
    int gb = cdiv(per4, 256);
    if (gb > 4096) gb = 4096;
    p->reduce = it.combine ? WgradCall::NONE : p->slabs >= 32 ? WgradCall::LANE_SUM : WgradCall::SLAB_SUM;
    p->reduce_grid = p->reduce == WgradCall::LANE_SUM ? dim3(cdiv(per4, 32)) : dim3(gb);
    return LISEC_OK;
}

// Puts the tensors and the workspace placement into a planned call.
// workspace = [kWgradCounters arrival counters][slabs]; counter0: first counter of this call, slab_off: bytes into the slabs
void bind_wgrad(WgradCall* p, const float* in, const float* in_bn, const float* dy, const float* dy_bn, int transpose_out,
                float* dW, const int32_t* row_coords, const int32_t* row_count, void* workspace, int counter0, size_t slab_off) {
    int* counters = static_cast<int*>(workspace) + counter0;
    float* slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + sizeof(int) * kWgradCounters + slab_off);
    if (p->kind == WgradCall::RING) {
        RingItem& it = p->ring;
        it.in = in; it.in_bn = in_bn; it.dy = dy; it.dW = dW; it.transpose = transpose_out;
        it.counters = counters; it.slabs = slabs;
    } else {
        WgradItem& it = p->it;
        it.in = in; it.in_bn = in_bn; it.dy = dy; it.dW = dW; it.transpose = transpose_out;
        it.counters = counters; it.partial = slabs;
        it.g.row_coords = row_coords; it.g.row_count = row_count;
        p->dy_bn = dy_bn;
    }
}

int run_reduce(const WgradCall& p, hipStream_t st) {
    const WgradItem& it = p.it;
    switch (p.reduce) {
    case WgradCall::NONE: return LISEC_OK;
    case WgradCall::RING_SUM: LISEC_LAUNCH(k_wgrad_ring_reduce, p.reduce_grid, dim3(256), 0, st, p.ring); break;
    case WgradCall::LANE_SUM:
    case WgradCall::SLAB_SUM:
        LISEC_LAUNCH(p.reduce == WgradCall::LANE_SUM ? k_wgrad_reduce_lanes : k_wgrad_reduce, p.reduce_grid, dim3(256), 0, st,
                     it.partial, it.nsplit, it.g.KD * it.g.KH * it.g.KW, it.g.Cin, it.g.Cout, it.transpose, it.dW, p.dead_taps);
        break;
    }
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

// Issues a bound call: the main launch, then its slab sum.
int run_wgrad(const WgradCall& p, hipStream_t st) {
    const WgradItem& it = p.it;
    switch (p.kind) {
    case WgradCall::RING: LISEC_LAUNCH(p.ring_fn, p.grid, p.block, p.lds, st, p.ring); break;
    case WgradCall::HALO: LISEC_LAUNCH(p.halo_fn, p.grid, p.block, p.lds, st, it); break;
    case WgradCall::PLAIN:
        LISEC_LAUNCH(p.plain_fn, p.grid, p.block, p.lds, st, it.g, it.in, it.in_bn, it.flags, it.dy, p.dy_bn, it.nsplit,
                     it.tiles_per_split, it.partial);
        break;
    }
    LISEC_LAUNCH_CHECK();
    return run_reduce(p, st);
}

// Several weight gradients in one launch (see k_wgrad_halo_batch): every item must take the same kernel -- `kind`, ring or
// w-halo -- with the same staging variant, as the stride-1 3x3 convolutions of one RPN block do.  The chip is shared in
// proportion to the items' work: pass one plans every item at full share for its work, pass two re-plans it with its part.
// Returns 0 and the planned calls when the items share a launch; 1 when they do not; < 0 on error.
int plan_batch(const lisec_wgrad_item* items, int n, WgradCall::Kind kind, WgradCall* calls, size_t* total) {
    const bool ring = kind == WgradCall::RING;
    long long work[kBatchMax], all = 0;
    size_t off = 0;
    int cells = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n; ++i) {
            int share = 0;
            if (pass == 1) {
                share = ring ? (int)((double)ring_slots() * (double)work[i] / (double)all)
                             : (int)((double)tuning().wgrad_batch_blocks * (double)work[i] / (double)all + 0.5);
                if (share < 1) share = 1;
            }
            WgradCall& p = calls[i];
            if (int rc = plan_wgrad(items[i].g, items[i].flags, items[i].in_bnstate != nullptr, false, false, 0, share, kind, &p))
                return rc;
            if (p.kind != kind) return 1;
            if (pass == 0) {
                const RingItem& r = p.ring;
                const ConvGeom& g = p.it.g;
                work[i] = ring ? (long long)r.gy * r.gz * r.tpl * r.npairs * r.g.Ho * (r.LT + 8)
                               : (long long)g.Do * g.Ho * g.Wo * g.KD * g.KH * cdiv(g.Cin, BC) * cdiv(g.Cout, BC);
                all += work[i];
            } else {
                if (p.xf != calls[0].xf || p.np != calls[0].np) return 1;
                off += p.slab_bytes;
                cells += p.cells;
            }
        }
    if (cells > kWgradCounters || (ring && off >= (1ull << 31))) return 1;
    *total = sizeof(int) * kWgradCounters + off;
    return 0;
}

// Binds the planned calls of a batch one behind the other in the workspace and issues them: one launch of `kernel` over
// the items' grids, then the slab sums of the items that do not combine in place.
template <typename Batch, typename Item>
int run_batch(void (*kernel)(Batch), Item WgradCall::*item, WgradCall* calls, const lisec_wgrad_item* items, int n,
              void* workspace, hipStream_t st) {
    Batch b;
    b.n = n;
    size_t lds = 0, off = 0;
    int blocks = 0, cells = 0;
    for (int i = 0; i < n; ++i) {
        LISEC_CHECK_ARG(items[i].in && items[i].dy && items[i].dW && ((uintptr_t)items[i].in & 15) == 0 &&
                        ((uintptr_t)items[i].dy & 15) == 0, "item %d: NULL or unaligned tensor", i);
        WgradCall& p = calls[i];
        bind_wgrad(&p, items[i].in, items[i].in_bnstate, items[i].dy, nullptr, items[i].transpose_out, items[i].dW, nullptr,
                   nullptr, workspace, cells, off);
        cells += p.cells;
        off += p.slab_bytes;
        b.first[i] = blocks;
        b.item[i] = p.*item;
        blocks += (int)(p.grid.x * p.grid.y * p.grid.z);
        lds = p.lds > lds ? p.lds : lds;
    }
    b.first[n] = blocks;
    LISEC_LAUNCH(kernel, dim3(blocks), calls[0].block, lds, st, b);
    LISEC_LAUNCH_CHECK();
    for (int i = 0; i < n; ++i)
        if (int rc = run_reduce(calls[i], st)) return rc;
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_conv_wgrad_workspace_bytes(const lisec_conv_geom* c, int row_capacity) {
    // The caller sizes its workspace before it knows the flags, so this is the largest plan the geometry can get at this
    // M: the slab plan without and with the w-halo kernel (as given, dy transformed, mirrored), and the ring without a row list
    ConvGeom g;
    if (conv_geom_check(c, &g)) return 0;
    if (row_capacity > 0) g.M = row_capacity;
    WgradCall p;
    plan_tiles(g, false, 0, &p);
    size_t w = p.ws_bytes;
    if (halo_shape(g)) {
        plan_tiles(g, true, 0, &p);
        w = p.ws_bytes > w ? p.ws_bytes : w;
    }
    if (row_capacity <= 0 && plan_wgrad(c, 0, false, false, false, 0, 0, WgradCall::RING, &p) == 0 && p.kind == WgradCall::RING &&
        p.ws_bytes > w)
        w = p.ws_bytes;
    return w;
}

extern "C" int lisec_conv_wgrad_plan_query(const lisec_conv_geom* c, int flags, int has_dy_bnstate, int has_row_list,
                                           int row_capacity, lisec_wgrad_plan* out) {
    LISEC_CHECK_ARG(out, "NULL plan");
    WgradCall p;                                // (no reported field depends on the on-load transform of `in`)
    if (int rc = plan_wgrad(c, flags, false, has_dy_bnstate != 0, has_row_list != 0, row_capacity, 0, WgradCall::RING, &p))
        return rc;
    out->ring = p.kind == WgradCall::RING ? 1 : 0;
    out->halo = p.kind == WgradCall::HALO ? 1 : 0;
    out->mirrored = p.mirrored ? 1 : 0;
    out->taps_per_group = p.taps_per_group;
    out->groups = p.groups;
    out->tile_rows = p.tile_rows;
    out->staging_passes = p.np;
    out->tiles = p.tiles;
    out->slabs = p.slabs;
    out->tiles_per_slab = p.tiles_per_slab;
    out->workgroups = (int)(p.grid.x * p.grid.y * p.grid.z);
    out->lane_reduce = (p.reduce == WgradCall::RING_SUM || p.reduce == WgradCall::LANE_SUM) ? 1 : 0;
    out->combine_in_kernel = p.reduce == WgradCall::NONE ? 1 : 0;
    out->runs_per_column = p.kind == WgradCall::RING ? p.ring.R : 0;
    out->lines_per_run = p.lines_per_run;
    return LISEC_OK;
}

extern "C" int lisec_conv_wgrad(const lisec_conv_geom* c, const float* in, const float* in_bnstate, int flags,
                                const float* dy, const float* dy_bnstate, void* workspace,
                                size_t workspace_bytes, int transpose_out, float* dW, const int32_t* row_coords,
                                const int32_t* row_count, int row_capacity, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(in && dy && workspace && dW, "NULL pointer");
    LISEC_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)dy & 15) == 0, "in/dy must be 16-byte aligned");
    LISEC_CHECK_ARG(!row_coords || (row_count && row_capacity > 0), "row list needs a device count and a capacity");
    WgradCall p;
    if (int rc = plan_wgrad(c, flags, in_bnstate != nullptr, dy_bnstate != nullptr, row_coords != nullptr, row_capacity, 0,
                            WgradCall::RING, &p))
        return rc;
    LISEC_CHECK_ARG(c->out_stride % 4 == 0 && c->Cout % 4 == 0, "dY channels/stride must be multiples of 4");
    if (workspace_bytes < p.ws_bytes) {
        set_error("wgrad workspace too small: %zu < %zu", workspace_bytes, p.ws_bytes);
        return LISEC_ENOSPC;
    }
    bind_wgrad(&p, in, in_bnstate, dy, dy_bnstate, transpose_out, dW, row_coords, row_count, workspace, 0, 0);
    return run_wgrad(p, static_cast<hipStream_t>(stream_));
}

// Several weight gradients in one launch: of the ring kernel if every item takes it, else of the w-halo kernel if every
// item takes that; otherwise the items run one after the other.
extern "C" size_t lisec_conv_wgrad_batched_workspace_bytes(const lisec_wgrad_item* items, int n) {
    if (!items || n < 1 || n > kBatchMax) return 0;
    WgradCall calls[kBatchMax];
    size_t total = 0;
    if (plan_batch(items, n, WgradCall::RING, calls, &total) == 0 || plan_batch(items, n, WgradCall::HALO, calls, &total) == 0)
        return total;
    size_t worst = 0;                               // not batchable: the items run one by one in the same workspace
    for (int i = 0; i < n; ++i) {
        const size_t w = lisec_conv_wgrad_workspace_bytes(items[i].g, 0);
        worst = w > worst ? w : worst;
    }
    return worst;
}

extern "C" int lisec_conv_wgrad_batched(const lisec_wgrad_item* items, int n, void* workspace, size_t workspace_bytes,
                                        lisec_stream_t stream_) {
    LISEC_CHECK_ARG(items && n >= 1 && n <= kBatchMax && workspace, "1 .. 6 items and a workspace");
    hipStream_t st = static_cast<hipStream_t>(stream_);
    WgradCall calls[kBatchMax];
    size_t total = 0;
    int kind = plan_batch(items, n, WgradCall::RING, calls, &total);
    if (kind == 1) kind = plan_batch(items, n, WgradCall::HALO, calls, &total);
    if (kind < 0) return kind;
    if (kind != 0) {                                // one by one (same stream: they may share the workspace)
        for (int i = 0; i < n; ++i)
            if (int rc = lisec_conv_wgrad(items[i].g, items[i].in, items[i].in_bnstate, items[i].flags, items[i].dy, nullptr,
                                          workspace, workspace_bytes, items[i].transpose_out, items[i].dW, nullptr, nullptr, 0,
                                          stream_))
                return rc;
        return LISEC_OK;
    }
    if (workspace_bytes < total) {
        set_error("batched wgrad workspace too small: %zu < %zu", workspace_bytes, total);
        return LISEC_ENOSPC;
    }
    const WgradCall& p0 = calls[0];
    if (p0.kind == WgradCall::RING)
        return run_batch<RingBatch>(ring_kernel_batch(p0.xf, p0.np), &WgradCall::ring, calls, items, n, workspace, st);
    return run_batch<WgradBatch>(halo_kernel_batch(p0.xf, p0.np), &WgradCall::it, calls, items, n, workspace, st);
}

// Diagnostic: points the weight-gradient kernels' stamp buffer at `buf` (device, 8192*8 uint64) or NULL.
extern "C" int lisec_debug_wgrad_stamps(unsigned long long* buf) {
    LISEC_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_wgrad_stamps), &buf, sizeof(buf)));
    return LISEC_OK;
}
