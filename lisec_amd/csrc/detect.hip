// Many-box detection output (gfx950; include/lisec_hip.h section 5b): score cut, exact top-N, greedy rotated NMS over those N.
//
//   k_detect_key      one thread per candidate: the filters, then the 64-bit key (ordered score bits << 32 | flat index), 0 = out
//   k_detect_select   one workgroup: radix selection of the N-th largest key (8-bit digits, integer LDS histograms), which moves
//                  into LDS once the bin of the cut is small, a bitonic sort of the winners by descending key, and the decode
//                  of the ranked list
//   k_detect_mask     one workgroup per 64 x 64 tile of the upper triangle of the suppression matrix, both box sets staged in
//                  LDS: a lane per row lists the pairs whose footprints can touch (centre distance against the circumradii),
//                  then every thread clips one listed pair at a time (pair_iou of box_geom.h, float64) and ORs its bit in
//   k_detect_greedy   one wave64: lane l holds word l of the removed set, rows of the matrix are loaded a group ahead; the kept
//                  ranks are listed in LDS and written out by all lanes at the end
// Everything is an integer or a float64 value computed in a fixed order; the LDS atomics are integer additions and ORs, whose
// result does not depend on the arrival order.  Integer/latency-bound work: no MFMA.
#include "common.h"
#include "box_geom.h"

namespace lisec {
namespace {

using u64 = unsigned long long;

constexpr int kTopN = LISEC_DETECT_MAX_TOP_N;
constexpr int kSelThreads = 1024;
constexpr int kDigitBits = 8;
constexpr int kChunk = 8;                                     // keys a selection thread loads before it bins them
constexpr int kBin = 2048;                                    // keys of one radix bin that finish the selection in LDS
constexpr int kMaskWaves = 4;                                 // waves of a mask workgroup
constexpr int kAhead = 8;                                     // mask rows the greedy reduce loads ahead of the one it decides

// unsigned order of the result = numeric order of the float (-0.0 below +0.0); never 0 for a number
__device__ __forceinline__ unsigned ordered_bits(float s) {
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// the value lane `src` holds, src the same in every lane: two v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ unsigned lane_value(unsigned v, int src) {
    return (unsigned)__builtin_amdgcn_readlane((int)v, src);
}
__device__ __forceinline__ u64 lane_value(u64 v, int src) {
    return ((u64)lane_value((unsigned)(v >> 32), src) << 32) | lane_value((unsigned)v, src);
}

__global__ void k_detect_key(const float* __restrict__ cls, int cls_stride, const float* __restrict__ reg, int reg_stride,
                          lisec_rpn_cfg cfg, double score_threshold, int inside_only, u64* __restrict__ keys) {
    const int M = cfg.outX * cfg.outY;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * M) return;
    const int a = i / M, m = i - a * M;
    const float s = cls[(size_t)m * cls_stride + a];
    u64 key = 0;
    if (!isnan(s) && (double)s > score_threshold) {
        double b[7];
        rpn_decode_box(cfg, reg, reg_stride, i, b);
        bool ok = finite7(b) && b[3] > 0 && b[4] > 0 && b[5] > 0;
        if (inside_only) ok = ok && b[0] >= 0 && b[0] <= cfg.outX * cfg.vx && b[1] >= 0 && b[1] <= cfg.outY * cfg.vy;
        if (ok) key = ((u64)ordered_bits(s) << 32) | (unsigned)i;
    }
    keys[i] = key;
}

// hist[d] += 1 for every lane with `valid`.  The leading digits of the keys (sign and exponent of the score) fall into a
// handful of bins: the two most common digits of the wave are added once each, by one lane, before the rest go one by one.
// Called by whole waves.
__device__ __forceinline__ void hist_add(unsigned* hist, bool valid, unsigned d) {
    u64 todo = __ballot(valid);
    for (int r = 0; r < 2 && todo; ++r) {
        const int lead = __ffsll(todo) - 1;
        const unsigned d0 = lane_value(d, lead);
        const u64 same = __ballot(valid && d == d0) & todo;
        if (lane_id() == lead) atomicAdd(&hist[d0], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane_id()) & 1) atomicAdd(&hist[d], 1u);
}

// keys[n] -> the min(top_n, passing) largest, ranked, decoded into rows 0 .. npad-1 (dead past the live ones).
// state = {live ranks, passing candidates}.  The selection reads the keys from memory until the bin of the cut holds at most
// kBin of them (with a score threshold that is after the first pass, without one after two or three); then the keys above
// that bin go to LDS as winners, the bin's keys beside them, and the remaining digits are decided there.
__global__ void __launch_bounds__(kSelThreads)
k_detect_select(const u64* __restrict__ keys, int n, int idx_bits, int top_n, int npad, const float* __restrict__ reg,
             int reg_stride, lisec_rpn_cfg cfg, int sigmoid_scores, double* __restrict__ boxes, double* __restrict__ scores,
             int* __restrict__ index, int* __restrict__ state) {
    __shared__ u64 s_key[kTopN], s_bin[kBin];
    __shared__ unsigned s_hist[1 << kDigitBits];
    __shared__ u64 s_prefix;
    __shared__ int s_remaining, s_want, s_passing, s_fill, s_bin_count, s_bin_fill;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = 0; s_remaining = 0; s_want = 0; s_passing = 0; s_fill = 0; s_bin_count = 0; s_bin_fill = 0; }
    for (int r = tid; r < kTopN; r += kSelThreads) s_key[r] = 0;          // dead keys pad the list for the sort

    // ---- the want-th largest key, digit by digit from the top; bits [idx_bits, 32) are 0 in every key ----
    bool first = true, in_lds = false;
    int m = 0;                                                 // keys in s_bin once in_lds
    for (int hi = 64; hi > 0;) {
        if (hi == 32) hi = idx_bits;
        if (hi == 0) break;
        const int lo = max(hi - kDigitBits, hi > 32 ? 32 : 0);
        const unsigned digit_mask = (1u << (hi - lo)) - 1u;
        if (tid < (1 << kDigitBits)) s_hist[tid] = 0;
        __syncthreads();
        const u64 prefix = s_prefix;
        if (!in_lds) {
            for (int base = 0; base < n; base += kSelThreads * kChunk) {   // a chunk of loads in flight, then its histogram
                u64 k[kChunk];
#pragma unroll
                for (int q = 0; q < kChunk; ++q) {
                    const int j = base + q * kSelThreads + tid;
                    k[q] = j < n ? keys[j] : 0;
                }
#pragma unroll
                for (int q = 0; q < kChunk; ++q) {
                    const bool in = k[q] != 0 && (hi == 64 || (k[q] >> hi) == (prefix >> hi));
                    hist_add(s_hist, in, (unsigned)(k[q] >> lo) & digit_mask);
                }
            }
        } else {
            for (int base = 0; base < m; base += kSelThreads) {
                const int j = base + tid;
                const u64 k = j < m ? s_bin[j] : 0;
                hist_add(s_hist, k != 0 && (k >> hi) == (prefix >> hi), (unsigned)(k >> lo) & digit_mask);
            }
        }
        __syncthreads();
        if (tid < kWave) {                                     // lane l owns the four digits 255 - 4l .. 252 - 4l, largest first
            unsigned c[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = s_hist[255 - 4 * tid - q]; sum += c[q]; }
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const unsigned up = __shfl_up(incl, o, 64);
                if (tid >= o) incl += up;
            }
            unsigned remaining = (unsigned)s_remaining;
            if (first) {                                       // the first histogram holds every passing candidate
                const int passing = (int)__shfl(incl, kWave - 1, 64);
                remaining = (unsigned)min(top_n, passing);
                if (tid == 0) { s_passing = passing; s_want = (int)remaining; }
            }
            unsigned above = incl - sum;                       // keys of this prefix with a larger digit than this lane's
            if (above < remaining && remaining <= incl) {      // exactly one lane (none when nothing passed)
                int q = 0;
                while (above + c[q] < remaining) { above += c[q]; ++q; }
                s_prefix = prefix | ((u64)(255 - 4 * tid - q) << lo);
                s_remaining = (int)(remaining - above);
                s_bin_count = (int)c[q];
            }
        }
        __syncthreads();
        if (s_want == 0) break;
        first = false;
        if (!in_lds && s_bin_count <= kBin) {                  // the last pass leaves one key in the bin: this is reached
            const u64 cut = s_prefix >> lo;
            for (int base = 0; base < n; base += kSelThreads * kChunk) {
                u64 k[kChunk];
#pragma unroll
                for (int q = 0; q < kChunk; ++q) {
                    const int j = base + q * kSelThreads + tid;
                    k[q] = j < n ? keys[j] : 0;
                }
#pragma unroll
                for (int q = 0; q < kChunk; ++q) {
                    if (k[q] == 0) continue;
                    if ((k[q] >> lo) > cut) {                  // above the bin of the cut: a winner whatever follows
                        const int slot = atomicAdd(&s_fill, 1);
                        if (slot < kTopN) s_key[slot] = k[q];
                    } else if ((k[q] >> lo) == cut) {
                        const int slot = atomicAdd(&s_bin_fill, 1);
                        if (slot < kBin) s_bin[slot] = k[q];
                    }
                }
            }
            __syncthreads();
            in_lds = true;
            m = s_bin_count;
        }
        hi = lo;
    }
    const int want = s_want, passing = s_passing;

    // ---- the winners inside the bin join the others (in any order: the sort follows) ----
    if (want > 0) {
        const u64 cut = s_prefix;
        for (int j = tid; j < m; j += kSelThreads) {
            const u64 k = s_bin[j];
            if (k >= cut) {
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < kTopN) s_key[slot] = k;
            }
        }
    }
    __syncthreads();
    int P = kWave;
    while (P < want) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += kSelThreads) {
                const int lo_i = 2 * t - (t & (j - 1)), hi_i = lo_i + j;
                const bool descending = (lo_i & k) == 0;
                const u64 x = s_key[lo_i], y = s_key[hi_i];
                if ((x < y) == descending) { s_key[lo_i] = y; s_key[hi_i] = x; }
            }
            __syncthreads();
        }
    }

    // ---- the ranked list, decoded ----
    for (int r = tid; r < npad; r += kSelThreads) {
        const u64 k = r < want ? s_key[r] : 0;
        double b[7] = {0, 0, 0, 0, 0, 0, 0}, sc = 0.0;
        int idx = -1;
        if (k != 0) {
            idx = (int)(unsigned)k;
            rpn_decode_box(cfg, reg, reg_stride, idx, b);
            sc = (double)from_ordered((unsigned)(k >> 32));
            if (sigmoid_scores) sc = 1.0 / (1.0 + exp(-sc));
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) boxes[(size_t)r * 7 + c] = b[c];
        scores[r] = sc;
        index[r] = idx;
    }
    if (tid == 0) { state[0] = want; state[1] = passing; }
}

// mask[i * T + w], bit b: rank j = 64 w + b with i < j < live and pair_iou(box_i, box_j) > thresh.  Workgroup t is tile
// (ti, tj), tj >= ti, of the upper triangle in row-major order; tiles past the live ranks write nothing (and are not read).
// A lane that clips while its 63 neighbours wait is what a row-per-lane sweep of the columns comes to (in a scene spread over
// the grid under 1 % of the pairs are near), hence the list: the clips are dealt to the threads one pair each.
__global__ void __launch_bounds__(kMaskWaves * kWave)
k_detect_mask(const double* __restrict__ boxes, const int* __restrict__ state, int T, double thresh, int mode,
           u64* __restrict__ mask) {
    __shared__ double s_row[kWave * 7], s_col[kWave * 7], s_row_diag[kWave], s_col_diag[kWave];
    __shared__ u64 s_word[kWave];
    __shared__ unsigned short s_pair[kWave * kWave];
    __shared__ int s_pairs;
    constexpr int kThreads = kMaskWaves * kWave;
    const int live = state[0];
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) { rem -= T - ti; ++ti; }
    const int tj = ti + rem;
    if (tj * kWave >= live) return;                            // tj >= ti: the row tile is live whenever the column tile is
    const int tid = threadIdx.x;
    for (int e = tid; e < kWave * 7; e += kThreads) {
        s_row[e] = boxes[(size_t)ti * kWave * 7 + e];
        s_col[e] = boxes[(size_t)tj * kWave * 7 + e];
    }
    if (tid < kWave) s_word[tid] = 0;
    if (tid == 0) s_pairs = 0;
    __syncthreads();
    if (tid < kWave) s_row_diag[tid] = hypot(s_row[tid * 7 + 3], s_row[tid * 7 + 4]);
    else if (tid < 2 * kWave) s_col_diag[tid - kWave] = hypot(s_col[(tid - kWave) * 7 + 3], s_col[(tid - kWave) * 7 + 4]);
    __syncthreads();

    // ---- the pairs whose footprints can touch, by pair_iou's own test (centres within the sum of the circumradii): every
    //      other pair has IoU exactly 0 there and sets no bit.  The list order is arbitrary; what it decides is not. ----
    const int lane = lane_id(), wv = tid >> 6;
    const int i = ti * kWave + lane;
    for (int c = wv; c < kWave; c += kMaskWaves) {
        const int j = tj * kWave + c;
        bool near = i < live && j > i && j < live;
        if (near) {
            const double dx = s_row[lane * 7] - s_col[c * 7], dy = s_row[lane * 7 + 1] - s_col[c * 7 + 1];
            const double r = 0.5 * (s_row_diag[lane] + s_col_diag[c]);
            near = !(dx * dx + dy * dy > r * r * 1.0000001);
        }
        const u64 hits = __ballot(near);
        if (hits == 0) continue;
        int at = 0;
        if (lane == 0) at = atomicAdd(&s_pairs, __popcll(hits));
        at = __shfl(at, 0, 64) + __popcll(hits & ((1ull << lane) - 1ull));
        if (near) s_pair[at] = (unsigned short)(lane * kWave + c);
    }
    __syncthreads();

    // ---- one listed pair per thread: the clip, in float64 ----
    const int pairs = s_pairs;
    for (int p = tid; p < pairs; p += kThreads) {
        const int r = s_pair[p] / kWave, c = s_pair[p] % kWave;
        double rb[7], cb[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { rb[q] = s_row[r * 7 + q]; cb[q] = s_col[c * 7 + q]; }
        if (pair_iou(rb, cb, mode) > thresh) atomicOr(&s_word[r], 1ull << c);
    }
    __syncthreads();
    if (tid < kWave && i < live) mask[(size_t)i * T + tj] = s_word[tid];
}

__global__ void __launch_bounds__(kWave)
k_detect_greedy(const u64* __restrict__ mask, int T, const double* __restrict__ boxes, const double* __restrict__ scores,
             const int* __restrict__ index, const int* __restrict__ state, int max_boxes, double* __restrict__ out_boxes,
             double* __restrict__ out_scores, int* __restrict__ out_index, int* __restrict__ out_count) {
    const int lane = lane_id();
    const int live = state[0], passing = state[1];
    const int live_words = (live + kWave - 1) / kWave;
    // word `lane` of row i; a row's address does not depend on whether the row will be needed
    auto row = [&](int i) -> u64 {
        return (i < live && lane >= i / kWave && lane < live_words) ? mask[(size_t)i * T + lane] : 0ull;
    };
    __shared__ int s_kept[kTopN];
    u64 removed = 0, cur[kAhead], nxt[kAhead];
    int kept = 0;
#pragma unroll
    for (int d = 0; d < kAhead; ++d) cur[d] = row(d);
    for (int base = 0; base < live && kept < max_boxes; base += kAhead) {
#pragma unroll
        for (int d = 0; d < kAhead; ++d) nxt[d] = row(base + kAhead + d);
#pragma unroll
        for (int d = 0; d < kAhead; ++d) {
            const int i = base + d;
            if (i >= live || kept >= max_boxes) break;
            const u64 word = lane_value(removed, i / kWave);
            if ((word >> (i % kWave)) & 1) continue;
            removed |= cur[d];
            if (lane == 0) s_kept[kept] = i;                  // no global load or store inside the chain of decisions
            ++kept;
        }
#pragma unroll
        for (int d = 0; d < kAhead; ++d) cur[d] = nxt[d];
    }
    __syncthreads();
    for (int k = lane; k < kept; k += kWave) {
        const int i = s_kept[k];
#pragma unroll
        for (int c = 0; c < 7; ++c) out_boxes[(size_t)k * 7 + c] = boxes[(size_t)i * 7 + c];
        out_scores[k] = scores[i];
        out_index[k] = index[i];
    }
    if (lane == 0) out_count[0] = kept;
    else if (lane == 1) out_count[1] = passing;
}

struct DetectWs {
    u64 *keys, *mask;
    double *boxes, *scores;
    int *index, *state;
    int npad, tiles;
    size_t bytes;
    DetectWs(void* base, int n, int top_n) {
        npad = (top_n + kWave - 1) / kWave * kWave;
        tiles = npad / kWave;
        Carver c(base);
        keys = c.take<u64>(n);
        boxes = c.take<double>((size_t)npad * 7);
        scores = c.take<double>(npad);
        index = c.take<int>(npad);
        state = c.take<int>(4);
        mask = c.take<u64>((size_t)npad * tiles);
        bytes = c.off;
    }
};

int check_detect(const lisec_rpn_cfg* cfg, const lisec_detect_cfg* det) {
    LISEC_CHECK_ARG(cfg && cfg->outX > 0 && cfg->outY > 0 && cfg->outX % 2 == 0 && cfg->outY % 2 == 0 && cfg->vx > 0 &&
                    cfg->vy > 0 && (long long)cfg->outX * cfg->outY <= (1ll << 29), "bad RPN grid configuration");
    LISEC_CHECK_ARG(det, "no detection configuration");
    LISEC_CHECK_ARG(det->pre_nms_top_n >= 1 && det->pre_nms_top_n <= kTopN, "pre_nms_top_n %d outside 1..%d",
                    det->pre_nms_top_n, kTopN);
    LISEC_CHECK_ARG(det->max_boxes >= 1 && det->max_boxes <= det->pre_nms_top_n, "max_boxes %d outside 1..pre_nms_top_n (%d)",
                    det->max_boxes, det->pre_nms_top_n);
    LISEC_CHECK_ARG(det->iou_threshold >= 0.0 && det->iou_threshold < 1.0, "iou_threshold %g outside [0, 1)",
                    det->iou_threshold);
    LISEC_CHECK_ARG(det->score_threshold == det->score_threshold, "score_threshold is NaN");
    LISEC_CHECK_ARG(det->iou_mode == LISEC_IOU_3D || det->iou_mode == LISEC_IOU_BEV, "iou_mode %d is neither LISEC_IOU_3D nor LISEC_IOU_BEV",
                    det->iou_mode);
    LISEC_CHECK_ARG((det->sigmoid_scores == 0 || det->sigmoid_scores == 1) && (det->inside_only == 0 || det->inside_only == 1),
                    "sigmoid_scores and inside_only are 0 or 1");
    return 0;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_detect_workspace_bytes(const lisec_rpn_cfg* cfg, const lisec_detect_cfg* det) {
    if (check_detect(cfg, det)) return 0;
    return DetectWs(nullptr, 2 * cfg->outX * cfg->outY, det->pre_nms_top_n).bytes;
}

extern "C" int lisec_detect(const lisec_rpn_cfg* cfg, const lisec_detect_cfg* det, const float* cls, int cls_stride,
                            const float* reg, int reg_stride, void* workspace, size_t workspace_bytes, double* out_boxes,
                            double* out_scores, int32_t* out_index, int32_t* out_count, lisec_stream_t stream_) {
    if (int rc = check_detect(cfg, det)) return rc;
    LISEC_CHECK_ARG(cls && reg && workspace && out_boxes && out_scores && out_index && out_count && cls_stride >= 2 &&
                    reg_stride >= 14, "bad arguments");
    const int n = 2 * cfg->outX * cfg->outY;
    DetectWs ws(workspace, n, det->pre_nms_top_n);
    if (workspace_bytes < ws.bytes) {
        set_error("detect workspace too small");
        return LISEC_ENOSPC;
    }
    int idx_bits = 0;
    while ((1ll << idx_bits) < n) ++idx_bits;                 // the flat index n - 1 fits idx_bits bits
    hipStream_t st = static_cast<hipStream_t>(stream_);
    LISEC_LAUNCH(k_detect_key, dim3(cdiv(n, 256)), dim3(256), 0, st, cls, cls_stride, reg, reg_stride, *cfg,
                 det->score_threshold, det->inside_only, ws.keys);
    LISEC_LAUNCH(k_detect_select, dim3(1), dim3(kSelThreads), 0, st, ws.keys, n, idx_bits, det->pre_nms_top_n, ws.npad, reg,
                 reg_stride, *cfg, det->sigmoid_scores, ws.boxes, ws.scores, ws.index, ws.state);
    LISEC_LAUNCH(k_detect_mask, dim3(ws.tiles * (ws.tiles + 1) / 2), dim3(kMaskWaves * kWave), 0, st, ws.boxes, ws.state, ws.tiles,
                 det->iou_threshold, det->iou_mode, ws.mask);
    LISEC_LAUNCH(k_detect_greedy, dim3(1), dim3(kWave), 0, st, ws.mask, ws.tiles, ws.boxes, ws.scores, ws.index, ws.state,
                 det->max_boxes, out_boxes, out_scores, out_index, out_count);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
