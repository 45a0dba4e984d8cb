// Training-time augmentation of a sweep together with its boxes (VoxelNet section 3.3) and the RPN label maps of the
// augmented boxes, all on the device (gfx950); include/lisec_hip.h section 5c.
//
//   lisec_augment_draw    the transforms of one (sweep, epoch): per-box yaw / translation noise with collision rejection,
//                         one global scale and rotation.  ONE workgroup: box b's test reads the poses boxes < b ended with.
//   lisec_augment_apply   moves the points: a point inside a box rides with it, then every point takes the global transform.
//   lisec_rpn_targets     fixBoxScaling + lisec_rpn_labels + the region balancing of serialize_data.py:310-325 with
//                         counter-based keys, written as the float32 maps the training step reads.
//   lisec_augment_owner   the lowest box holding each point: what the object database is cut out with.
//   lisec_augment_sample  ground-truth sampling (SECOND section 3.2): K database objects drawn, collision-checked against
//                         the scene and against each other, the accepted ones appended to the box table.  ONE workgroup.
//   lisec_augment_paste   the scene points (those inside a pasted box removed) followed by the accepted objects' points.
//   The *_n entries read the box count from the device (what lisec_augment_sample leaves there) and share the kernels.
//
// Box rows are (x, y, z, l, w, h, yaw) in ego metres with z the box CENTRE (boxes.annotationBoxes: the annotation's
// translation): the z extent is [z - h/2, z + h/2].  The footprint is box_corners of box_geom.h: axes u = (cos yaw, -sin yaw)
// with half extent w/2 and v = (sin yaw, cos yaw) with half extent l/2.
//
// Random numbers: Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit seed (low word, high word), counter =
// (stream, item, epoch, index).  Streams: 0 global, 1 per-box, 2 balance, 3 sampling (4: voxelize.hip).  Integer-exact, so a numpy restatement
// reproduces every draw bit for bit; uniform = (u32 + 0.5) * 2^-32, normals by Box-Muller, both in double.
// Integer / latency-bound work in float64: no MFMA.
#include <algorithm>

#include "common.h"
#include "box_geom.h"
#include "philox.h"

namespace lisec {
namespace {

constexpr int kMaxBoxes = LISEC_AUG_MAX_BOXES;
constexpr int kMaxAttempts = LISEC_AUG_MAX_ATTEMPTS;
constexpr int kMaxSamples = LISEC_AUG_MAX_SAMPLES;
constexpr int kChunk = 128;                        // boxes staged in LDS at a time by k_augment_apply
constexpr double kTwoPi = 6.283185307179586476925286766559;

__device__ __forceinline__ double uniform01(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

__device__ __forceinline__ void box_muller(uint32_t w1, uint32_t w2, double& z0, double& z1) {
    const double r = sqrt(-2.0 * log(uniform01(w1))), t = kTwoPi * uniform01(w2);
    z0 = r * cos(t); z1 = r * sin(t);
}

// ---- draw ----------------------------------------------------------------------------------------------------------------
struct Pose { double cx, cy, r; Pt c[4]; };        // a footprint with its bounding circle

__device__ __forceinline__ void set_pose(Pose& p, double x, double y, double l, double w, double yaw) {
    const double row[7] = {x, y, 0.0, l, w, 0.0, yaw};
    p.cx = x; p.cy = y; p.r = 0.5 * hypot(l, w);
    box_corners(row, p.c);
}

struct Drawn { double s, alpha, cs, sn; };

// the outputs of box b: its transform row, the accepted attempt with its integer draws, and the row after both stages
__device__ void emit_box(const double* __restrict__ box, int b, const double* t, int acc, const uint32_t* words,
                         const Drawn& g, double* __restrict__ transforms, double* __restrict__ boxes_out,
                         int* __restrict__ attempt_out, uint32_t* __restrict__ draws_out) {
    for (int c = 0; c < 4; ++c) transforms[b * 4 + c] = t[c];
    attempt_out[b] = acc;
    for (int c = 0; c < 8; ++c) draws_out[4 + b * 8 + c] = words ? words[c] : 0u;
    const double x = box[0] + t[0], y = box[1] + t[1], z = box[2] + t[2];
    double* o = boxes_out + (size_t)b * 7;
    o[0] = g.s * (x * g.cs - y * g.sn);
    o[1] = g.s * (x * g.sn + y * g.cs);
    o[2] = g.s * z;
    o[3] = g.s * box[3]; o[4] = g.s * box[4]; o[5] = g.s * box[5];
    o[6] = box[6] + t[3] - g.alpha;                // u = (cos yaw, -sin yaw): a counter-clockwise turn LOWERS yaw
}

__global__ void __launch_bounds__(256)
k_augment_draw(const double* __restrict__ boxes, int B, const int* __restrict__ n_dev, lisec_augment_params P, uint32_t k0,
               uint32_t k1, uint32_t item, uint32_t epoch, double* __restrict__ transforms, double* __restrict__ global_out,
               double* __restrict__ boxes_out, int* __restrict__ attempt_out, uint32_t* __restrict__ draws_out) {
    if (n_dev) B = min(B, max(*n_dev, 0));         // the count lisec_augment_sample left on the device; B bounds it
    __shared__ Pose pose[kMaxBoxes];               // 45 KB: the current footprint of every box
    __shared__ Pose cand[kMaxAttempts];
    __shared__ double cand_t[kMaxAttempts][4];
    __shared__ uint32_t cand_w[kMaxAttempts][8];
    __shared__ int collide[kMaxAttempts];
    __shared__ Drawn g;
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += 256) {
        const double* r = boxes + (size_t)b * 7;
        set_pose(pose[b], r[0], r[1], r[3], r[4], r[6]);
    }
    if (tid == 0) {
        const U4 w = philox4x32_10(0u, item, epoch, 0u, k0, k1);
        g.s = P.scale_lo + (P.scale_hi - P.scale_lo) * uniform01(w.v[0]);
        g.alpha = P.rot_global * (2.0 * uniform01(w.v[1]) - 1.0);
        g.cs = cos(g.alpha); g.sn = sin(g.alpha);
        global_out[0] = g.s; global_out[1] = g.alpha;
        for (int c = 0; c < 4; ++c) draws_out[c] = w.v[c];
    }
    __syncthreads();
    const int A = P.attempts;
    if (A == 0) {
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = tid; b < B; b += 256)
            emit_box(boxes + (size_t)b * 7, b, zero, -1, nullptr, g, transforms, boxes_out, attempt_out, draws_out);
        return;
    }
    for (int b = 0; b < B; ++b) {
        const double* r = boxes + (size_t)b * 7;
        if (tid < A) {                             // the candidates of box b
            const uint32_t idx = (uint32_t)(b * kMaxAttempts + tid) * 2u;
            const U4 w0 = philox4x32_10(1u, item, epoch, idx, k0, k1), w1 = philox4x32_10(1u, item, epoch, idx + 1u, k0, k1);
            double n0, n1, n2, unused;
            box_muller(w0.v[1], w0.v[2], n0, n1);
            box_muller(w1.v[0], w1.v[1], n2, unused);
            double* t = cand_t[tid];
            t[0] = P.sigma[0] * n0; t[1] = P.sigma[1] * n1; t[2] = P.sigma[2] * n2;
            t[3] = P.rot_box * (2.0 * uniform01(w0.v[0]) - 1.0);
            set_pose(cand[tid], r[0] + t[0], r[1] + t[1], r[3], r[4], r[6] + t[3]);
            for (int c = 0; c < 4; ++c) { cand_w[tid][c] = w0.v[c]; cand_w[tid][4 + c] = w1.v[c]; }
            collide[tid] = 0;
        }
        __syncthreads();
        for (int t = tid; t < A * B; t += 256) {   // attempts x other boxes across the workgroup
            const int a = t / B, j = t - a * B;
            if (j == b) continue;
            const Pose& p = cand[a];
            const Pose& q = pose[j];
            const double dx = p.cx - q.cx, dy = p.cy - q.cy, rr = p.r + q.r;
            if (dx * dx + dy * dy > rr * rr * 1.0000001) continue;       // bounding circles apart: area exactly 0
            if (quad_intersection_area(p.c, q.c) != 0.0) collide[a] = 1;
        }
        __syncthreads();
        if (tid == 0) {
            int acc = -1;
            for (int a = 0; a < A && acc < 0; ++a)
                if (!collide[a]) acc = a;
            const double zero[4] = {0.0, 0.0, 0.0, 0.0};
            emit_box(r, b, acc < 0 ? zero : cand_t[acc], acc, acc < 0 ? nullptr : cand_w[acc], g, transforms, boxes_out,
                     attempt_out, draws_out);
            if (acc >= 0) pose[b] = cand[acc];
        }
        __syncthreads();
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------
struct Slab { double cx, cy, r2, hw, hl, zlo, zhi, cs, sn; };   // a box as the closed point-in-box test reads it
struct Staged { Slab s; double ncx, ncy, ncs, nsn, dz; int moved; };

__device__ __forceinline__ Slab make_slab(const double* __restrict__ r) {
    Slab q;
    q.cx = r[0]; q.cy = r[1]; q.hw = 0.5 * r[4]; q.hl = 0.5 * r[3];
    q.r2 = (q.hw * q.hw + q.hl * q.hl) * 1.0000001;
    q.zlo = r[2] - 0.5 * r[5]; q.zhi = r[2] + 0.5 * r[5];
    q.cs = cos(r[6]); q.sn = sin(r[6]);
    return q;
}

// the closed slab test of section 5c; (du, dv) are the point's coordinates in the box's frame when it is inside
__device__ __forceinline__ bool inside_slab(const Slab& q, double x, double y, double z, double& du, double& dv) {
    const double dx = x - q.cx, dy = y - q.cy;
    if (dx * dx + dy * dy > q.r2) return false;
    du = dx * q.cs - dy * q.sn; dv = dx * q.sn + dy * q.cs;
    return fabs(du) <= q.hw && fabs(dv) <= q.hl && z >= q.zlo && z <= q.zhi;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_augment_apply(const T* __restrict__ pts, int n, int stride, const double* __restrict__ boxes, int B,
                const int* __restrict__ n_dev, const double* __restrict__ tr, const double* __restrict__ glob,
                double pad_limit, T* __restrict__ out) {
    __shared__ Staged sb[kChunk];
    if (n_dev) B = min(B, max(*n_dev, 0));
    const int tid = threadIdx.x, per = gridDim.x * 256;
    const int trips = (int)(((long long)n + per - 1) / per), chunks = (B + kChunk - 1) / kChunk;
    const double s = glob[0], alpha = glob[1], gc = cos(alpha), gs = sin(alpha);
    int staged = -1;                               // the chunk sb holds (uniform over the workgroup)
    for (int trip = 0; trip < trips; ++trip) {
        const long long i = (long long)trip * per + (long long)blockIdx.x * 256 + tid;
        const bool live = i < n;
        double x = 0.0, y = 0.0, z = 0.0;
        if (live) {
            const T* p = pts + (size_t)i * stride;
            x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
        }
        const bool pad = !(fabs(x) < pad_limit);   // a pad row of the step's point buffer (or NaN): left as it is
        bool found = !live || pad;
        for (int ch = 0; ch < chunks; ++ch) {
            if (staged != ch) {
                __syncthreads();
                for (int k = tid; k < kChunk && ch * kChunk + k < B; k += 256) {
                    const double* r = boxes + (size_t)(ch * kChunk + k) * 7;
                    const double* t = tr + (size_t)(ch * kChunk + k) * 4;
                    Staged q;
                    q.s = make_slab(r);
                    q.ncx = r[0] + t[0]; q.ncy = r[1] + t[1]; q.dz = t[2];
                    q.ncs = cos(r[6] + t[3]); q.nsn = sin(r[6] + t[3]);
                    q.moved = t[0] != 0.0 || t[1] != 0.0 || t[2] != 0.0 || t[3] != 0.0;   // a box that stays: its points too
                    sb[k] = q;
                }
                __syncthreads();
                staged = ch;
            }
            if (found) continue;
            const int m = min(kChunk, B - ch * kChunk);
            for (int k = 0; k < m; ++k) {          // in index order: the lowest box holding the point takes it
                const Staged& q = sb[k];
                double du, dv;
                if (inside_slab(q.s, x, y, z, du, dv)) {
                    if (q.moved) {
                        x = q.ncx + du * q.ncs + dv * q.nsn;
                        y = q.ncy - du * q.nsn + dv * q.ncs;
                        z = z + q.dz;
                    }
                    found = true;
                    break;
                }
            }
        }
        if (live) {
            T* o = out + (size_t)i * 3;
            if (pad) { o[0] = (T)x; o[1] = (T)y; o[2] = (T)z; }
            else {
                o[0] = (T)(s * (x * gc - y * gs));
                o[1] = (T)(s * (x * gs + y * gc));
                o[2] = (T)(s * z);
            }
        }
    }
}

// ---- owner ---------------------------------------------------------------------------------------------------------------
// one point per lane, the boxes through LDS in chunks as k_augment_apply stages them
template <typename T>
__global__ void __launch_bounds__(256)
k_augment_owner(const T* __restrict__ pts, int n, int stride, const double* __restrict__ boxes, int B, double pad_limit,
                int* __restrict__ owner) {
    __shared__ Slab sb[kChunk];
    const int tid = threadIdx.x, per = gridDim.x * 256;
    const int trips = (int)(((long long)n + per - 1) / per), chunks = (B + kChunk - 1) / kChunk;
    int staged = -1;                               // the chunk sb holds (uniform over the workgroup)
    for (int trip = 0; trip < trips; ++trip) {
        const long long i = (long long)trip * per + (long long)blockIdx.x * 256 + tid;
        const bool live = i < n;
        double x = 0.0, y = 0.0, z = 0.0;
        if (live) {
            const T* p = pts + (size_t)i * stride;
            x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
        }
        int own = -1;
        bool found = !live || !(fabs(x) < pad_limit);   // a pad row belongs to no box
        for (int ch = 0; ch < chunks; ++ch) {
            if (staged != ch) {
                __syncthreads();
                for (int k = tid; k < kChunk && ch * kChunk + k < B; k += 256)
                    sb[k] = make_slab(boxes + (size_t)(ch * kChunk + k) * 7);
                __syncthreads();
                staged = ch;
            }
            if (found) continue;
            const int m = min(kChunk, B - ch * kChunk);
            for (int k = 0; k < m; ++k) {          // in index order: the lowest box holding the point owns it
                double du, dv;
                if (inside_slab(sb[k], x, y, z, du, dv)) { own = ch * kChunk + k; found = true; break; }
            }
        }
        if (live) owner[i] = own;
    }
}

// ---- sample --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool poses_collide(const Pose& p, const Pose& q) {
    const double dx = p.cx - q.cx, dy = p.cy - q.cy, rr = p.r + q.r;
    if (dx * dx + dy * dy > rr * rr * 1.0000001) return false;           // bounding circles apart: area exactly 0
    return quad_intersection_area(p.c, q.c) != 0.0;
}

// B scene boxes, K candidates (B + K <= kMaxBoxes), M database objects.  pose[0, B) are the scene's footprints and
// pose[B, B + K) the candidates', the layout k_augment_draw keeps its boxes in.
__global__ void __launch_bounds__(256)
k_augment_sample(const double* __restrict__ boxes, int B, const double* __restrict__ db_boxes,
                 const int* __restrict__ db_offsets, int M, int K, uint32_t k0, uint32_t k1, uint32_t item, uint32_t epoch,
                 int* __restrict__ index_out, int* __restrict__ n_boxes_out, double* __restrict__ boxes_all,
                 int* __restrict__ point_offset, uint32_t* __restrict__ draws_out) {
    __shared__ Pose pose[kMaxBoxes];
    __shared__ unsigned long long hits[kMaxSamples];   // bit m of hits[k]: candidate k overlaps candidate m < k
    __shared__ int scene_hit[kMaxSamples];
    __shared__ int cand_idx[kMaxSamples], cand_cnt[kMaxSamples], slot[kMaxSamples], offs[kMaxSamples + 1];
    __shared__ int n_acc;
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += 256) {
        const double* r = boxes + (size_t)b * 7;
        set_pose(pose[b], r[0], r[1], r[3], r[4], r[6]);
    }
    if (tid < K) {
        const U4 w = philox4x32_10(3u, item, epoch, (uint32_t)tid, k0, k1);
        for (int c = 0; c < 4; ++c) draws_out[tid * 4 + c] = w.v[c];
        int idx = -1, cnt = 0;
        if (M > 0) {
            idx = (int)(((unsigned long long)w.v[0] * (unsigned long long)M) >> 32);     // < M: integer-exact
            cnt = db_offsets[idx + 1] - db_offsets[idx];
            const double* r = db_boxes + (size_t)idx * 7;
            set_pose(pose[B + tid], r[0], r[1], r[3], r[4], r[6]);
        }
        cand_idx[tid] = idx; cand_cnt[tid] = cnt;
        scene_hit[tid] = 0; hits[tid] = 0ull;
    }
    __syncthreads();
    if (M > 0) {
        for (int t = tid; t < K * B; t += 256) {       // candidates x scene boxes across the workgroup
            const int k = t / B, j = t - k * B;
            if (poses_collide(pose[B + k], pose[j])) scene_hit[k] = 1;
        }
        for (int t = tid; t < K * K; t += 256) {       // candidates x earlier candidates: the K x K bit matrix
            const int k = t / K, m = t - k * K;
            if (m < k && poses_collide(pose[B + k], pose[B + m])) atomicOr(&hits[k], 1ull << m);
        }
    }
    __syncthreads();
    if (tid == 0) {                                    // the greedy walk: k is taken iff it touches nothing taken before it
        unsigned long long taken = 0ull;
        int acc = 0, off = 0;
        for (int k = 0; k < K; ++k) {
            const bool ok = cand_idx[k] >= 0 && !scene_hit[k] && (hits[k] & taken) == 0ull;
            offs[k] = off;
            slot[k] = ok ? acc : -1;
            if (ok) { taken |= 1ull << k; ++acc; off += cand_cnt[k]; }
        }
        offs[K] = off;
        n_acc = acc;
        n_boxes_out[0] = B + acc;
    }
    __syncthreads();
    for (int k = tid; k <= K; k += 256) point_offset[k] = offs[k];
    for (int k = tid; k < K; k += 256) index_out[k] = slot[k] >= 0 ? cand_idx[k] : -1;
    for (int t = tid; t < (B + K) * 7; t += 256) {     // the scene rows, zeros past the accepted ones
        const int row = t / 7;
        if (row < B) boxes_all[t] = boxes[t];
        else if (row >= B + n_acc) boxes_all[t] = 0.0;
    }
    for (int t = tid; t < K * 7; t += 256) {           // the accepted rows, compacted in order of k
        const int k = t / 7, c = t - k * 7;
        if (slot[k] >= 0) boxes_all[(size_t)(B + slot[k]) * 7 + c] = db_boxes[(size_t)cand_idx[k] * 7 + c];
    }
}

// ---- paste ---------------------------------------------------------------------------------------------------------------
// rows [0, n): the scene (a live point inside an accepted pasted box becomes a pad row); [n, n + n_add): the accepted
// objects' points in order of k; [n + n_add, cap): pad rows
template <typename T>
__global__ void __launch_bounds__(256)
k_augment_paste(const T* __restrict__ pts, int n, int stride, const T* __restrict__ db_points,
                const int* __restrict__ db_offsets, const int* __restrict__ index, const int* __restrict__ point_offset,
                const double* __restrict__ boxes_all, int B, const int* __restrict__ n_boxes_dev, int K, double pad_limit,
                T* __restrict__ out, int cap) {
    __shared__ Slab sb[kMaxSamples];
    __shared__ int offs[kMaxSamples + 1], first[kMaxSamples];
    const int tid = threadIdx.x;
    const int n_acc = min(max(*n_boxes_dev - B, 0), K);
    for (int k = tid; k < n_acc; k += 256) sb[k] = make_slab(boxes_all + (size_t)(B + k) * 7);
    for (int k = tid; k <= K; k += 256) offs[k] = point_offset[k];
    for (int k = tid; k < K; k += 256) first[k] = index[k] >= 0 ? db_offsets[index[k]] : 0;
    __syncthreads();
    const int n_add = offs[K];
    const T pad = (T)(2.0 * pad_limit);
    for (long long i = (long long)blockIdx.x * 256 + tid; i < cap; i += (long long)gridDim.x * 256) {
        T x = pad, y = pad, z = pad;
        if (i < n) {
            const T* p = pts + (size_t)i * stride;
            x = p[0]; y = p[1]; z = p[2];
            if (fabs((double)x) < pad_limit) {
                bool hit = false;
                double du, dv;
                for (int k = 0; k < n_acc && !hit; ++k) hit = inside_slab(sb[k], (double)x, (double)y, (double)z, du, dv);
                if (hit) { x = pad; y = pad; z = pad; }
            }
        } else if (i - n < n_add) {
            const int j = (int)(i - n);
            int lo = 0, hi = K;                        // the last k with offs[k] <= j: a rejected candidate is an empty range
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (offs[mid] <= j) lo = mid; else hi = mid;
            }
            const T* p = db_points + (size_t)(first[lo] + (j - offs[lo])) * 3;
            x = p[0]; y = p[1]; z = p[2];
        }
        T* o = out + (size_t)i * 3;
        o[0] = x; o[1] = y; o[2] = z;
    }
}

// ---- label maps ----------------------------------------------------------------------------------------------------------
__global__ void k_fix_scaling(const double* __restrict__ boxes, int B, const int* __restrict__ n_dev, double sx, double sy,
                              double* __restrict__ fixed) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;    // fixBoxScaling (serialize_data.py:181-191)
    if (n_dev) B = min(B, max(*n_dev, 0));
    if (b >= B) return;
    const double* r = boxes + (size_t)b * 7;
    double* f = fixed + (size_t)b * 7;
    f[0] = r[0] * sx; f[1] = r[1] * sy; f[2] = r[2]; f[3] = r[3] * sx; f[4] = r[4] * sy; f[5] = r[5]; f[6] = r[6];
}

// Region balancing (serialize_data.py:310-325) without random.sample: every candidate anchor gets the key
// (Philox(2, item, epoch, flat index)[0] << 32 | flat index) and the `keep` smallest keys of its class survive -- the key is
// unique, and equal Philox words fall to the smaller flat index.  One workgroup: the counts, then an 8-pass radix select
// of the keep-th smallest key per class.  sel = {threshold, mode} x {positive, negative}; mode 0 keeps all, 1 keeps keys
// <= threshold, 2 keeps none.
__global__ void __launch_bounds__(1024)
k_balance_select(const double* __restrict__ valid, const double* __restrict__ overlap, int n, int max_regions, uint32_t k0,
                 uint32_t k1, uint32_t item, uint32_t epoch, unsigned long long* __restrict__ keys,
                 uint8_t* __restrict__ cls, unsigned long long* __restrict__ sel) {
    __shared__ int hist[256];
    __shared__ int cnt[2];
    __shared__ int bucket_s, k_s;
    const int tid = threadIdx.x;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const double v = valid[i], o = overlap[i];
        const uint8_t c = v == 1.0 ? (o == 1.0 ? 1 : (o == 0.0 ? 2 : 0)) : 0;
        cls[i] = c;
        if (c) {
            keys[i] = ((unsigned long long)philox4x32_10(2u, item, epoch, (uint32_t)i, k0, k1).v[0] << 32) | (uint32_t)i;
            atomicAdd(&cnt[c - 1], 1);
        }
    }
    __syncthreads();
    const int n_pos = cnt[0], n_neg = cnt[1];
    const int keep_pos = min(n_pos, max_regions / 2);
    const int keep_neg = n_neg + keep_pos > max_regions ? keep_pos : n_neg;
    for (int c = 0; c < 2; ++c) {
        const int members = c ? n_neg : n_pos, keep = c ? keep_neg : keep_pos;
        unsigned long long prefix = 0ull;
        int mode = keep >= members ? 0 : (keep == 0 ? 2 : 1);
        if (mode == 1) {
            int k = keep;
            for (int shift = 56; shift >= 0; shift -= 8) {
                if (tid < 256) hist[tid] = 0;
                __syncthreads();
                const unsigned long long above = shift == 56 ? 0ull : ~0ull << (shift + 8);
                for (int i = tid; i < n; i += 1024)
                    if (cls[i] == c + 1 && (keys[i] & above) == prefix) atomicAdd(&hist[(keys[i] >> shift) & 255], 1);
                __syncthreads();
                if (tid == 0) {
                    int cum = 0, h = 0;
                    for (; h < 255 && cum + hist[h] < k; ++h) cum += hist[h];
                    bucket_s = h; k_s = k - cum;
                }
                __syncthreads();
                prefix |= (unsigned long long)bucket_s << shift;
                k = k_s;
            }
        }
        if (tid == 0) { sel[2 * c] = prefix; sel[2 * c + 1] = (unsigned long long)mode; }
    }
}

// y_cls = valid + overlap, y_reg = out_regress + repeat(overlap, 7) (serialize_data.py:327-338) as float32, with the
// balancing applied to `valid`
__global__ void k_targets_finish(const double* __restrict__ valid, const double* __restrict__ overlap,
                                 const double* __restrict__ out_reg, int n, int balance,
                                 const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ cls,
                                 const unsigned long long* __restrict__ sel, float* __restrict__ y_cls,
                                 float* __restrict__ y_reg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = valid[i];
    const double o = overlap[i];
    if (balance && cls[i]) {
        const int c = cls[i] - 1;
        const unsigned long long mode = sel[2 * c + 1];
        if (mode == 2ull || (mode == 1ull && keys[i] > sel[2 * c])) v = 0.0;
    }
    y_cls[i] = (float)(v + o);
    const size_t at = (size_t)(i >> 1) * 14 + (size_t)(i & 1) * 7;
    for (int c = 0; c < 7; ++c) y_reg[at + c] = (float)(out_reg[at + c] + o);
}

struct TargetWs {
    double *fixed, *valid, *overlap, *out_reg;
    void* labels;
    unsigned long long *keys, *sel;
    uint8_t* cls;
    size_t labels_bytes, bytes;
    TargetWs(void* base, size_t cells, int B) {
        Carver c(base);
        fixed = c.take<double>((size_t)(B + 1) * 7);
        valid = c.take<double>(cells * 2);
        overlap = c.take<double>(cells * 2);
        out_reg = c.take<double>(cells * 14);
        labels_bytes = lisec_rpn_labels_workspace_bytes(B);
        labels = c.take<char>(labels_bytes);
        keys = c.take<unsigned long long>(cells * 2);
        sel = c.take<unsigned long long>(4);
        cls = c.take<uint8_t>(cells * 2);
        bytes = c.off;
    }
};

int check_params(const lisec_augment_params* p) {
    LISEC_CHECK_ARG(p, "augmentation parameters missing");
    LISEC_CHECK_ARG(p->attempts >= 0 && p->attempts <= kMaxAttempts, "attempts must lie in [0, %d], not %d", kMaxAttempts,
                    p->attempts);
    LISEC_CHECK_ARG(p->rot_box >= 0 && p->rot_global >= 0 && p->sigma[0] >= 0 && p->sigma[1] >= 0 && p->sigma[2] >= 0 &&
                    p->scale_lo > 0 && p->scale_hi >= p->scale_lo, "augmentation parameters out of range");
    return 0;
}

// the three stages that run behind the sampling: n_dev == nullptr is the host count n_boxes, else n_boxes bounds *n_dev
int draw_impl(const double* boxes, int n_boxes, const int32_t* n_dev, const lisec_augment_params* params,
              unsigned long long seed, unsigned int item, unsigned int epoch, double* transforms, double* global,
              double* boxes_out, int32_t* attempt, uint32_t* draws, lisec_stream_t stream_) {
    if (int rc = check_params(params)) return rc;
    LISEC_CHECK_ARG(n_boxes >= 0, "negative box count");
    LISEC_CHECK_ARG(n_boxes <= kMaxBoxes, "%d boxes exceed LISEC_AUG_MAX_BOXES = %d (the poses live in LDS)", n_boxes,
                    kMaxBoxes);
    LISEC_CHECK_ARG(global && draws && (n_boxes == 0 || (boxes && transforms && boxes_out && attempt)), "bad arguments");
    LISEC_LAUNCH(k_augment_draw, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream_), boxes, n_boxes, n_dev, *params,
                 (uint32_t)seed, (uint32_t)(seed >> 32), item, epoch, transforms, global, boxes_out, attempt, draws);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

int apply_impl(const void* points, int dtype, int n, int stride, const double* boxes_before, int n_boxes,
               const int32_t* n_dev, const double* transforms, const double* global, double pad_limit, void* points_out,
               lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n >= 0 && stride >= 3 && (dtype == 0 || dtype == 1) && n_boxes >= 0 && global && pad_limit > 0 &&
                    (n == 0 || (points && points_out)) && (n_boxes == 0 || (boxes_before && transforms)), "bad arguments");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(std::min(cdiv(n, 256), 4 * cu_count()));
    if (dtype == 0)
        LISEC_LAUNCH(k_augment_apply<float>, grid, dim3(256), 0, st, static_cast<const float*>(points), n, stride,
                     boxes_before, n_boxes, n_dev, transforms, global, pad_limit, static_cast<float*>(points_out));
    else
        LISEC_LAUNCH(k_augment_apply<double>, grid, dim3(256), 0, st, static_cast<const double*>(points), n, stride,
                     boxes_before, n_boxes, n_dev, transforms, global, pad_limit, static_cast<double*>(points_out));
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

int targets_impl(const lisec_rpn_cfg* cfg, const double* boxes, int n_boxes, const int32_t* n_dev, double scale_x,
                 double scale_y, double iou_lo, double iou_hi, int balance, int max_regions, unsigned long long seed,
                 unsigned int item, unsigned int epoch, void* workspace, size_t workspace_bytes, float* y_cls, float* y_reg,
                 lisec_stream_t stream_) {
    LISEC_CHECK_ARG(cfg && cfg->outX > 0 && cfg->outY > 0, "bad RPN grid configuration");
    LISEC_CHECK_ARG(n_boxes >= 0 && (n_boxes == 0 || boxes) && workspace && y_cls && y_reg && max_regions >= 0 &&
                    max_regions % 2 == 0, "bad arguments");
    const size_t cells = (size_t)cfg->outX * cfg->outY;
    TargetWs ws(workspace, cells, n_boxes);
    if (workspace_bytes < ws.bytes) {
        set_error("rpn_targets workspace too small");
        return LISEC_ENOSPC;
    }
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (n_boxes > 0)
        LISEC_LAUNCH(k_fix_scaling, dim3(cdiv(n_boxes, 64)), dim3(64), 0, st, boxes, n_boxes, n_dev, scale_x, scale_y,
                     ws.fixed);
    if (int rc = rpn_labels_counted(cfg, ws.fixed, n_boxes, n_dev, iou_lo, iou_hi, ws.labels, ws.labels_bytes, ws.valid,
                                    ws.overlap, ws.out_reg, stream_))
        return rc;
    const int n = 2 * (int)cells;
    if (balance)
        LISEC_LAUNCH(k_balance_select, dim3(1), dim3(1024), 0, st, ws.valid, ws.overlap, n, max_regions, (uint32_t)seed,
                     (uint32_t)(seed >> 32), item, epoch, ws.keys, ws.cls, ws.sel);
    LISEC_LAUNCH(k_targets_finish, dim3(cdiv(n, 256)), dim3(256), 0, st, ws.valid, ws.overlap, ws.out_reg, n, balance,
                 ws.keys, ws.cls, ws.sel, y_cls, y_reg);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" int lisec_augment_draw(const double* boxes, int n_boxes, const lisec_augment_params* params,
                                  unsigned long long seed, unsigned int item, unsigned int epoch, double* transforms,
                                  double* global, double* boxes_out, int32_t* attempt, uint32_t* draws,
                                  lisec_stream_t stream) {
    return draw_impl(boxes, n_boxes, nullptr, params, seed, item, epoch, transforms, global, boxes_out, attempt, draws, stream);
}

extern "C" int lisec_augment_draw_n(const double* boxes, const int32_t* n_boxes_dev, int max_boxes,
                                    const lisec_augment_params* params, unsigned long long seed, unsigned int item,
                                    unsigned int epoch, double* transforms, double* global, double* boxes_out,
                                    int32_t* attempt, uint32_t* draws, lisec_stream_t stream) {
    LISEC_CHECK_ARG(n_boxes_dev, "the device-side box count is missing");
    return draw_impl(boxes, max_boxes, n_boxes_dev, params, seed, item, epoch, transforms, global, boxes_out, attempt, draws,
                     stream);
}

extern "C" int lisec_augment_apply(const void* points, int dtype, int n, int stride, const double* boxes_before,
                                   int n_boxes, const double* transforms, const double* global, double pad_limit,
                                   void* points_out, lisec_stream_t stream) {
    return apply_impl(points, dtype, n, stride, boxes_before, n_boxes, nullptr, transforms, global, pad_limit, points_out,
                      stream);
}

extern "C" int lisec_augment_apply_n(const void* points, int dtype, int n, int stride, const double* boxes_before,
                                     const int32_t* n_boxes_dev, int max_boxes, const double* transforms,
                                     const double* global, double pad_limit, void* points_out, lisec_stream_t stream) {
    LISEC_CHECK_ARG(n_boxes_dev, "the device-side box count is missing");
    return apply_impl(points, dtype, n, stride, boxes_before, max_boxes, n_boxes_dev, transforms, global, pad_limit,
                      points_out, stream);
}

extern "C" size_t lisec_rpn_targets_workspace_bytes(const lisec_rpn_cfg* cfg, int n_boxes) {
    if (!cfg || cfg->outX <= 0 || cfg->outY <= 0 || n_boxes < 0) return 0;
    return TargetWs(nullptr, (size_t)cfg->outX * cfg->outY, n_boxes).bytes;
}

extern "C" int lisec_rpn_targets(const lisec_rpn_cfg* cfg, const double* boxes, int n_boxes, double scale_x, double scale_y,
                                 double iou_lo, double iou_hi, int balance, int max_regions, unsigned long long seed,
                                 unsigned int item, unsigned int epoch, void* workspace, size_t workspace_bytes,
                                 float* y_cls, float* y_reg, lisec_stream_t stream) {
    return targets_impl(cfg, boxes, n_boxes, nullptr, scale_x, scale_y, iou_lo, iou_hi, balance, max_regions, seed, item,
                        epoch, workspace, workspace_bytes, y_cls, y_reg, stream);
}

extern "C" int lisec_rpn_targets_n(const lisec_rpn_cfg* cfg, const double* boxes, const int32_t* n_boxes_dev, int max_boxes,
                                   double scale_x, double scale_y, double iou_lo, double iou_hi, int balance,
                                   int max_regions, unsigned long long seed, unsigned int item, unsigned int epoch,
                                   void* workspace, size_t workspace_bytes, float* y_cls, float* y_reg,
                                   lisec_stream_t stream) {
    LISEC_CHECK_ARG(n_boxes_dev, "the device-side box count is missing");
    return targets_impl(cfg, boxes, max_boxes, n_boxes_dev, scale_x, scale_y, iou_lo, iou_hi, balance, max_regions, seed, item,
                        epoch, workspace, workspace_bytes, y_cls, y_reg, stream);
}

extern "C" int lisec_augment_owner(const void* points, int dtype, int n, int stride, const double* boxes, int n_boxes,
                                   double pad_limit, int32_t* owner, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n >= 0 && stride >= 3 && (dtype == 0 || dtype == 1) && n_boxes >= 0 && pad_limit > 0 &&
                    (n == 0 || (points && owner)) && (n_boxes == 0 || boxes), "bad arguments");
    if (n == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(std::min(cdiv(n, 256), 4 * cu_count()));
    if (dtype == 0)
        LISEC_LAUNCH(k_augment_owner<float>, grid, dim3(256), 0, st, static_cast<const float*>(points), n, stride, boxes,
                     n_boxes, pad_limit, owner);
    else
        LISEC_LAUNCH(k_augment_owner<double>, grid, dim3(256), 0, st, static_cast<const double*>(points), n, stride, boxes,
                     n_boxes, pad_limit, owner);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_augment_sample(const double* boxes, int n_boxes, const double* db_boxes, const int32_t* db_offsets,
                                    int n_objects, int n_samples, unsigned long long seed, unsigned int item,
                                    unsigned int epoch, int32_t* index, int32_t* n_boxes_out, double* boxes_all,
                                    int32_t* point_offset, uint32_t* draws, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n_boxes >= 0 && n_objects >= 0 && n_samples >= 0, "negative count");
    LISEC_CHECK_ARG(n_samples <= kMaxSamples, "%d samples exceed LISEC_AUG_MAX_SAMPLES = %d", n_samples, kMaxSamples);
    LISEC_CHECK_ARG(n_boxes + n_samples <= kMaxBoxes, "%d boxes + %d samples exceed LISEC_AUG_MAX_BOXES = %d", n_boxes,
                    n_samples, kMaxBoxes);
    LISEC_CHECK_ARG(n_boxes_out && point_offset && (n_boxes == 0 || boxes) && (n_objects == 0 || (db_boxes && db_offsets)) &&
                    (n_samples == 0 || (index && draws)) && (n_boxes + n_samples == 0 || boxes_all), "bad arguments");
    LISEC_LAUNCH(k_augment_sample, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream_), boxes, n_boxes, db_boxes,
                 db_offsets, n_objects, n_samples, (uint32_t)seed, (uint32_t)(seed >> 32), item, epoch, index, n_boxes_out,
                 boxes_all, point_offset, draws);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_augment_paste(const void* points, int dtype, int n, int stride, const void* db_points,
                                   const int32_t* db_offsets, const int32_t* index, const int32_t* point_offset,
                                   const double* boxes_all, int n_scene_boxes, const int32_t* n_boxes_dev, int n_samples,
                                   double pad_limit, void* points_out, int cap, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(n >= 0 && stride >= 3 && (dtype == 0 || dtype == 1) && n_scene_boxes >= 0 && n_samples >= 0 &&
                    n_samples <= kMaxSamples && pad_limit > 0 && cap >= n, "bad arguments");
    LISEC_CHECK_ARG(n_boxes_dev && point_offset && (n == 0 || points) && (cap == 0 || points_out) &&
                    (n_samples == 0 || (index && boxes_all)), "bad arguments");
    LISEC_CHECK_ARG(points_out != points || cap == 0, "the output may not alias the input");
    if (cap == 0) return LISEC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const dim3 grid(std::min(cdiv(cap, 256), 4 * cu_count()));
    if (dtype == 0)
        LISEC_LAUNCH(k_augment_paste<float>, grid, dim3(256), 0, st, static_cast<const float*>(points), n, stride,
                     static_cast<const float*>(db_points), db_offsets, index, point_offset, boxes_all, n_scene_boxes,
                     n_boxes_dev, n_samples, pad_limit, static_cast<float*>(points_out), cap);
    else
        LISEC_LAUNCH(k_augment_paste<double>, grid, dim3(256), 0, st, static_cast<const double*>(points), n, stride,
                     static_cast<const double*>(db_points), db_offsets, index, point_offset, boxes_all, n_scene_boxes,
                     n_boxes_dev, n_samples, pad_limit, static_cast<double*>(points_out), cap);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
