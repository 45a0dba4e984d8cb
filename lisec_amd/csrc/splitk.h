// Internal: the in-kernel meeting point of the slices of one contraction -- the K slices of a 128 x 64 (64 x 64, 128 x 128)
// tile of the implicit-GEMM kernels (igemm.hip, igemm_bf16.hip), the row slices of a weight-gradient cell (wgrad.hip).
// The ONLY inter-workgroup memory-ordering protocol of the library lives in the three steps below.
#pragma once
#include "common.h"

#ifdef __HIPCC__
namespace lisec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Slices meet here.  Every slice stores its accumulators to its slab IN THE REGISTER LAYOUT
// (slab[z][slot][wave][q][lane] float4: one 1 KB line per store instruction, nothing to transpose), takes a ticket on the
// slot's arrival counter, and all but the LAST slice to arrive are done.  The last one adds the slabs in slice order
// z = 0 .. nslices-1 (so the sum does not depend on who arrived last: deterministic), leaves the counter at zero for the
// next call and goes on to the ordinary epilogue with the complete accumulators.  No combine launch, no second pass.
// Hand-off (MI355X guide, inter-workgroup visibility): write-through (sc1) slab stores, every storing wave waits for its
// stores, workgroup barrier, ONE lane's agent-scope add; the last arriver's waves load (sc1, past their L1) only after the
// barrier behind the add that told them they are last.
// a0, a1, a2: the wave's accumulators, NQ sixteen-byte pieces per lane (piece q = elements 4 (q & 3) .. of accumulator
// q >> 2; an accumulator beyond (NQ + 3) / 4 is never touched: pass any);
// off: byte offset of this lane's first piece in the buffer `rs`, the pieces of a wave are 1 KB apart.

// Step 1: store my slab.
template <int NQ>
__device__ __forceinline__ void slab_store(const f32x16& a0, const f32x16& a1, const f32x16& a2, __amdgpu_buffer_rsrc_t rs, unsigned off) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const f32x16& a = q < 4 ? a0 : (q < 8 ? a1 : a2);
        const int r = (q & 3) * 4;
        u32x4 v;
        v.x = __float_as_uint(a[r]); v.y = __float_as_uint(a[r + 1]); v.z = __float_as_uint(a[r + 2]); v.w = __float_as_uint(a[r + 3]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, off + q * 64 * 16, 0, 16);          // aux 16 = sc1
    }
}

// Step 2: take the ticket.  True for the last of the nslices workgroups to arrive, which has reset the counter.
// last_word: an LDS word of the caller's (a static __shared__ word costs some kernels a workgroup per CU, see wgrad.hip).
__device__ __forceinline__ bool slice_ticket(int* counter, int nslices, int* last_word) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        *last_word = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nslices - 1;
    __syncthreads();
    if (!*last_word) return false;
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// Step 3: the sum of the slabs of slices 0 .. nslices-1 (zstride bytes apart, off = this lane's piece in slice 0), in slice order.
// DEEP: three slabs in flight at a time (3 NQ sixteen-byte loads), added in slice order: one memory round trip per three
// slices instead of one per slice -- the combine sits on the serial chain of every K-sliced RPN layer (the two-image
// kernels: one workgroup per CU, registers to spare)
template <bool DEEP, int NQ>
__device__ __forceinline__ void slab_sum(f32x16& a0, f32x16& a1, f32x16& a2, __amdgpu_buffer_rsrc_t rs, unsigned off, unsigned zstride, int nslices) {
    f32x16 s0 = {0}, s1 = {0}, s2 = {0};
    int z = 0;
    for (; DEEP && z + 3 <= nslices; z += 3, off += 3 * zstride) {
        u32x4 v[3 * NQ];
#pragma unroll
        for (int q = 0; q < 3 * NQ; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (q / NQ) * zstride + (q % NQ) * 64 * 16, 0, 16);
#pragma unroll
        for (int q = 0; q < 3 * NQ; ++q) {
            f32x16& a = (q % NQ) < 4 ? s0 : ((q % NQ) < 8 ? s1 : s2);
            const int r = (q & 3) * 4;
            a[r] += __uint_as_float(v[q].x); a[r + 1] += __uint_as_float(v[q].y);
            a[r + 2] += __uint_as_float(v[q].z); a[r + 3] += __uint_as_float(v[q].w);
        }
    }
    for (; z < nslices; ++z, off += zstride) {
        u32x4 v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + q * 64 * 16, 0, 16);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x16& a = q < 4 ? s0 : (q < 8 ? s1 : s2);
            const int r = (q & 3) * 4;
            a[r] += __uint_as_float(v[q].x); a[r + 1] += __uint_as_float(v[q].y);
            a[r + 2] += __uint_as_float(v[q].z); a[r + 3] += __uint_as_float(v[q].w);
        }
    }
    a0 = s0;
    if (NQ > 4) a1 = s1;
    if (NQ > 8) a2 = s2;
}

// The K slices (blockIdx.z of nsplit) of one implicit-GEMM tile: the three steps over the workspace `partial`.
constexpr int kSplitCounters = 4096;             // arrival counters at the head of the workspace (ints)
constexpr int kSlabF4 = 4 * 8 * 64;              // float4 per (slice, tile, column block): 128 x 64 floats

// NQ: sixteen-byte stores per lane and slab.  8 = both accumulators of a wave (128 x 64 tile); 4 = acc0 alone (the 64 x 64
// tile: slab[z][slot][wave][q][lane] with q < 4, half the slab, stride and combine traffic); acc1 is then not touched.
// WAVES: waves per workgroup (8: the 128 x 128 tile of k_igemm_wide).
template <bool DEEP = false, int NQ = 8, int WAVES = 4>
__device__ __forceinline__ bool splitk_arrive(f32x16& acc0, f32x16& acc1, float* partial, int nsplit, int slot, int nslots,
                                              int wave, int lane) {
    __shared__ int splitk_last;
    constexpr int kSlab = WAVES * NQ * 64;       // float4 per (slice, slot): kSlabF4 for NQ = 8, WAVES = 4
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(partial + kSplitCounters, 0, (int)((size_t)nsplit * nslots * kSlab * 16),
                                                                  0x00020000);
    const unsigned lane_off = (unsigned)((wave * NQ) * 64 + lane) * 16u;
    slab_store<NQ>(acc0, acc1, acc1, rs, (unsigned)(((size_t)blockIdx.z * nslots + slot) * kSlab * 16) + lane_off);
    if (!slice_ticket(reinterpret_cast<int*>(partial) + slot, nsplit, &splitk_last)) return false;
    slab_sum<DEEP, NQ>(acc0, acc1, acc1, rs, (unsigned)((size_t)slot * kSlab * 16) + lane_off, (unsigned)((size_t)nslots * kSlab * 16), nsplit);
    return true;
}

}  // namespace
}  // namespace lisec
#endif
