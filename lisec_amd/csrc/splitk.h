// Internal: the in-kernel meeting point of the K slices of one 128 x 64 (or 64 x 64) tile, shared by the implicit-GEMM
// kernels (igemm.hip, igemm_bf16.hip).
#pragma once
#include "common.h"

#ifdef __HIPCC__
namespace lisec {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// K slices of one tile meet here (nsplit > 1).  Every slice stores its two accumulators to its slab IN THE REGISTER LAYOUT
// (slab[z][slot][wave][q][lane] float4: one 1 KB line per store instruction, nothing to transpose), takes a ticket on the
// tile's arrival counter, and all but the LAST slice to arrive are done.  The last one adds the slabs in slice order
// z = 0 .. nsplit-1 (so the sum does not depend on who arrived last: deterministic), leaves the counter at zero for the
// next call and goes on to the ordinary epilogue with the complete accumulators -- bias, gate, BatchNormalization sums and
// the sink ticket exactly as an un-sliced tile.  No combine launch, no second pass over the output.
// Hand-off (MI355X guide, inter-workgroup visibility): write-through (sc1) slab stores, every storing wave waits for its
// stores, workgroup barrier, ONE lane's agent-scope add; the last arriver's waves load (sc1, past their L1) only after the
// barrier behind the add that told them they are last.
constexpr int kSplitCounters = 4096;             // arrival counters at the head of the workspace (ints)
constexpr int kSlabF4 = 4 * 8 * 64;              // float4 per (slice, tile, column block): 128 x 64 floats

// DEEP: three slabs in flight in the last arriver's combine (the two-image kernels: one workgroup per CU, registers to spare)
// NQ: sixteen-byte stores per lane and slab.  8 = both accumulators of a wave (128 x 64 tile); 4 = acc0 alone (the 64 x 64
// tile: slab[z][slot][wave][q][lane] with q < 4, half the slab, stride and combine traffic); acc1 is then not touched.
template <bool DEEP = false, int NQ = 8>
__device__ __forceinline__ bool splitk_arrive(f32x16& acc0, f32x16& acc1, float* partial, int nsplit, int slot, int nslots,
                                              int wave, int lane) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ int splitk_last;
    int* counters = reinterpret_cast<int*>(partial);
    float* slabs = partial + kSplitCounters;
    constexpr int kSlab = 4 * NQ * 64;           // float4 per (slice, tile, column block): kSlabF4 for NQ = 8
    const size_t bytes = (size_t)nsplit * nslots * kSlab * 16;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(slabs, 0, (int)bytes, 0x00020000);
    const unsigned lane_off = (unsigned)((wave * NQ) * 64 + lane) * 16u;
    const unsigned mine = (unsigned)(((size_t)blockIdx.z * nslots + slot) * kSlab * 16) + lane_off;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const f32x16& a = q < 4 ? acc0 : acc1;
        const int r = (q & 3) * 4;
        u32x4 v;
        v.x = __float_as_uint(a[r]); v.y = __float_as_uint(a[r + 1]); v.z = __float_as_uint(a[r + 2]); v.w = __float_as_uint(a[r + 3]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, mine + q * 64 * 16, 0, 16);          // aux 16 = sc1
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        splitk_last = __hip_atomic_fetch_add(counters + slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsplit - 1;
    __syncthreads();
    if (!splitk_last) return false;
    if (threadIdx.x == 0) __hip_atomic_store(counters + slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f32x16 s0 = {0}, s1 = {0};
    const unsigned zstride = (unsigned)((size_t)nslots * kSlab * 16);
    unsigned off = (unsigned)((size_t)slot * kSlab * 16) + lane_off;
    // three slabs in flight at a time (24 sixteen-byte loads), added in slice order: one memory round trip per three slices
    // instead of one per slice -- the combine sits on the serial chain of every K-sliced RPN layer
    int z = 0;
    for (; DEEP && z + 3 <= nsplit; z += 3, off += 3 * zstride) {
        u32x4 v[3 * NQ];
#pragma unroll
        for (int q = 0; q < 3 * NQ; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (q / NQ) * zstride + (q % NQ) * 64 * 16, 0, 16);
#pragma unroll
        for (int q = 0; q < 3 * NQ; ++q) {
            f32x16& a = (q % NQ) < 4 ? s0 : s1;
            const int r = (q & 3) * 4;
            a[r] += __uint_as_float(v[q].x); a[r + 1] += __uint_as_float(v[q].y);
            a[r + 2] += __uint_as_float(v[q].z); a[r + 3] += __uint_as_float(v[q].w);
        }
    }
    for (; z < nsplit; ++z, off += zstride) {
        u32x4 v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + q * 64 * 16, 0, 16);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x16& a = q < 4 ? s0 : s1;
            const int r = (q & 3) * 4;
            a[r] += __uint_as_float(v[q].x); a[r + 1] += __uint_as_float(v[q].y);
            a[r + 2] += __uint_as_float(v[q].z); a[r + 3] += __uint_as_float(v[q].w);
        }
    }
    acc0 = s0;
    if (NQ == 8) acc1 = s1;
    return true;
}

}  // namespace
}  // namespace lisec
#endif
