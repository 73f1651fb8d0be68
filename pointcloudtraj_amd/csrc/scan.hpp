// scan.hpp -- the one block-wide exclusive prefix sum under every rank, offset and compaction step of the engine (needs the HIP
// runtime alone: voxel.hip, a translation unit of its own, includes it too).  Each wave scans with __shfl_up, the per-wave totals meet
// in LDS, each wave adds the totals of the waves before it.  Users: lidar crop, cell index (per-point-atomic build and gridbuild.hpp),
// query sort, radius-search offsets, voxel map, de-duplicating and depth appends.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pct {

// Exclusive prefix of v over the block's THREADS threads (T = uint32_t or uint64_t; THREADS = 256, 512 or 1024), and the block's total.
// ONE barrier inside and none after: the static s_wave belongs to all call sites of an instantiation, so a second call in the same
// kernel must be separated from this one by a barrier (block_scan_array has it at the end of every round).
template <typename T, int THREADS>
__device__ __forceinline__ T block_exclusive(T v, T &total)
{
    static_assert(THREADS % 64 == 0 && (sizeof(T) == 4 || sizeof(T) == 8), "whole waves of 32- or 64-bit values");
    __shared__ T s_wave[THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        T o;
        if constexpr (sizeof(T) == 8) o = (T)__shfl_up((long long)inc, off, 64);
        else o = (T)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T wave_off = 0;
    for (int w = 0; w < wave; w++) wave_off += s_wave[w];
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) total += s_wave[w];
    return wave_off + inc - v;
}

// Exclusive scan of a[0, n) in place by the whole block, THREADS values a round with the running carry in one LDS word: any n, a
// global or an LDS pointer; the caller has made a[] visible to the block.  Three barriers a round, the last one at its end, so a[]
// may be read (and the scan called again) at once.
template <typename T, int THREADS>
__device__ __forceinline__ void block_scan_array(T *a, uint32_t n, T &total)
{
    __shared__ T s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += THREADS) {
        const uint32_t i = base + threadIdx.x;
        const T v = i < n ? a[i] : (T)0;
        T chunk;
        const T ex = block_exclusive<T, THREADS>(v, chunk) + s_carry;
        if (i < n) a[i] = ex;
        __syncthreads();                              // every thread has read the carry
        if (threadIdx.x == THREADS - 1) s_carry = ex + v;
        __syncthreads();                              // ... and the next round writes s_wave again
    }
    total = s_carry;
}

// The 4-values-per-thread rank of a 1024-element tile (256 threads): exclusive prefix of this thread's first value, and the tile's
// total.  The values need not be flags (the cell index scans cell counts with it).
__device__ __forceinline__ uint32_t tile_rank4(const uint32_t f[4], uint32_t &tile_total)
{
    return block_exclusive<uint32_t, 256>(f[0] + f[1] + f[2] + f[3], tile_total);
}

// One block: exclusive scan of the tile sums in place (ntiles arbitrary); thread 0 then hands the grand total to `done`.
struct ScanDoneNothing {
    template <typename T> __device__ void operator()(T) const {}
};

template <typename T, typename DONE>
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(T *__restrict__ tile_sum, uint32_t ntiles, DONE done)
{
    T total;
    block_scan_array<T, 256>(tile_sum, ntiles, total);
    if (threadIdx.x == 0) done(total);
}

}  // namespace pct
