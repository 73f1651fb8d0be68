// ring_compact.hpp -- compacting the ROLLING obstacle map (ring.hpp) after removals (pct_cloud_ring_compact): the live rows -- below
// the window's size, no NaN coordinate -- move to slots 0 .. L-1 in arrival order, oldest first, and the table is filed again from
// them, so that the next appends fill the reclaimed slots instead of evicting live points (include/pct_engine.h, "Compacting the
// window").
//
// Arrival order is slot order from `start` on: age position p of the n rows is slot (start + p) mod cap, start = the cursor on a
// wrapped ring and 0 otherwise -- contiguous in memory except at the one wrap.  The pass is pure streaming over 1024-position tiles:
//   1. rc_count_kernel         live rows per tile (tile_rank4 of scan.hpp for the total)
//   2. scan_tile_sums_kernel   one block (scan.hpp): exclusive scan of the tile totals; DdPublish (ring_dedup.hpp) sends L to the
//                              host-mapped word the host polls -- L == n ends the call there, nothing moves
//   3. rc_scatter_kernel       flags and in-tile ranks again (12 B read per slot beat 4 B written and 4 B read of a kept rank), live
//                              rows to the scratch SoA at tile offset + rank, remap[slot] = that or PCT_NO_INDEX when the caller asks
//   4. three device copies     [0, L) of the scratch back into x, y, z: the arrays keep their addresses (captured plans hold them)
//   5. ring_refile_all         clears the table, files the L rows, sets the device-side count
// No atomics and nothing that meets across blocks inside a launch: every hand-off between the steps is a kernel boundary.
#pragma once
#include "ring_dedup.hpp"
#include "scan.hpp"

namespace pct {

constexpr int kRcTile = 1024;                     // age positions per tile (256 threads x 4)

// the window in age order: n rows, the oldest in slot `start` (start < cap, n <= cap; start != 0 only when n == cap)
struct RcWindow { uint32_t start, cap, n; };

__device__ __forceinline__ uint32_t rc_slot(const RcWindow &W, uint32_t p)
{
    const uint64_t s = (uint64_t)W.start + p;
    return (uint32_t)(s >= W.cap ? s - W.cap : s);
}

// this thread's four age positions: their slots, rows and live flags (a position past n is not live)
__device__ __forceinline__ void rc_load4(const RcWindow &W, const float *__restrict__ x, const float *__restrict__ y,
                                         const float *__restrict__ z, uint32_t first, uint32_t slot[4], float px[4], float py[4],
                                         float pz[4], uint32_t f[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        f[k] = 0u;
        if (first + k < W.n) {
            slot[k] = rc_slot(W, first + k);
            px[k] = x[slot[k]]; py[k] = y[slot[k]]; pz[k] = z[slot[k]];
            f[k] = (px[k] == px[k] && py[k] == py[k] && pz[k] == pz[k]) ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void rc_count_kernel(RcWindow W, const float *__restrict__ x, const float *__restrict__ y,
                                                       const float *__restrict__ z, uint32_t *__restrict__ tile_sum)
{
    const uint32_t first = blockIdx.x * kRcTile + threadIdx.x * 4;
    uint32_t slot[4], f[4];
    float px[4], py[4], pz[4];
    rc_load4(W, x, y, z, first, slot, px, py, pz, f);
    uint32_t total;
    tile_rank4(f, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// ox / oy / oz: the scratch SoA (at least L rows each); remap (may be null): cap words, new slot or 0xFFFFFFFF per OLD slot
__global__ __launch_bounds__(256) void rc_scatter_kernel(RcWindow W, const float *__restrict__ x, const float *__restrict__ y,
                                                         const float *__restrict__ z, const uint32_t *__restrict__ tile_off,
                                                         float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ oz,
                                                         uint32_t *__restrict__ remap)
{
    const uint32_t first = blockIdx.x * kRcTile + threadIdx.x * 4;
    uint32_t slot[4], f[4];
    float px[4], py[4], pz[4];
    rc_load4(W, x, y, z, first, slot, px, py, pz, f);
    uint32_t total;
    uint32_t run = tile_off[blockIdx.x] + tile_rank4(f, total);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (first + k >= W.n) break;
        if (f[k]) { ox[run] = px[k]; oy[run] = py[k]; oz[run] = pz[k]; }
        if (remap) remap[slot[k]] = f[k] ? run : 0xFFFFFFFFu;
        run += f[k];
    }
}

}  // namespace pct
