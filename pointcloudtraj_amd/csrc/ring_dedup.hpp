// ring_dedup.hpp -- the frame filter of a de-duplicating rolling map (pct_cloud_ring_dedup): a window of UNIQUE voxels.
//
// The rolling map files every point it is given; a sensor that re-emits the same surface lattice frame after frame (the reference's
// rgbd mode, camera_sensor.cpp:160-166) fills the window with copies.  With de-dup on, an append of the frame F[0..n) keeps F[i] iff
//   * F[i] is keyless (a non-finite coordinate, or a voxel coordinate outside [-2^20, 2^20)), or
//   * no earlier point of the frame has its key (voxel_map's "first seen wins"), and no LIVE point of the window that this append
//     would NOT overwrite has it: the "doomed" slots (next + j) mod cap, j < n, are not asked -- a holder that the same append evicts
//     must not suppress its own replacement.
// key(p) = pct_voxel.h's voxel coordinate per axis, (int) round((double) p / res).  The kept points, in frame order, are then
// appended by the unchanged eviction / insert kernels of ring.hpp.  Invariant: after the append the key of every keyed point of
// the frame is in the window (the evicted slots are a subset of the doomed ones).
//
// Launches per append (all on the library's stream, behind the previous append's):
//   0. vox_table_init_kernel   clear the per-cloud key table (a power of two >= 2n)
//   1. dd_key_kernel           claim / find the key (64-bit CAS, vox_key.hpp), atomicMin of the frame position: the table ends up
//                              holding the first occurrence of every key
//   2. dd_probe_kernel         first occurrences only, 8 lanes per point: the buckets the voxel's box touches (at most 3 per axis,
//                              the cell is never smaller than res / 2), head to tail, dead and doomed records skipped, key equality
//                              on the STORED coordinates; then the overflow queue, staged through LDS 256 entries at a time, by the
//                              blocks that still have an undecided point.  Writes the kept flags.
//   3. dd_rank_kernel          rank of the kept points inside 1024-point tiles (tile_rank4 of scan.hpp), tile totals
//   4. scan_tile_sums_kernel   one block (scan.hpp): exclusive scan of the tile totals; DdPublish sends the grand total to the
//                              host-mapped word the host polls -- it needs n' before it can queue the eviction and insert launches
//   5. dd_compact_kernel       kept points, in frame order, into the packed device staging buffer the insert kernel reads
// Atomics: one CAS per key that is new to the table, one atomicMin per point that may lower the stored position (a plain read
// first: later copies of a key find a lower position already there and issue none).  Nothing else meets across blocks inside a
// launch; every hand-off between the steps is a kernel boundary.
#pragma once
#include "ring.hpp"
#include "vox_key.hpp"

namespace pct {

constexpr int kDdTile = 1024;                     // points per rank tile (256 threads x 4)
constexpr int kDdLanes = 8;                       // lanes that share one point's buckets in the window probe
constexpr int kDdPointsPerBlock = 256 / kDdLanes;

__global__ __launch_bounds__(256) void dd_key_kernel(const unsigned char *__restrict__ src, uint32_t n, uint32_t stride, double res,
                                                     unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t mask,
                                                     uint32_t *__restrict__ pslot)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int ix, iy, iz;
    uint32_t slot = pct_vox::kNoSlot;
    if (pct_vox::vox_coords<float>(src + (size_t)i * stride, res, ix, iy, iz)) {
        slot = pct_vox::vox_find_or_claim(keys, mask, pct_vox::vox_pack(ix, iy, iz));      // cannot fail: <= n keys, >= 2n slots
        if (slot != pct_vox::kNoSlot && __hip_atomic_load(&vals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&vals[slot], i);
    }
    pslot[i] = slot;
}

// the window as an append of `n_offered` points finds it: slot `slot` is doomed iff that append would overwrite it
struct DdWindow { uint32_t next, cap, n_offered; };

__device__ __forceinline__ bool dd_doomed(const DdWindow &W, uint32_t slot)
{
    const uint64_t d = slot >= W.next ? (uint64_t)slot - W.next : (uint64_t)slot + W.cap - W.next;
    return d < (uint64_t)W.n_offered;
}

// key of a filed record, kEmptyKey when it cannot hold one: dead, doomed, or keyless
__device__ __forceinline__ unsigned long long dd_record_key(const float4 &rec, const DdWindow &W, double res)
{
    const uint32_t id = __float_as_uint(rec.w);
    if (id == kRingDead || dd_doomed(W, id)) return pct_vox::kEmptyKey;
    int ix, iy, iz;
    if (!pct_vox::vox_coords<float>(reinterpret_cast<const unsigned char *>(&rec), res, ix, iy, iz)) return pct_vox::kEmptyKey;
    return pct_vox::vox_pack(ix, iy, iz);
}

// PROBE = false: the window is empty (first data on a cloud whose table does not exist yet): the in-frame rule alone
template <bool PROBE>
__global__ __launch_bounds__(256) void dd_probe_kernel(RingView V, DdWindow W, double res, uint32_t n,
                                                       const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                       const uint32_t *__restrict__ pslot, uint8_t *__restrict__ flags)
{
    __shared__ unsigned long long s_keys[256];
    const uint32_t part = threadIdx.x % kDdLanes;
    const uint32_t i = blockIdx.x * kDdPointsPerBlock + threadIdx.x / kDdLanes;
    const uint32_t slot = i < n ? pslot[i] : pct_vox::kNoSlot;
    const bool keyed = slot != pct_vox::kNoSlot;
    const bool first = keyed && vals[slot] == i;
    const unsigned long long key = first ? keys[slot] : pct_vox::kEmptyKey;
    bool found = false;
    if (PROBE) {
        const RingDesc &R = V.R;
        if (first) {
            int k[3];
            pct_vox::vox_unpack(key, k[0], k[1], k[2]);
            int lo[3], cnt[3];
            const int g[3] = { R.gx, R.gy, R.gz };
#pragma unroll
            for (int a = 0; a < 3; a++) {
                // the voxel's box on this axis, widened by a relative 1e-6: every coordinate that rounds to k lies inside, and
                // the cell coordinate is monotonic in the coordinate; a bucket too many is harmless (the decision is key equality)
                double b0 = ((double)k[a] - 0.5) * res, b1 = ((double)k[a] + 0.5) * res;
                b0 -= 1e-6 * fabs(b0); b1 += 1e-6 * fabs(b1);
                bool wild = false;
                const int c0 = ring_cell_coord(b0, R.inv_h, wild), c1 = ring_cell_coord(b1, R.inv_h, wild);
                lo[a] = c0;
                cnt[a] = (int)min((long long)c1 - (long long)c0 + 1ll, (long long)g[a]);      // never more than the table has on the axis
            }
            const int total = cnt[0] * cnt[1] * cnt[2];
            for (int t = 0; t < total; t++) {
                const int jx = t % cnt[0], jy = (t / cnt[0]) % cnt[1], jz = t / (cnt[0] * cnt[1]);
                const uint32_t b = ring_lin(R, lo[0] + jx, lo[1] + jy, lo[2] + jz);
                const uint2 m = V.ht[b];
                const uint32_t len = m.y - m.x;
                const float4 *base = V.slots + (size_t)b * R.K;
                for (uint32_t j = part; j < len; j += kDdLanes)
                    found = found || dd_record_key(base[(m.x + j) & (R.K - 1)], W, res) == key;
                // the point's 8 lanes run the same iterations together: their bits of the ballot are complete
                const unsigned long long bal = __ballot(found);
                if ((bal >> ((threadIdx.x & 63u) & ~(uint32_t)(kDdLanes - 1))) & ((1ull << kDdLanes) - 1ull)) { found = true; break; }
            }
        }
        // the overflow queue (empty unless a cell holds more records than a bucket): every entry against the block's undecided
        // points, 256 entries at a time through LDS
        const uint32_t oh = V.st->ovf_head, on = V.st->ovf_tail - oh;
        if (on != 0u && __syncthreads_or(first && !found)) {
            for (uint32_t e0 = 0; e0 < on; e0 += 256u) {
                const uint32_t e = e0 + threadIdx.x;
                s_keys[threadIdx.x] = e < on ? dd_record_key(V.ovf[(oh + e) & R.ovf_mask], W, res) : pct_vox::kEmptyKey;
                __syncthreads();
                if (first && !found)
                    for (uint32_t j = part; j < 256u; j += kDdLanes) found = found || s_keys[j] == key;
                __syncthreads();
            }
            const unsigned long long bal = __ballot(found);
            found = ((bal >> ((threadIdx.x & 63u) & ~(uint32_t)(kDdLanes - 1))) & ((1ull << kDdLanes) - 1ull)) != 0ull;
        }
    }
    if (i < n && part == 0) flags[i] = (!keyed || (first && !found)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void dd_rank_kernel(const uint8_t *__restrict__ flags, uint32_t n, uint32_t *__restrict__ rank,
                                                      uint32_t *__restrict__ tile_sum)
{
    const uint32_t first = blockIdx.x * kDdTile + threadIdx.x * 4;
    uint32_t f[4];
#pragma unroll
    for (int k = 0; k < 4; k++) f[k] = (first + k < n && flags[first + k]) ? 1u : 0u;
    uint32_t total;
    uint32_t run = tile_rank4(f, total);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (first + k < n) rank[first + k] = run;
        run += f[k];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// what thread 0 of scan_tile_sums_kernel (scan.hpp) does with the grand total of the tile scan: the total and then the sequence word
// go to host-mapped memory (host_word[1] = n', host_word[0] = seq, released at system scope: the host spins on it)
struct DdPublish {
    uint32_t *host_word;
    uint32_t seq;
    __device__ void operator()(uint32_t total) const
    {
        __hip_atomic_store(&host_word[1], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(&host_word[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
};

__global__ __launch_bounds__(256) void dd_compact_kernel(const unsigned char *__restrict__ src, uint32_t n, uint32_t stride,
                                                         const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank,
                                                         const uint32_t *__restrict__ tile_off, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const float *p = reinterpret_cast<const float *>(src + (size_t)i * stride);
    float *o = out + 3 * (size_t)(tile_off[i / kDdTile] + rank[i]);
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

}  // namespace pct
