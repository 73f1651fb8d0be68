// ring_outlier.hpp -- radius outlier removal on the ROLLING obstacle map (pct_cloud_ring_remove_outliers,
// pct_cloud_ring_neighbour_counts): the window judged against itself, in place, for gfx950.  The rule is the paragraph "Removing
// outliers" of include/pct_engine.h: a judged row stays iff at least m OTHER rows of the window lie within r of it.
//
// Two launches, so that the judgement cannot see the removal:
//   1. ring_outlier_judge_kernel   read-only over the bucket table.  EIGHT LANES PER JUDGED ROW, 32 rows per 256-thread block (a
//                                  block per row, as ring_count_kernel spends, is right for a tick's few hundred queries and wrong
//                                  for the 3 000 .. 300 000 rows of a frame or the 5 M of a window).  The eight lanes split every
//                                  bucket's [head, tail) records (ring_for_records, ring_search.hpp: the record loop of the radius
//                                  count, with `part` / `lanes` = this lane of eight).  The row's own
//                                  bucket comes first -- on a surface window it alone usually reaches m -- then the rest of the
//                                  ball's box (ring_ball_box: the fold and wild-axis rules stay where they are; the box never names
//                                  a bucket twice, and the own bucket is skipped by its table position when the walk meets it
//                                  again), then the overflow queue, only when it holds something and the row is still undecided.
//                                  After every non-empty bucket the group of eight sums its counts (xor 1, 2, 4: no exchange leaves
//                                  the group) and stops once the sum reaches the target; the sum is the same in all eight lanes, so
//                                  they leave together and no lane reads from a group that has gone.
//                                  Output: out[slot] = min(neighbours, target) for a judged row; the host has filled the buffer
//                                  with PCT_NO_INDEX beforehand (rows out of scope, rows that hold a NaN).
//   2. ring_remove_kernel<RoBelow> the one removal kernel (ring_remove.hpp) with the predicate "this slot's count is below m"; the
//                                  counts, the host word and the bookkeeping behind it are those of every other removal.
// The arithmetic is dist2() in fp64 on the float-widened rows, inclusive, no fp32 screen: three subtractions, three products, two
// sums and a compare beside a 16-byte read.  A record is skipped when its id is kRingDead or the judged slot itself -- exclusion is
// by slot, a coincident copy in another slot is a neighbour.
#pragma once
#include "ring_search.hpp"
#include "ring_remove.hpp"
#include "ring_compact.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr uint32_t kRoLanes = 8;                       // lanes that share one judged row
constexpr uint32_t kRoRows = 256 / kRoLanes;           // judged rows per block

// sum over the group of eight lanes this lane belongs to; every lane of the group receives it
__device__ __forceinline__ uint32_t ro_group_sum(uint32_t v)
{
    v += (uint32_t)__shfl_xor((int)v, 1, (int)kRoLanes);
    v += (uint32_t)__shfl_xor((int)v, 2, (int)kRoLanes);
    v += (uint32_t)__shfl_xor((int)v, 4, (int)kRoLanes);
    return v;
}

// this lane's share of n records starting at `head` of a queue of mask + 1 places: neighbours of (qx, qy, qz) other than `self`
__device__ __forceinline__ uint32_t ro_scan(const float4 *__restrict__ base, uint32_t head, uint32_t n, uint32_t mask, uint32_t part,
                                            uint32_t self, double qx, double qy, double qz, double r2, uint32_t &npts)
{
    uint32_t c = 0;
    ring_for_records(base, head, n, mask, part, kRoLanes, qx, qy, qz, npts, [&](double d2, uint32_t id) {
        if (id != self && d2 <= r2) c++;
    });
    return c;
}

// Judged rows: age positions [p0, W.n) of the window (rc_slot: the order a compaction uses).  r2 = r * r, r finite and >= 0;
// target >= 1.  WORK (the probe's build of the kernel, pct_set_work_counters): points = records read, cells = rows walked,
// nodes = rows that their own bucket decided.
template <bool WORK>
__global__ __launch_bounds__(256) void ring_outlier_judge_kernel(RingView V, RcWindow W, uint32_t p0, const float *__restrict__ x,
                                                                 const float *__restrict__ y, const float *__restrict__ z, double r, double r2,
                                                                 uint32_t target, uint32_t *__restrict__ out, WorkCounters *__restrict__ work)
{
    __shared__ unsigned long long s_w[8];
    const RingDesc &R = V.R;
    const uint32_t part = threadIdx.x & (kRoLanes - 1);
    const uint64_t p = (uint64_t)p0 + (uint64_t)blockIdx.x * kRoRows + (threadIdx.x / kRoLanes);
    uint32_t npts = 0, walked = 0, own = 0;
    if (p < W.n) {                                                      // everything below is uniform over the group of eight
        const uint32_t slot = rc_slot(W, (uint32_t)p);
        const float px = x[slot], py = y[slot], pz = z[slot];
        if (px == px && py == py && pz == pz) {                         // a row that holds a NaN is not judged
            uint32_t mine = 0, total = 0;
            const float finf = __builtin_huge_valf();
            // a row with an infinite coordinate: every d2 that involves it is inf or NaN, it has no neighbour (and its box would be
            // the whole table)
            if (fabsf(px) < finf && fabsf(py) < finf && fabsf(pz) < finf) {
                const double qx = (double)px, qy = (double)py, qz = (double)pz;
                const uint32_t b0 = ring_bucket_of(R, px, py, pz);
                {
                    const uint2 m = V.ht[b0];
                    const uint32_t n = m.y - m.x;
                    if (n) {
                        mine += ro_scan(V.slots + (size_t)b0 * R.K, m.x, n, R.K - 1, part, slot, qx, qy, qz, r2, npts);
                        total = ro_group_sum(mine);
                    }
                }
                if (WORK) { walked = 1; own = total >= target ? 1u : 0u; }
                if (total < target) {
                    const RingBox B = ring_ball_box(R, qx, qy, qz, r);
                    bool done = false;
                    for (int jz = 0; jz < B.nz && !done; jz++)
                        for (int jy = 0; jy < B.ny && !done; jy++)
                            for (int jx = 0; jx < B.nx; jx++) {
                                const uint32_t b = ring_lin(R, B.x0 + jx, B.y0 + jy, B.z0 + jz);
                                if (b == b0) continue;
                                const uint2 m = V.ht[b];
                                const uint32_t n = m.y - m.x;
                                if (!n) continue;
                                mine += ro_scan(V.slots + (size_t)b * R.K, m.x, n, R.K - 1, part, slot, qx, qy, qz, r2, npts);
                                total = ro_group_sum(mine);
                                if (total >= target) { done = true; break; }
                            }
                }
                if (total < target) {
                    const uint32_t oh = V.st->ovf_head, on = V.st->ovf_tail - oh;
                    if (on) {
                        mine += ro_scan(V.ovf, oh, on, R.ovf_mask, part, slot, qx, qy, qz, r2, npts);
                        total = ro_group_sum(mine);
                    }
                }
            }
            if (part == 0) out[slot] = min(total, target);
        }
    }
    if (WORK) {
        ring_add_work(work, npts, part == 0 ? walked : 0u, s_w);
        ring_add_nodes(work, part == 0 ? own : 0u);
    }
}

// the removal's predicate of ring_remove_kernel (ring_remove.hpp): counts[slot] as the judge kernel left it (PCT_NO_INDEX: not
// judged); a judged row below m neighbours is removed
struct RoBelow {
    const uint32_t *counts;
    uint32_t m;
    __device__ __forceinline__ bool operator()(uint32_t slot, float, float, float) const { return counts[slot] < m; }
};

}  // namespace pct
