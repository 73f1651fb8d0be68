// ring_search.hpp -- radius count, radius lists and k nearest neighbours over the ROLLING-MAP index (ring.hpp), for gfx950.
//
// The search side of the bucket table for the three query kinds that list or count points instead of naming one: PCT_ALGO_RING of
// pct_radius_count_batch*, pct_radius_search_batch* and pct_knn_batch*, and what PCT_ALGO_AUTO takes on a ring-indexed cloud.  One
// 256-thread block per query, as ring_batch_kernel: a tick's batch is a few hundred queries, each touching a few hundred records, so
// a block per query fills the machine and lets the lanes share fat buckets (`part` / `lanes` split, ring_lanes_per_bucket).
//
// The arithmetic is the engine's: dist2() in fp64 on the float-widened operands, no FMA, no fp32 screen; the order is better() =
// (d2, then ring slot); a record whose id word is kRingDead has left the window and is skipped.  A point is filed either in its
// bucket or in the overflow queue, never in both: every kernel scans the queue exhaustively ONCE per query and then visits every
// bucket that can matter.
//
// Unlike the minimum of ring_block_nn_search, a count and a list are not idempotent, so what "visits" means differs:
//   * count / fill walk the box of world cells the ball can touch, folded onto the table (ring_for_ball).  On an axis where the box
//     spans the table (or the query / radius is wild) the g table positions are visited once each instead of the span, so no
//     bucket is read twice.
//   * k-NN walks the expanding cube (ring_knn_walk over ring_shell, ring.hpp: the enumeration and its exactness argument are
//     ring_block_nn_search's), which revisits the whole box when an axis closes.  Its insert is IDEMPOTENT instead: a candidate
//     whose (d2, slot) equals an entry already in the list is dropped (ring_knn_insert).  A record that was seen before and is no
//     longer in the list was evicted by better ones, so it is still worse than tau and never gets as far as the insert.
// ring_knn_walk is also the walk of the statistical filter (ring_statistical.hpp: a wave per row instead of a block per query), and
// ring_for_records, the record loop under ring_for_ball, is the outlier judge's too (ring_outlier.hpp).
#pragma once
#include "ring.hpp"
#include "knn.hpp"
#include "rsearch.hpp"

#pragma clang fp contract(off)

namespace pct {

// per-block work of an instrumented launch -> WorkCounters (the slot scheme of knn_grid_kernel); s_w: 8 words of LDS
__device__ __forceinline__ void ring_add_work(WorkCounters *__restrict__ work, uint32_t npts, uint32_t nbuckets, unsigned long long *s_w)
{
    unsigned long long a = npts, b = nbuckets;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += (unsigned long long)__shfl_xor((long long)a, off, kWave);
        b += (unsigned long long)__shfl_xor((long long)b, off, kWave);
    }
    if ((threadIdx.x & 63) == 0) { s_w[2 * (threadIdx.x >> 6)] = a; s_w[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        WorkCounters *w = work + (blockIdx.x & (kWorkSlots - 1));
        atomicAdd(&w->points, s_w[0] + s_w[2] + s_w[4] + s_w[6]);
        atomicAdd(&w->cells, s_w[1] + s_w[3] + s_w[5] + s_w[7]);
    }
}

// the third counter of the kernels that judge rows (what `nodes` counts is theirs to say): summed per wave, one atomic for each
__device__ __forceinline__ void ring_add_nodes(WorkCounters *__restrict__ work, uint32_t nodes)
{
    unsigned long long o = nodes;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) o += (unsigned long long)__shfl_xor((long long)o, off, kWave);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(&work[blockIdx.x & (kWorkSlots - 1)].nodes, o);
}

// ---- the ball's box ---------------------------------------------------------------------------------------------------------
// Table positions a ball (q, |r|) can touch: per axis the world cells cell(q - |r|) - 1 .. cell(q + |r|) + 1.  The fp64 products
// that place a point and the two ends err by a few ulp, far less than the cell of slack on either side, and exactness comes from
// the fp64 test on every record: the box only has to be a superset.  An end that is wild (NaN, infinite, beyond the cell clamp) or
// a span that reaches the table size takes the axis' g positions once.
struct RingBox { int x0, y0, z0, nx, ny, nz; };

// the axis of a box whose ends are given: [vlo, vhi] (a ball's q - |r| .. q + |r|; a capsule's, segment.hpp)
__device__ __forceinline__ void ring_box_axis_ends(double vlo, double vhi, double inv_h, int g, int &c0, int &n)
{
    bool wild = false;
    const int lo = ring_cell_coord(vlo, inv_h, wild), hi = ring_cell_coord(vhi, inv_h, wild);
    const long long span = (long long)hi - (long long)lo + 3;
    if (wild || span >= (long long)g) { c0 = 0; n = g; }
    else { c0 = lo - 1; n = (int)span; }
}

__device__ __forceinline__ void ring_box_axis(double q, double ra, double inv_h, int g, int &c0, int &n)
{
    ring_box_axis_ends(q - ra, q + ra, inv_h, g, c0, n);
}

__device__ __forceinline__ RingBox ring_ball_box(const RingDesc &R, double qx, double qy, double qz, double ra)
{
    RingBox B;
    ring_box_axis(qx, ra, R.inv_h, R.gx, B.x0, B.nx);
    ring_box_axis(qy, ra, R.inv_h, R.gy, B.y0, B.ny);
    ring_box_axis(qz, ra, R.inv_h, R.gz, B.z0, B.nz);
    return B;
}

// The record loop: this lane's share (records part, part + lanes, ..) of the n records from `head` of a queue of mask + 1 places --
// a bucket or the overflow queue.  Every read is counted in npts, a dead record is skipped, g(x, y, z, slot) for the rest: the
// widened coordinates, for a caller that measures something other than the distance to a point (a segment: segment.hpp).
template <typename G>
__device__ __forceinline__ void ring_for_live_records(const float4 *__restrict__ base, uint32_t head, uint32_t n, uint32_t mask, uint32_t part,
                                                      uint32_t lanes, uint32_t &npts, G g)
{
    for (uint32_t j = part; j < n; j += lanes) {
        const float4 P = base[(head + j) & mask];
        const uint32_t id = __float_as_uint(P.w);
        npts++;
        if (id != kRingDead) g((double)P.x, (double)P.y, (double)P.z, id);
    }
}

// the point queries' form: f(d2, slot) with d2 = dist2 to (qx, qy, qz)
template <typename F>
__device__ __forceinline__ void ring_for_records(const float4 *__restrict__ base, uint32_t head, uint32_t n, uint32_t mask, uint32_t part,
                                                 uint32_t lanes, double qx, double qy, double qz, uint32_t &npts, F f)
{
    ring_for_live_records(base, head, n, mask, part, lanes, npts,
                          [&](double px, double py, double pz, uint32_t id) { f(dist2(px, py, pz, qx, qy, qz), id); });
}

// every live record of the overflow queue and of the box's buckets, once: f(d2, slot).  Returns through npts / nbuckets what was read.
template <typename F>
__device__ __forceinline__ void ring_for_ball(const RingView &V, double qx, double qy, double qz, double ra, uint32_t &npts, uint32_t &nbuckets, F f)
{
    const RingDesc &R = V.R;
    const uint32_t oh = V.st->ovf_head;
    ring_for_records(V.ovf, oh, V.st->ovf_tail - oh, R.ovf_mask, threadIdx.x, 256u, qx, qy, qz, npts, f);
    const RingBox B = ring_ball_box(R, qx, qy, qz, ra);
    const int total = B.nx * B.ny * B.nz;                   // at most the table: 2^24 buckets
    // grown buckets: the ball's records sit in a few fat buckets among many empty ones, so eight lanes share a bucket in larger boxes too
    const int lanes = R.K > kRingK && total <= 8192 ? 8 : ring_lanes_per_bucket(R, total);
    const uint32_t part = threadIdx.x % (uint32_t)lanes;
    for (int k = (int)threadIdx.x / lanes; k < total; k += 256 / lanes) {
        const int jx = k % B.nx, jy = (k / B.nx) % B.ny, jz = k / (B.nx * B.ny);
        const uint32_t b = ring_lin(R, B.x0 + jx, B.y0 + jy, B.z0 + jz);
        const uint2 m = V.ht[b];
        const uint32_t n = m.y - m.x;
        const float4 *base = V.slots + (size_t)b * R.K;
        if (part == 0) nbuckets++;
        ring_for_records(base, m.x, n, R.K - 1, part, (uint32_t)lanes, qx, qy, qz, npts, f);
    }
}

// ---- radius count -----------------------------------------------------------------------------------------------------------
// count[i] = live records with d2 <= (double)r * (double)r.  A NaN radius or query coordinate makes every comparison false (the
// walk is skipped: it could only find 0); r*r = +inf counts every record whose d2 is not NaN, non-finite rows included, as the
// streaming count does.
__global__ __launch_bounds__(256) void ring_count_kernel(RingView V, const float *__restrict__ q, const float *__restrict__ rad,
                                                         uint32_t *__restrict__ count, WorkCounters *__restrict__ work)
{
    __shared__ uint32_t s_c[4];
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    const double qx = (double)q[3 * slot], qy = (double)q[3 * slot + 1], qz = (double)q[3 * slot + 2];
    const double rw = (double)rad[slot], r2 = rw * rw;
    uint32_t n = 0, npts = 0, nbuckets = 0;
    if (V.st->count != 0 && r2 >= 0.0 && qx == qx && qy == qy && qz == qz)
        ring_for_ball(V, qx, qy, qz, fabs(rw), npts, nbuckets, [&](double d2, uint32_t) { n += d2 <= r2 ? 1u : 0u; });
    rs_block_count(n, s_c, count, slot);
    if (work) ring_add_work(work, npts, nbuckets, s_w);
}

// ---- radius lists: step 3a of rsearch.hpp's count -> scan -> fill -> sort ---------------------------------------------------------
// The walk and the test of ring_count_kernel, on the same table (same stream, no append in between), so row i receives exactly
// offsets[i + 1] - offsets[i] hits.  A hit takes the next place of its row from a cursor in LDS -- arrival order; every row of two
// or more entries is queued for rs_sort_rows_kernel (sort_min = 1, as for the streaming fill), which makes the order a function of
// the keys alone.  BY_DIST rows always carry their d2 (the sort key); index-ordered rows carry it when the caller asked for it.
template <bool BY_DIST>
__global__ __launch_bounds__(256) void ring_fill_kernel(RingView V, const float *__restrict__ q, const float *__restrict__ rad, uint32_t Q,
                                                        uint32_t index_base, const long long *__restrict__ offsets, long long cap,
                                                        uint32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                        WorkCounters *__restrict__ work)
{
    __shared__ uint32_t s_cursor;
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    long long off0;
    uint32_t len;
    if (!rs_row_open(offsets, Q, cap, slot, &s_cursor, off0, len)) return;
    const double qx = (double)q[3 * slot], qy = (double)q[3 * slot + 1], qz = (double)q[3 * slot + 2];
    const double rw = (double)rad[slot], r2 = rw * rw;
    const RsLists L{ out_idx, out_d2, index_base, BY_DIST || out_d2 };
    uint32_t npts = 0, nbuckets = 0;
    ring_for_ball(V, qx, qy, qz, fabs(rw), npts, nbuckets, [&](double d2, uint32_t id) { rs_place(L, off0, len, &s_cursor, d2 <= r2, id, d2); });
    if (work) ring_add_work(work, npts, nbuckets, s_w);
}

// ---- k nearest neighbours ---------------------------------------------------------------------------------------------------
// (cd, ci), known to the whole wave and better than entry k - 1, enters the wave's sorted list unless it is there already
__device__ __forceinline__ void ring_knn_insert(double *ld, uint32_t *li, int k, int lane, double cd, uint32_t ci)
{
    const bool same = lane < k && li[lane] == ci && ld[lane] == cd;
    if (__builtin_amdgcn_ballot_w64(same)) return;          // wave-uniform
    knn_wave_insert(ld, li, k, lane, cd, ci);
}

// one candidate per lane (have: this lane holds one), inserted one after the other into the wave's list; tau (td, ti) moves with
// every insert, hence the second compare.  tau is the better of the block's tau and this list's entry k - 1.
__device__ __forceinline__ void ring_knn_offer(double *ld, uint32_t *li, int k, int lane, bool have, double d2, uint32_t id, double &td, uint32_t &ti)
{
    unsigned long long m = __builtin_amdgcn_ballot_w64(have && d2 < __builtin_huge_val() && better(d2, id, td, ti));
    while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const double cd = knn_readlane_f64(d2, l);
        const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)id, l);
        if (better(cd, ci, td, ti)) {
            ring_knn_insert(ld, li, k, lane, cd, ci);
            const double nd = ld[k - 1];
            const uint32_t ni = li[k - 1];
            if (better(nd, ni, td, ti)) { td = nd; ti = ni; }
        }
    }
}

// The k-NN walk: the overflow queue exhaustively, then the expanding cube (ring_shell, ring.hpp), every live record other than
// `self` offered to this wave's sorted list (ld, li), until the list holds k entries and tau <= bound^2 (ring_open_face_bound: every
// unseen record is then strictly farther than entry k - 1) or no axis is open.  GROUP threads share the walk -- a whole number of
// waves, t = this thread's place among them -- and everything in it is uniform over the group.  lanes_of(total) = the threads that
// share one bucket of a step with `total` buckets (a power of two, at most 64).  step(td, ti) runs after the queue and the first
// cube and after every further shell, and leaves in (td, ti) the tau to go on with: the group's waves may meet there.  The lanes of
// a wave insert together, so the bucket and record loops run while ANY lane of the wave has a bucket / a record left; that is why
// the record loop is not ring_for_records.  npts / nbuckets: records read, buckets visited.
template <int GROUP, typename Lanes, typename Step>
__device__ __forceinline__ void ring_knn_walk(const RingView &V, double qx, double qy, double qz, uint32_t t, uint32_t self, double *ld,
                                              uint32_t *li, int k, uint32_t &npts, uint32_t &nbuckets, Lanes lanes_of, Step step)
{
    const RingDesc &R = V.R;
    const int lane = (int)(t & 63u);
    double td = __builtin_huge_val();
    uint32_t ti = kNoIndex;
    {   // wave-uniform trip count; beyond the end: the last entry again
        const uint32_t oh = V.st->ovf_head, on = V.st->ovf_tail - oh;
        for (uint32_t k0 = 0; k0 < on; k0 += (uint32_t)GROUP) {
            const uint32_t e = k0 + t;
            const bool have = e < on;
            const float4 P = V.ovf[(oh + (have ? e : on - 1u)) & R.ovf_mask];
            const uint32_t id = __float_as_uint(P.w);
            npts += have ? 1u : 0u;
            ring_knn_offer(ld, li, k, lane, have && id != kRingDead && id != self, dist2((double)P.x, (double)P.y, (double)P.z, qx, qy, qz), id, td, ti);
        }
    }
    bool wild = false;
    const int cx = ring_cell_coord(qx, R.inv_h, wild), cy = ring_cell_coord(qy, R.inv_h, wild), cz = ring_cell_coord(qz, R.inv_h, wild);
    for (int r = 1;; r++) {
        const RingShell S = ring_shell(R, cx, cy, cz, r, wild);
        const int lanes = lanes_of(S.total);
        const uint32_t part = t % (uint32_t)lanes;
        for (int k0 = 0; k0 < S.total; k0 += GROUP / lanes) {
            const int kb = k0 + (int)t / lanes;
            const bool live = kb < S.total;
            uint2 m = make_uint2(0u, 0u);
            uint32_t b = 0;
            if (live) { b = ring_shell_bucket(R, S, kb); m = V.ht[b]; }
            const uint32_t n = m.y - m.x;
            const float4 *base = V.slots + (size_t)b * R.K;
            if (live && part == 0) nbuckets++;
            for (uint32_t j = part; __builtin_amdgcn_ballot_w64(j < n); j += (uint32_t)lanes) {
                const bool have = j < n;
                double d2 = __builtin_huge_val();
                uint32_t id = kRingDead;
                if (have) {
                    const float4 P = base[(m.x + j) & (R.K - 1)];
                    d2 = dist2((double)P.x, (double)P.y, (double)P.z, qx, qy, qz);
                    id = __float_as_uint(P.w);
                    npts++;
                }
                ring_knn_offer(ld, li, k, lane, have && id != kRingDead && id != self, d2, id, td, ti);
            }
        }
        step(td, ti);
        double bound;
        if (!ring_open_face_bound(R, S.ox, S.oy, S.oz, cx, cy, cz, r, qx, qy, qz, bound)) break;      // every bucket has been visited
        if (bound > 0.0 && td <= bound * bound) break;              // td < +inf: the list is full
    }
}

// Row i of idx / d2 = the k best live records of query i by better().  Each of the block's four waves owns one sorted list in LDS
// (lane e owns entry e, knn_wave_insert); wave 0's is the block's list.  The block shares one ring_knn_walk; its step: wave 0 folds
// the other three lists into its own, they start empty again, and the folded tau (entry k - 1) goes back to every lane's registers
// -- a record costs its distance and one compare unless it beats tau.  The box of a step whose axis has just closed holds the
// buckets seen before: the insert drops what the list already has (top of this file), in wave 0 directly and in the fold for what
// another wave collected.
// A query with a NaN or infinite coordinate has no record at a finite d2 and keeps the padded row it starts with; so do the slots
// beyond the number of records at a finite d2.
template <int KCAP>
__global__ __launch_bounds__(256) void ring_knn_kernel(RingView V, const float *__restrict__ q, int k, uint32_t index_base,
                                                       uint32_t *__restrict__ out_idx, double *__restrict__ out_d2, WorkCounters *__restrict__ work)
{
    __shared__ double s_d[4][KCAP];
    __shared__ uint32_t s_i[4][KCAP];
    __shared__ unsigned long long s_w[8];
    __shared__ double s_tau_d;                              // the folded tau: written by wave 0 between a step's two barriers only, so
    __shared__ uint32_t s_tau_i;                            // every wave reads the same value and takes the same way out of the walk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t slot = blockIdx.x;
    const float qxf = q[3 * slot], qyf = q[3 * slot + 1], qzf = q[3 * slot + 2];
    double *ld = s_d[wave];
    uint32_t *li = s_i[wave];
    if (lane < k) { ld[lane] = __builtin_huge_val(); li[lane] = kNoIndex; }
    knn_lds_order();
    // the walk's step (it holds copies of k, lane, wave and the list pointers): the fold between two block barriers
    const auto fold = [=](double &td, uint32_t &ti) {
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < 4; w++) {
                for (int e = 0; e < k; e++) {                   // a sorted source is done at its first entry that does not beat tau
                    const double cd = s_d[w][e];
                    const uint32_t ci = s_i[w][e];
                    if (!(cd < __builtin_huge_val()) || !better(cd, ci, ld[k - 1], li[k - 1])) break;
                    ring_knn_insert(ld, li, k, lane, cd, ci);
                }
            }
            if (lane == 0) { s_tau_d = ld[k - 1]; s_tau_i = li[k - 1]; }
        }
        __syncthreads();
        td = s_tau_d;
        ti = s_tau_i;
        if (wave != 0 && lane < k) { ld[lane] = __builtin_huge_val(); li[lane] = kNoIndex; }
        knn_lds_order();
    };
    uint32_t npts = 0, nbuckets = 0;
    const float finf = __builtin_huge_valf();
    if (V.st->count != 0 && fabsf(qxf) < finf && fabsf(qyf) < finf && fabsf(qzf) < finf)            // block-uniform
        // no record is the query's own: `self` = kRingDead folds into the walk's dead-record test
        ring_knn_walk<256>(V, (double)qxf, (double)qyf, (double)qzf, threadIdx.x, kRingDead, ld, li, k, npts, nbuckets,
                           [&](int total) { return ring_lanes_per_bucket(V.R, total); }, fold);
    __syncthreads();
    if (wave == 0 && lane < k) {
        const double d = s_d[0][lane];
        out_idx[slot * (size_t)k + lane] = reported_index(d, s_i[0][lane], index_base);
        out_d2[slot * (size_t)k + lane] = d;
    }
    if (work) ring_add_work(work, npts, nbuckets, s_w);
}

}  // namespace pct
