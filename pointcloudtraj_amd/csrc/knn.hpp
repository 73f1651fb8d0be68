// Exact k-nearest-neighbour kernels for gfx950 (pct_knn_batch*, include/pct_engine.h).
//
// Same arithmetic and the same total order as the 1-NN kernels: every distance is dist2() in fp64 on the float-widened operands,
// candidates are ordered by better() = (smaller d2, then lower index), and a row lists the k smallest points in that order.  What is
// new is the state a search carries: a SORTED LIST of up to k (d2, id) entries in LDS instead of one best pair in registers, and a
// threshold tau = the list's entry k-1 in registers.  A point that cannot enter the list costs its distance and one compare against
// tau; the few that can are inserted one at a time, the lanes that share the list shifting its tail in parallel.
//
// List layout in LDS: two arrays, d2 (8 B) and id (4 B) = 12 B per entry, one row of knn_row<KCAP>() entries per list.  Lane j of the
// owners touches entries j, j + 8, ... (cell-pruned kernel: 8 owners) or entry j (streaming kernel: 64 owners), so the lanes of one
// list always hit consecutive banks.  The 8 lists of a wave of the cell-pruned kernel are accessed at the same time; their rows are
// KCAP entries apart for KCAP = 8 and KCAP + 8 for the larger ones, which puts the rows of the 4 groups a ds_read_b64 serves
// together 16 dwords apart modulo 64 banks (8 lanes x 2 dwords each: no overlap), the rows of the 4 groups of a ds_read_b32 /
// ds_write_b32 8 dwords apart modulo 32, and the 2 groups of a ds_write_b64 16 apart modulo 32.  Insert positions differ between
// lists, so this is conflict-free for aligned positions and at most 2-way otherwise.
#pragma once

#include "kernels.hpp"

namespace pct {

constexpr int kKnnMaxK = 64;                 // PCT_KNN_MAX_K
constexpr int kKnnGroups = 256 / kCoop;      // queries per block of the cell-pruned kernel
constexpr int kKnnTile = 8;                  // wave-uniform queries per pass of the streaming kernel

template <int KCAP>
constexpr int knn_row() { return KCAP + (KCAP > 8 ? 8 : 0); }

// The lanes that share a list run in lockstep inside one wave and the LDS executes a wave's accesses in order, so all that is needed
// between one lane's store and another lane's load is that the compiler keeps them in program order.
__device__ __forceinline__ void knn_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the calling lane's group of 8 in a wave ballot
__device__ __forceinline__ uint32_t knn_group_ballot(bool pred)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);
    return (uint32_t)(m >> (threadIdx.x & 56u)) & 0xFFu;
}

__device__ __forceinline__ double knn_readlane_f64(double v, int lane)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// (cd, ci), known to the 8 lanes of a group and better than entry k - 1, enters the sorted list ld / li [0, k).  Chunks of 8 entries
// from the top down: a lane reads its entry and the one below it, then every entry the candidate beats takes its lower neighbour's
// value (or the candidate itself at the insert position).  A chunk's stores touch only its own entries and the next chunk reads below
// them, so nothing is overwritten before it has been read; the walk stops at the chunk that holds the insert position.
__device__ __forceinline__ void knn_group_insert(double *ld, uint32_t *li, int k, uint32_t sub, double cd, uint32_t ci)
{
    for (int base = (k - 1) & ~(kCoop - 1); base >= 0; base -= kCoop) {
        const int e = base + (int)sub;
        const bool mine = e < k;
        double d = 0.0, pd = 0.0;
        uint32_t i = 0, pi = 0;
        if (mine) {
            d = ld[e]; i = li[e];
            if (e > 0) { pd = ld[e - 1]; pi = li[e - 1]; }
        }
        const bool shift = mine && better(cd, ci, d, i);
        const bool from_below = shift && e > 0 && better(cd, ci, pd, pi);
        knn_lds_order();
        if (shift) { ld[e] = from_below ? pd : cd; li[e] = from_below ? pi : ci; }
        knn_lds_order();
        if (knn_group_ballot(mine && !shift)) break;
    }
}

struct KnnList {
    double *d;
    uint32_t *i;
    int k;
    double td;       // tau: entry k - 1, the same in every lane that shares the list
    uint32_t ti;
};

// [s, e) of the cell-sorted records against the group's list: 8 points per step, one per lane; the lanes whose point beats tau are
// found with a ballot and their points inserted one after the other (tau moves with every insert, hence the second compare).
__device__ __forceinline__ void knn_group_scan(const float4 *__restrict__ pts, uint32_t s, uint32_t e, uint32_t sub, double qx, double qy,
                                               double qz, KnnList &L)
{
    for (uint32_t b = s; b < e; b += kCoop) {
        const uint32_t p = b + sub;
        double d2 = __builtin_huge_val();
        uint32_t id = kNoIndex;
        if (p < e) {
            const float4 P = pts[p];
            d2 = dist2((double)P.x, (double)P.y, (double)P.z, qx, qy, qz);
            id = __float_as_uint(P.w);
        }
        uint32_t m = knn_group_ballot(d2 < __builtin_huge_val() && better(d2, id, L.td, L.ti));
        while (m) {
            const int l = __builtin_ctz(m);
            m &= m - 1;
            const double cd = __shfl(d2, l, kCoop);
            const uint32_t ci = (uint32_t)__shfl((int)id, l, kCoop);
            if (better(cd, ci, L.td, L.ti)) {
                knn_group_insert(L.d, L.i, L.k, sub, cd, ci);
                L.td = L.d[L.k - 1];
                L.ti = L.i[L.k - 1];
            }
        }
    }
}

// -------------------------------------------------------------------------------------
// Cell-pruned k-NN: EIGHT lanes per query over the cell-sorted records (as nn_grid_coop_kernel), queries in the counting-sorted
// batch order when the batch was sorted (qsorted), answers written to each query's own row.  The walk takes the query's cell, then
// the shells of Chebyshev radius 1, 2, ... around it, and stops when the list is full and tau <= cube_bound()^2 -- every point
// outside the cube is then strictly farther than entry k - 1 (the bound's slack covers the fp32 cell assignment), so neither a closer
// point nor a tie is missed -- or when the cube covers the grid.  All fp64: no fp32 screen.  A query with a NaN or infinite
// coordinate has no point at a finite distance and keeps the padded row it starts with.
// -------------------------------------------------------------------------------------
template <int KCAP>
__global__ __launch_bounds__(256) void knn_grid_kernel(GridDesc G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                       const float *__restrict__ q, uint32_t Q, int k, uint32_t index_base,
                                                       const float4 *__restrict__ qsorted, uint32_t *__restrict__ out_idx,
                                                       double *__restrict__ out_d2, WorkCounters *__restrict__ work)
{
    constexpr int ROW = knn_row<KCAP>();
    __shared__ double s_d[kKnnGroups * ROW];
    __shared__ uint32_t s_i[kKnnGroups * ROW];
    // The slot, the query fetch, the cell and the rows of a shell stay spelled out in this kernel (elsewhere: coop_slot, coop_fetch_query,
    // query_cell, shell_row_runs of kernels.hpp -- the same steps).  It sits at exactly 64 VGPRs, the last count that gives 8 waves per
    // SIMD: with the cell or the shell rows through their helpers the same instructions come out in another order at 65-69, and with the
    // slot and the fetch alone (64 VGPRs, one instruction fewer) k = 64 ran 14.36 against 14.30 ms, above every round of this form
    // (profiles/grid_walk_asm.txt part 2, profiles/grid_walk_ab.txt).
    const uint32_t sub = threadIdx.x & (kCoop - 1), group = threadIdx.x / kCoop;
    const uint32_t bslot = qsorted ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint32_t slot = bslot * kKnnGroups + group;
    if (slot >= Q) return;                            // uniform within a group; the kernel has no block-wide barrier
    uint32_t t = slot;
    float qxf, qyf, qzf;
    if (qsorted) {
        const float4 R = qsorted[slot];
        qxf = R.x; qyf = R.y; qzf = R.z; t = __float_as_uint(R.w);
    } else {
        qxf = q[3 * t]; qyf = q[3 * t + 1]; qzf = q[3 * t + 2];
    }
    KnnList L{ s_d + group * ROW, s_i + group * ROW, k, __builtin_huge_val(), kNoIndex };
    for (int e = (int)sub; e < k; e += kCoop) { L.d[e] = __builtin_huge_val(); L.i[e] = kNoIndex; }
    knn_lds_order();
    uint32_t npts = 0, nruns = 0;
    const float finf = __builtin_huge_valf();
    if (fabsf(qxf) < finf && fabsf(qyf) < finf && fabsf(qzf) < finf) {
        const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
        const int cx = cell_coord(qxf, G.ox, G.inv_h, G.gx);
        const int cy = cell_coord(qyf, G.oy, G.inv_h, G.gy);
        const int cz = cell_coord(qzf, G.oz, G.inv_h, G.gz);
        for (int r = 0;; r++) {
            // the rows of shell r (r = 0: the cell itself), walked in the same order by the whole group
            const int x0 = max(cx - r, 0), x1 = min(cx + r, G.gx - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, G.gy - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, G.gz - 1);
            for (int zz = z0; zz <= z1; zz++) {
                const bool zface = (zz == cz - r) || (zz == cz + r);
                for (int yy = y0; yy <= y1; yy++) {
                    const uint32_t row = cell_lin(G, 0, yy, zz);
                    if (zface || yy == cy - r || yy == cy + r) {
                        const uint32_t s = cell_start[row + x0], e = cell_start[row + x1 + 1];
                        npts += e - s; nruns += 1;
                        knn_group_scan(pts, s, e, sub, qx, qy, qz, L);
                    } else {
                        if (cx - r >= 0) {
                            const uint32_t s = cell_start[row + cx - r], e = cell_start[row + cx - r + 1];
                            npts += e - s; nruns += 1;
                            knn_group_scan(pts, s, e, sub, qx, qy, qz, L);
                        }
                        if (cx + r <= G.gx - 1) {
                            const uint32_t s = cell_start[row + cx + r], e = cell_start[row + cx + r + 1];
                            npts += e - s; nruns += 1;
                            knn_group_scan(pts, s, e, sub, qx, qy, qz, L);
                        }
                    }
                }
            }
            const double bound = cube_bound(G, cx, cy, cz, r, qx, qy, qz);
            if (bound == __builtin_huge_val() || (bound > 0.0 && L.td <= bound * bound)) break;
        }
    }
    knn_lds_order();
    for (int e = (int)sub; e < k; e += kCoop) {
        const double d = L.d[e];
        out_idx[(size_t)t * k + e] = reported_index(d, L.i[e], index_base);
        out_d2[(size_t)t * k + e] = d;
    }
    if (work && sub == 0) {
        WorkCounters *w = work + (blockIdx.x & (kWorkSlots - 1));
        atomicAdd(&w->points, (unsigned long long)npts);
        atomicAdd(&w->cells, (unsigned long long)nruns);
    }
}

// (cd, ci), known to the whole wave and better than entry k - 1, enters a wave's sorted list: lane e owns entry e (k <= 64)
__device__ __forceinline__ void knn_wave_insert(double *ld, uint32_t *li, int k, int lane, double cd, uint32_t ci)
{
    const bool mine = lane < k;
    double d = 0.0, pd = 0.0;
    uint32_t i = 0, pi = 0;
    if (mine) {
        d = ld[lane]; i = li[lane];
        if (lane > 0) { pd = ld[lane - 1]; pi = li[lane - 1]; }
    }
    const bool shift = mine && better(cd, ci, d, i);
    const bool from_below = shift && lane > 0 && better(cd, ci, pd, pi);
    knn_lds_order();
    if (shift) { ld[lane] = from_below ? pd : cd; li[lane] = from_below ? pi : ci; }
    knn_lds_order();
}

// the entries of a sorted list `src` (LDS or global, read by all lanes at once) that beat the wave's list enter it; a sorted source
// is done at its first entry that does not
template <typename D, typename I>
__device__ __forceinline__ void knn_wave_fold(double *ld, uint32_t *li, int k, int lane, const D *src_d, const I *src_i)
{
    double td = ld[k - 1];
    uint32_t ti = li[k - 1];
    for (int e = 0; e < k; e++) {
        const double cd = src_d[e];
        const uint32_t ci = src_i[e];
        if (!(cd < __builtin_huge_val()) || !better(cd, ci, td, ti)) break;
        knn_wave_insert(ld, li, k, lane, cd, ci);
        td = ld[k - 1];
        ti = li[k - 1];
    }
}

// -------------------------------------------------------------------------------------
// Streaming k-NN (no index): lanes own POINTS, a tile of kKnnTile queries is wave-uniform, grid = (point blocks, query tiles), so
// the cloud is read once per tile whatever k is.  Every wave keeps one sorted list per query of the tile in LDS and the thresholds
// in registers; a point costs one distance and one compare per query unless it beats a threshold, in which case the wave inserts it
// (lane e shifts entry e).  At the end the four waves' lists of a query are folded into one and written as the block's sorted
// partial list part_*[(query * nparts + block) * k ...]; knn_merge_kernel folds a query's partials.  A cloud row with a NaN or
// infinite coordinate has d2 = NaN or +inf against every query and never passes the d2 < +inf test; neither does any point against
// a query with such a coordinate, whose row stays padded.  Point index = position in x / y / z (the ring slot on a rolling map).
// -------------------------------------------------------------------------------------
template <int KCAP>
__global__ __launch_bounds__(256) void knn_stream_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                         uint32_t n, const float *__restrict__ q, int Q, int k, double *__restrict__ part_d2,
                                                         uint32_t *__restrict__ part_idx)
{
    __shared__ double s_d[4][kKnnTile][KCAP];
    __shared__ uint32_t s_i[4][kKnnTile][KCAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * kKnnTile, qcount = min(kKnnTile, Q - q0);
    double qx[kKnnTile], qy[kKnnTile], qz[kKnnTile], td[kKnnTile];
    uint32_t ti[kKnnTile];
#pragma unroll
    for (int j = 0; j < kKnnTile; j++) {
        const int qi = q0 + (j < qcount ? j : qcount - 1);
        qx[j] = (double)q[3 * qi]; qy[j] = (double)q[3 * qi + 1]; qz[j] = (double)q[3 * qi + 2];
        td[j] = __builtin_huge_val();
        ti[j] = kNoIndex;
        if (lane < k) { s_d[wave][j][lane] = __builtin_huge_val(); s_i[wave][j][lane] = kNoIndex; }
    }
    knn_lds_order();
    const uint32_t stride = gridDim.x * 256u;
    for (uint64_t base = blockIdx.x * 256u + (uint32_t)wave * 64u; base < n; base += stride) {      // wave-uniform trip count
        const uint32_t p = (uint32_t)min(base + (uint64_t)lane, (uint64_t)kNoIndex);
        const bool have = p < n;
        const double px = have ? (double)x[p] : 0.0, py = have ? (double)y[p] : 0.0, pz = have ? (double)z[p] : 0.0;
#pragma unroll
        for (int j = 0; j < kKnnTile; j++) {
            if (j >= qcount) break;
            const double d2 = dist2(px, py, pz, qx[j], qy[j], qz[j]);
            unsigned long long m = __builtin_amdgcn_ballot_w64(have && d2 < __builtin_huge_val() && better(d2, p, td[j], ti[j]));
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const double cd = knn_readlane_f64(d2, l);
                const uint32_t ci = (uint32_t)base + (uint32_t)l;
                if (better(cd, ci, td[j], ti[j])) {
                    knn_wave_insert(s_d[wave][j], s_i[wave][j], k, lane, cd, ci);
                    td[j] = s_d[wave][j][k - 1];
                    ti[j] = s_i[wave][j][k - 1];
                }
            }
        }
    }
    __syncthreads();
    for (int j = wave; j < qcount; j += 4) {          // wave (j mod 4) folds the other waves' lists of query j into its own
        for (int w = 1; w < 4; w++) knn_wave_fold(s_d[wave][j], s_i[wave][j], k, lane, s_d[(wave + w) & 3][j], s_i[(wave + w) & 3][j]);
        knn_lds_order();
        if (lane < k) {
            const size_t o = ((size_t)(q0 + j) * gridDim.x + blockIdx.x) * (size_t)k + (size_t)lane;
            part_d2[o] = s_d[wave][j][lane];
            part_idx[o] = s_i[wave][j][lane];
        }
    }
}

// one wave per query: the sorted partial lists of its `nparts` blocks folded into the final row
__global__ __launch_bounds__(64) void knn_merge_kernel(const double *__restrict__ part_d2, const uint32_t *__restrict__ part_idx, int nparts, int k,
                                                       uint32_t index_base, uint32_t *__restrict__ out_idx, double *__restrict__ out_d2)
{
    __shared__ double s_d[kKnnMaxK];
    __shared__ uint32_t s_i[kKnnMaxK];
    const int lane = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * (size_t)nparts * (size_t)k;
    if (lane < k) { s_d[lane] = part_d2[row + lane]; s_i[lane] = part_idx[row + lane]; }
    knn_lds_order();
    for (int b = 1; b < nparts; b++) knn_wave_fold(s_d, s_i, k, lane, part_d2 + row + (size_t)b * k, part_idx + row + (size_t)b * k);
    knn_lds_order();
    if (lane < k) {
        const double d = s_d[lane];
        out_idx[(size_t)blockIdx.x * k + lane] = reported_index(d, s_i[lane], index_base);
        out_d2[(size_t)blockIdx.x * k + lane] = d;
    }
}

}  // namespace pct
