// Batched fixed-radius search WITH LISTS for gfx950 (pct_radius_search_batch*, include/pct_engine.h).
//
// A batch is answered in three steps, all on the caller's stream:
//   1. count   the existing radius-count batch (count_grid_coop_kernel or the streaming count), unchanged: row lengths
//   2. scan    rs_scan_tiles_kernel, scan_tile_sums_kernel<uint64_t> (scan.hpp), rs_scan_final_kernel: uint32 counts -> int64 exclusive
//              offsets of a CSR, total in entry Q; two levels (2048 counts per block, the tile sums scanned by one block that loops),
//              so Q is not limited.  The last pass also queues the rows step 3b sorts.
//   3a. fill   rs_fill_grid_kernel (8 lanes per query over the box of rows the count walked) or rs_fill_stream_kernel (lanes own
//              points, a tile of 8 queries is wave-uniform); the ball test is the count's: fp64 dist2() <= (double)r * (double)r.
//              On a rolling map: ring_count_kernel / ring_fill_kernel over the bucket table (ring_search.hpp), rows queued as for the
//              streaming fill.
//   3b. sort   rs_sort_rows_kernel: a block per queued row, bitonic network in LDS (up to kRsSortLds entries) or in place in global
//              memory (any length: a row may be the whole cloud).  (A wave per row of up to 512 entries, four rows per block and no
//              block barrier, was measured and lost: 24.0 against 16.8 ms on 1 M rows of ~250 entries -- DESIGN.md.)
// The cell-pruned fill owns its row: hits are placed with a ballot and a prefix inside the group of 8, no atomics.  Rows of up to
// kRsShort entries are collected in LDS and written in final order by a rank sort (the keys of a row are distinct: indices are), so
// only longer rows are queued.  The streaming fill places hits through a per-query cursor (one vector atomic per wave and query with
// hits), in arrival order; every row of two or more entries is queued.  Final order is a function of the keys alone -- index, or
// (d2, index) with better() -- so two runs give identical bytes whatever order the hits arrived in.
//
// Every kernel that writes the lists first reads offsets[Q] and returns when it exceeds `cap`: the device form needs no host round
// trip to stay inside the caller's buffers.  Every list store is also bounded by the row's own length.
#pragma once

#include "knn.hpp"

namespace pct {

constexpr int kRsShort = 64;          // cell-pruned fill: rows up to this length are ordered in LDS (the k-NN list's 64 entries)
constexpr int kRsScanTile = 2048;     // counts per block of the scan: 256 threads x 8
constexpr int kRsSortLds = 2048;      // entries a block sorts in LDS (24 KiB); longer rows are sorted in global memory
constexpr int kRsTile = 8;            // wave-uniform queries per block of the streaming fill

template <bool BY_DIST>
__device__ __forceinline__ bool rs_before(double da, uint32_t ia, double db, uint32_t ib)
{
    return BY_DIST ? better(da, ia, db, ib) : ia < ib;
}

__global__ __launch_bounds__(256) void rs_scan_tiles_kernel(const uint32_t *__restrict__ count, uint32_t Q, uint64_t *__restrict__ tile_sum)
{
    const uint64_t first = (uint64_t)blockIdx.x * kRsScanTile + threadIdx.x * 8u;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += first + k < Q ? count[first + k] : 0u;
    uint64_t total;
    (void)block_exclusive<uint64_t, 256>(s, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// (the tile sums become exclusive tile offsets in scan_tile_sums_kernel<uint64_t> of scan.hpp: one block, any number of tiles)

// offsets[i] = sum of count[0 .. i), offsets[Q] = the total; rows longer than sort_min are appended to queue = {n, rows...}
__global__ __launch_bounds__(256) void rs_scan_final_kernel(const uint32_t *__restrict__ count, uint32_t Q, const uint64_t *__restrict__ tile_off,
                                                            long long *__restrict__ offsets, uint32_t sort_min, uint32_t *__restrict__ queue)
{
    const uint64_t first = (uint64_t)blockIdx.x * kRsScanTile + threadIdx.x * 8u;
    uint32_t c[8];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { c[k] = first + k < Q ? count[first + k] : 0u; s += c[k]; }
    uint64_t total;
    uint64_t run = tile_off[blockIdx.x] + block_exclusive<uint64_t, 256>(s, total);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t i = first + k;
        if (i < Q) {
            offsets[i] = (long long)run;
            run += c[k];
            if (c[k] > sort_min) queue[1u + atomicAdd(queue, 1u)] = (uint32_t)i;
            if (i == (uint64_t)Q - 1) offsets[Q] = (long long)run;
        }
    }
}

// -------------------------------------------------------------------------------------
// The row writers of every fill that places its hits in arrival order (the streaming and rolling-map fills here and in
// ring_search.hpp, the three capsule fills of segment_search.hpp), and the fold of a block-per-row count.
// -------------------------------------------------------------------------------------
struct RsLists {
    uint32_t *idx;
    double *d2;
    uint32_t index_base;
    bool keep_d2;            // the caller's decision: d2 is stored (BY_DIST rows always carry their sort key)
};

// a hit's entry `pos` of the row [off0, off0 + len)
__device__ __forceinline__ void rs_store(const RsLists &L, const long long &off0, const uint32_t &len, bool hit, uint32_t pos, uint32_t id, double d2)
{
    if (hit && pos < len) {                                 // every list store is bounded by the row's own length
        L.idx[off0 + pos] = id + L.index_base;
        if (L.keep_d2) L.d2[off0 + pos] = d2;
    }
}

// A block per row: false when the lists do not fit `cap` or the row is empty (block-uniform: such a row is not walked at all),
// else the row's bounds and a zeroed cursor in LDS.
__device__ __forceinline__ bool rs_row_open(const long long *__restrict__ offsets, uint32_t Q, long long cap, size_t slot, uint32_t *s_cursor,
                                            long long &off0, uint32_t &len)
{
    if (offsets[Q] > cap) return false;
    off0 = offsets[slot];
    len = (uint32_t)(offsets[slot + 1] - off0);
    if (len == 0) return false;
    if (threadIdx.x == 0) *s_cursor = 0;
    __syncthreads();
    return true;
}

// ... where a hit takes the next place of the row from that cursor
__device__ __forceinline__ void rs_place(const RsLists &L, long long off0, uint32_t len, uint32_t *s_cursor, bool hit, uint32_t id, double d2)
{
    if (hit) rs_store(L, off0, len, true, atomicAdd(s_cursor, 1u), id, d2);
}

// Lanes own points: the hits of a wave's 64 points take a block of the row through *cursor (one atomic per wave and step with
// hits) and their places inside it from the ballot.  Wave-uniform call.
__device__ __forceinline__ void rs_wave_place(const RsLists &L, const long long &off0, const uint32_t &len, uint32_t *cursor, int lane, bool hit,
                                              uint32_t id, double d2)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    if (m) {                                                // wave-uniform
        uint32_t first = 0;
        if (lane == 0) first = atomicAdd(cursor, (uint32_t)__popcll(m));
        first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
        const uint32_t pos = first + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        rs_store(L, off0, len, hit, pos, id, d2);
    }
}

// a 256-thread block's hit count into count[slot] (s_c: 4 words of LDS)
__device__ __forceinline__ void rs_block_count(uint32_t n, uint32_t *s_c, uint32_t *__restrict__ count, size_t slot)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, kWave);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) count[slot] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

// -------------------------------------------------------------------------------------
// Cell-pruned fill: EIGHT lanes per query over the rows of the ball's bounding box -- the box (grid_ball_box, kernels.hpp) and the order
// of the batch (qsorted: the counting-sorted records, rows going back to their own query) are count_grid_coop_kernel's, and so is the test,
// so a row receives exactly offsets[t + 1] - offsets[t] hits.  A row without hits is not walked at all.  The run bounds of 8 rows
// are fetched in one trip (one per lane); the points of a run are taken 8 at a time and the hits of a step placed at
// cursor + (hits in lower lanes), the cursor advancing by the step's hit count in every lane.
// -------------------------------------------------------------------------------------
template <bool BY_DIST>
__global__ __launch_bounds__(256) void rs_fill_grid_kernel(GridDesc G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                           const float *__restrict__ q, const float *__restrict__ rad, uint32_t Q,
                                                           const float4 *__restrict__ qsorted, uint32_t index_base,
                                                           const long long *__restrict__ offsets, long long cap, uint32_t *__restrict__ out_idx,
                                                           double *__restrict__ out_d2)
{
    __shared__ double s_d[kKnnGroups * kRsShort];
    __shared__ uint32_t s_i[kKnnGroups * kRsShort];
    if (offsets[Q] > cap) return;
    const uint32_t sub = threadIdx.x & (kCoop - 1), group = threadIdx.x / kCoop;
    const uint32_t slot = coop_slot<kKnnGroups>(qsorted);
    if (slot >= Q) return;                            // uniform within a group; the kernel has no block-wide barrier
    float qxf, qyf, qzf;
    const uint32_t t = coop_fetch_query(qsorted, q, slot, qxf, qyf, qzf);
    const long long off0 = offsets[t];
    const uint32_t len = (uint32_t)(offsets[t + 1] - off0);
    if (len == 0) return;
    const bool lds_row = len <= (uint32_t)kRsShort;
    double *ld = s_d + group * kRsShort;
    uint32_t *li = s_i + group * kRsShort;
    const float rf = rad[t];
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    const double r2 = (double)rf * (double)rf;
    BallBox B;
    grid_ball_box(G, qxf, qyf, qzf, rf, B);
    const int x0 = B.x0, x1 = B.x1, y0 = B.y0, z0 = B.z0;
    const int ny = B.y1 - y0 + 1, nrows = ny * (B.z1 - z0 + 1);
    uint32_t cur = 0;
    for (int base = 0; base < nrows; base += kCoop) {
        const int k = base + (int)sub;
        uint32_t bs, be;
        row_run(G, cell_start, k < nrows, y0 + k % ny, z0 + k / ny, x0, x1, bs, be);
        const int nr = min(kCoop, nrows - base);
        for (int i = 0; i < nr; i++) {                            // uniform within the group
            const uint32_t rs = (uint32_t)__shfl((int)bs, i, kCoop), re = (uint32_t)__shfl((int)be, i, kCoop);
            for (uint32_t p0 = rs; p0 < re; p0 += kCoop) {
                const uint32_t p = p0 + sub;
                bool hit = false;
                double d2 = 0.0;
                uint32_t id = 0;
                if (p < re) {
                    const float4 P = pts[p];
                    d2 = dist2((double)P.x, (double)P.y, (double)P.z, qx, qy, qz);
                    id = __float_as_uint(P.w);
                    hit = d2 <= r2;
                }
                const uint32_t m = knn_group_ballot(hit);
                const uint32_t pos = cur + (uint32_t)__popc(m & ((1u << sub) - 1u));
                if (hit && pos < len) {
                    if (lds_row) {
                        ld[pos] = d2; li[pos] = id;
                    } else {
                        out_idx[off0 + pos] = id + index_base;
                        if (out_d2) out_d2[off0 + pos] = d2;
                    }
                }
                cur += (uint32_t)__popc(m);
            }
        }
    }
    if (!lds_row) return;                             // arrival order; queued for rs_sort_rows_kernel by the scan
    knn_lds_order();
    // rank sort: an entry's place is the number of entries before it in the final order
    for (uint32_t e = sub; e < len; e += kCoop) {
        const double d = ld[e];
        const uint32_t i = li[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < len; j++) rank += rs_before<BY_DIST>(ld[j], li[j], d, i) ? 1u : 0u;
        out_idx[off0 + rank] = i + index_base;
        if (out_d2) out_d2[off0 + rank] = d;
    }
}

// -------------------------------------------------------------------------------------
// Streaming fill (no index): lanes own POINTS, a tile of kRsTile queries is wave-uniform, grid = (point blocks, query tiles), as
// knn_stream_kernel.  The hits of a wave's 64 points for one query take a block of that query's row through cursor[query] (one atomic
// per wave, query and step with hits) and their places inside it from the ballot.  A tile whose rows are all empty returns at once.
// Point index = position in x / y / z (the ring slot on a rolling map).
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rs_fill_stream_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                             uint32_t n, const float *__restrict__ q, const float *__restrict__ rad, uint32_t Q,
                                                             uint32_t tile0, uint32_t index_base, const long long *__restrict__ offsets, long long cap,
                                                             uint32_t *__restrict__ cursor, uint32_t *__restrict__ out_idx, double *__restrict__ out_d2)
{
    if (offsets[Q] > cap) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t q0 = (tile0 + blockIdx.y) * (uint32_t)kRsTile;
    const int qcount = (int)min((uint32_t)kRsTile, Q - q0);
    if (offsets[q0 + qcount] == offsets[q0]) return;
    double qx[kRsTile], qy[kRsTile], qz[kRsTile], rr[kRsTile];
    long long off[kRsTile];
    uint32_t len[kRsTile];
#pragma unroll
    for (int j = 0; j < kRsTile; j++) {
        const uint32_t qi = q0 + (uint32_t)(j < qcount ? j : qcount - 1);
        qx[j] = (double)q[3 * qi]; qy[j] = (double)q[3 * qi + 1]; qz[j] = (double)q[3 * qi + 2];
        const double w = (double)rad[qi];
        rr[j] = w * w;
        off[j] = offsets[qi];
        len[j] = (uint32_t)(offsets[qi + 1] - off[j]);
    }
    const RsLists L{ out_idx, out_d2, index_base, out_d2 != nullptr };
    const uint32_t stride = gridDim.x * 256u;
    for (uint64_t base = blockIdx.x * 256u + (uint32_t)wave * 64u; base < n; base += stride) {      // wave-uniform trip count
        const uint32_t p = (uint32_t)min(base + (uint64_t)lane, (uint64_t)kNoIndex);
        const bool have = p < n;
        const double px = have ? (double)x[p] : 0.0, py = have ? (double)y[p] : 0.0, pz = have ? (double)z[p] : 0.0;
#pragma unroll
        for (int j = 0; j < kRsTile; j++) {
            if (j >= qcount) break;
            const double d2 = dist2(px, py, pz, qx[j], qy[j], qz[j]);
            rs_wave_place(L, off[j], len[j], &cursor[q0 + j], lane, have && d2 <= rr[j], p, d2);
        }
    }
}

// -------------------------------------------------------------------------------------
// Row sort.  One block sorts i[0, n) (and d[0, n) with it; d may be null when the key is the index alone) with the bitonic network in
// its all-ascending form: merge size k = 2, 4, ...; the first step of a merge pairs e with its mirror image inside the block of k, the
// later steps pair e with e + j.  Every compare-exchange puts the smaller key at the lower position, so the entries n .. 2^m - 1 of the
// padded problem (+inf keys) would never move: a pair whose upper position is >= n is skipped and n need not be a power of two.
// The same code runs on LDS and on global memory; __syncthreads() orders a block's global stores and loads as well.
// -------------------------------------------------------------------------------------
template <bool BY_DIST>
__device__ __forceinline__ void rs_block_bitonic(double *d, uint32_t *i, uint64_t n)
{
    uint64_t npad = 1;
    while (npad < n) npad <<= 1;
    for (uint64_t k = 2, lk = 1; k <= npad; k <<= 1, lk++) {
        for (uint64_t j = k >> 1, lj = lk - 1; j > 0; j >>= 1, lj--) {          // j = 2^lj: no integer division in the loop
            for (uint64_t t = threadIdx.x; t < (npad >> 1); t += blockDim.x) {
                const uint64_t blk = t >> lj, r = t & (j - 1);
                const uint64_t lo = blk * 2 * j + r;
                const uint64_t hi = j == (k >> 1) ? blk * k + (k - 1 - r) : lo + j;
                if (hi < n) {
                    const uint32_t il = i[lo], ih = i[hi];
                    double dl = 0.0, dh = 0.0;
                    if (d) { dl = d[lo]; dh = d[hi]; }
                    if (rs_before<BY_DIST>(dh, ih, dl, il)) {
                        i[lo] = ih; i[hi] = il;
                        if (d) { d[lo] = dh; d[hi] = dl; }
                    }
                }
            }
            __syncthreads();
        }
    }
}

// queue = {number of rows, row numbers...} (rs_scan_final_kernel); blocks take the queued rows in turn
template <bool BY_DIST>
__global__ __launch_bounds__(256) void rs_sort_rows_kernel(const uint32_t *__restrict__ queue, const long long *__restrict__ offsets, uint32_t Q,
                                                           long long cap, uint32_t *idx, double *d2)
{
    __shared__ double s_d[kRsSortLds];
    __shared__ uint32_t s_i[kRsSortLds];
    if (offsets[Q] > cap) return;
    const uint32_t nq = min(queue[0], Q);
    for (uint32_t w = blockIdx.x; w < nq; w += gridDim.x) {      // block-uniform
        const uint32_t t = queue[1u + w];
        if (t >= Q) continue;
        const long long off0 = offsets[t];
        const uint64_t len = (uint64_t)(offsets[t + 1] - off0);
        if (len <= (uint64_t)kRsSortLds) {
            for (uint32_t e = threadIdx.x; e < len; e += 256) { s_i[e] = idx[off0 + e]; s_d[e] = d2 ? d2[off0 + e] : 0.0; }
            __syncthreads();
            rs_block_bitonic<BY_DIST>(s_d, s_i, len);
            for (uint32_t e = threadIdx.x; e < len; e += 256) { idx[off0 + e] = s_i[e]; if (d2) d2[off0 + e] = s_d[e]; }
            __syncthreads();
        } else {
            rs_block_bitonic<BY_DIST>(d2 ? d2 + off0 : nullptr, idx + off0, len);
        }
    }
}

}  // namespace pct
