// segment_search.hpp -- CAPSULE SEARCH: how many rows lie within reach of a line segment, and which (pct_segment_count_batch*,
// pct_segment_search_batch*), for gfx950.
//
// The contract is the paragraph "Capsule search" of include/pct_engine.h: row i lists every row of the window that is a candidate
// of segment i under reach[i] in the sense of "Segment queries" -- d2 from seg_point_d2 (segment.hpp), d2 <= r2 with r2 from
// seg_load_r2, inclusive.  Everything is fp64 on float-widened operands, no contraction, no fp32 screen: every record that is read
// is judged by that one test, and exactness never rests on what a walk leaves out.
//
// The frame is the radius search's (rsearch.hpp): count -> scan -> fill -> sort.  The count kernels below leave the row lengths in
// the cloud's count buffer, rs_scan_tiles_kernel / scan_tile_sums_kernel / rs_scan_final_kernel turn them into CSR offsets and
// queue every row of two or more entries (sort_min = 1: all three fills place their hits in arrival order), the fill kernels walk
// exactly as the count did, and rs_sort_rows_kernel orders the queued rows by index or by (d2, index).  s does not travel through
// the sort: ss_param_kernel recomputes it afterwards from the segment and the row the entry names -- it is a function of that pair
// alone, so it is the s the fill would have carried, bit for bit.
//
// Three forms, same answers bit for bit:
//   * ss_stream_*   PCT_ALGO_STREAM, any cloud: lanes own points, a tile of kSegTile segments sits in LDS (segment_stream_kernel's
//                   shape).  Count: per-lane hit counts folded per wave, one atomic per wave and segment with hits.  Fill:
//                   rs_fill_stream_kernel's scheme (rs_wave_place, rsearch.hpp).
//   * ss_ring_*     PCT_ALGO_RING: a 256-thread block per segment, ring_segment_kernel's walk (seg_ring_walk, segment.hpp): the
//                   overflow queue exhaustively, then seg_capsule_box with seg_cell_skipped and ring_for_live_records.
//   * ss_grid_*     PCT_ALGO_GRID: a 256-thread block per segment over the cell index -- the walk this file adds (ss_grid_walk).
// The ring and grid forms are one count body and one fill body (ss_count_body, ss_fill_body) over the two walks; the fill places
// its hits through a cursor in LDS (rs_row_open / rs_place, rsearch.hpp: ring_fill_kernel's).
#pragma once
#include "segment.hpp"

#pragma clang fp contract(off)

namespace pct {

// the tile's segments into LDS: ax ay az ex ey ez L2 r2 (r2 = -1 beyond the batch: no row is a candidate)
__device__ __forceinline__ void ss_load_tile(const double *__restrict__ seg, const double *__restrict__ reach, uint32_t q0, uint32_t Q,
                                             double (*s_g)[8])
{
    if (threadIdx.x < (uint32_t)kSegTile) {
        const uint32_t q = q0 + threadIdx.x;
        SegGeom S{};
        double r2 = -1.0, bx, by, bz, ra;
        if (q < Q) r2 = seg_load_r2(seg, reach, 0.0, q, S, bx, by, bz, ra);
        double *g = s_g[threadIdx.x];
        g[0] = S.ax; g[1] = S.ay; g[2] = S.az; g[3] = S.ex; g[4] = S.ey; g[5] = S.ez; g[6] = S.L2; g[7] = r2;
    }
}

// ---- the streaming form ---------------------------------------------------------------------------------------------------------
// grid (parts, tiles): block (p, t) measures rows p * 256 + lane, + parts * 256, .. against segments (tile0 + t) * kSegTile .. and
// adds its hits to count[] (zeroed by the caller).
__global__ __launch_bounds__(256) void ss_stream_count_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                              uint32_t n, const double *__restrict__ seg, const double *__restrict__ reach,
                                                              uint32_t Q, uint32_t tile0, uint32_t *__restrict__ count)
{
    __shared__ double s_g[kSegTile][8];
    const uint32_t q0 = (tile0 + blockIdx.y) * (uint32_t)kSegTile;
    ss_load_tile(seg, reach, q0, Q, s_g);
    __syncthreads();
    uint32_t c[kSegTile];
#pragma unroll
    for (int t = 0; t < kSegTile; t++) c[t] = 0;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += step) {
        const double px = (double)x[i], py = (double)y[i], pz = (double)z[i];
#pragma unroll
        for (int t = 0; t < kSegTile; t++) {
            const SegGeom S{ s_g[t][0], s_g[t][1], s_g[t][2], s_g[t][3], s_g[t][4], s_g[t][5], s_g[t][6] };
            double d2, s;
            seg_point_d2(S, px, py, pz, d2, s);
            c[t] += d2 <= s_g[t][7] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int t = 0; t < kSegTile; t++) {
        uint32_t v = c[t];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, kWave);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&count[q0 + t], v);      // v != 0 only below Q
    }
}

// The fill: the hits of a wave's 64 points for one segment are placed by rs_wave_place through cursor[segment] (zeroed by the
// caller).  A tile whose rows are all empty returns at once.
__global__ __launch_bounds__(256) void ss_stream_fill_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                             uint32_t n, const double *__restrict__ seg, const double *__restrict__ reach,
                                                             uint32_t Q, uint32_t tile0, uint32_t index_base, const long long *__restrict__ offsets,
                                                             long long cap, uint32_t *__restrict__ cursor, uint32_t *__restrict__ out_idx,
                                                             double *__restrict__ out_d2)
{
    __shared__ double s_g[kSegTile][8];
    __shared__ long long s_off[kSegTile];
    __shared__ uint32_t s_len[kSegTile];
    if (offsets[Q] > cap) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t q0 = (tile0 + blockIdx.y) * (uint32_t)kSegTile;
    const int qcount = (int)min((uint32_t)kSegTile, Q - q0);
    if (offsets[q0 + qcount] == offsets[q0]) return;          // block-uniform
    ss_load_tile(seg, reach, q0, Q, s_g);
    if (threadIdx.x < (uint32_t)kSegTile) {
        const bool have = (int)threadIdx.x < qcount;
        const long long o = have ? offsets[q0 + threadIdx.x] : 0;
        s_off[threadIdx.x] = o;
        s_len[threadIdx.x] = have ? (uint32_t)(offsets[q0 + threadIdx.x + 1] - o) : 0u;
    }
    __syncthreads();
    const RsLists L{ out_idx, out_d2, index_base, out_d2 != nullptr };
    const uint32_t stride = gridDim.x * 256u;
    for (uint64_t base = blockIdx.x * 256u + (uint32_t)wave * 64u; base < n; base += stride) {      // wave-uniform trip count
        const uint32_t p = (uint32_t)min(base + (uint64_t)lane, (uint64_t)kNoIndex);
        const bool have = p < n;
        const double px = have ? (double)x[p] : 0.0, py = have ? (double)y[p] : 0.0, pz = have ? (double)z[p] : 0.0;
#pragma unroll
        for (int t = 0; t < kSegTile; t++) {
            if (t >= qcount) break;
            const SegGeom S{ s_g[t][0], s_g[t][1], s_g[t][2], s_g[t][3], s_g[t][4], s_g[t][5], s_g[t][6] };
            double d2, s;
            seg_point_d2(S, px, py, pz, d2, s);
            rs_wave_place(L, s_off[t], s_len[t], &cursor[q0 + t], lane, have && d2 <= s_g[t][7], p, d2);
        }
    }
}

// ---- a block per segment: one count and one fill over either index ----------------------------------------------------------------
// A walk offers every record the capsule (S, reach) can hold, once: walk(S, bx, by, bz, ra, npts, nopened, offer), with live() false
// when there is nothing to walk.  The count and the fill are the same walk and the same test twice, on the same index (same stream,
// nothing in between), so row i receives exactly its length in hits; the fill places them through a cursor in LDS (rs_place).
template <typename W>
__device__ __forceinline__ void ss_count_body(const W &walk, const double *__restrict__ seg, const double *__restrict__ reach,
                                              uint32_t *__restrict__ count, WorkCounters *__restrict__ work)
{
    __shared__ uint32_t s_c[4];
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    SegGeom S;
    double bx, by, bz, ra;
    const double r2 = seg_load_r2(seg, reach, 0.0, slot, S, bx, by, bz, ra);
    uint32_t n = 0, npts = 0, nopened = 0;
    if (walk.live() && r2 >= 0.0)                           // block-uniform
        walk(S, bx, by, bz, ra, npts, nopened, [&](double px, double py, double pz, uint32_t) {
            double d2, s;
            seg_point_d2(S, px, py, pz, d2, s);
            n += d2 <= r2 ? 1u : 0u;
        });
    rs_block_count(n, s_c, count, slot);
    if (work) ring_add_work(work, npts, nopened, s_w);
}

template <typename W>
__device__ __forceinline__ void ss_fill_body(const W &walk, const double *__restrict__ seg, const double *__restrict__ reach, uint32_t Q,
                                             uint32_t index_base, const long long *__restrict__ offsets, long long cap,
                                             uint32_t *__restrict__ out_idx, double *__restrict__ out_d2, WorkCounters *__restrict__ work)
{
    __shared__ uint32_t s_cursor;
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    long long off0;
    uint32_t len;
    if (!rs_row_open(offsets, Q, cap, slot, &s_cursor, off0, len)) return;
    SegGeom S;
    double bx, by, bz, ra;
    const double r2 = seg_load_r2(seg, reach, 0.0, slot, S, bx, by, bz, ra);       // len > 0: the reach is valid
    const RsLists L{ out_idx, out_d2, index_base, out_d2 != nullptr };
    uint32_t npts = 0, nopened = 0;
    walk(S, bx, by, bz, ra, npts, nopened, [&](double px, double py, double pz, uint32_t id) {
        double d2, s;
        seg_point_d2(S, px, py, pz, d2, s);
        rs_place(L, off0, len, &s_cursor, d2 <= r2, id, d2);
    });
    if (work) ring_add_work(work, npts, nopened, s_w);
}

// ---- the rolling-map form -------------------------------------------------------------------------------------------------------
// ring_segment_kernel's walk (seg_ring_walk, segment.hpp) with another offer
struct SsRingWalk {
    const RingView &V;
    __device__ __forceinline__ bool live() const { return V.st->count != 0; }
    template <typename F>
    __device__ __forceinline__ void operator()(const SegGeom &S, double bx, double by, double bz, double ra, uint32_t &npts, uint32_t &nbuckets,
                                               F offer) const
    {
        seg_ring_walk(V, S, bx, by, bz, ra, npts, nbuckets, offer);
    }
};

__global__ __launch_bounds__(256) void ss_ring_count_kernel(RingView V, const double *__restrict__ seg, const double *__restrict__ reach,
                                                            uint32_t *__restrict__ count, WorkCounters *__restrict__ work)
{
    ss_count_body(SsRingWalk{ V }, seg, reach, count, work);
}

__global__ __launch_bounds__(256) void ss_ring_fill_kernel(RingView V, const double *__restrict__ seg, const double *__restrict__ reach, uint32_t Q,
                                                           uint32_t index_base, const long long *__restrict__ offsets, long long cap,
                                                           uint32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                           WorkCounters *__restrict__ work)
{
    ss_fill_body(SsRingWalk{ V }, seg, reach, Q, index_base, offsets, cap, out_idx, out_d2, work);
}

// ---- the cell-index form --------------------------------------------------------------------------------------------------------
// One block per segment over the cell index (GridDesc, the cell-sorted records and cell_start).
//
// The box.  Per axis the cells of [min(a, b) - reach - pad, max(a, b) + reach + pad], the ends narrowed as the contract narrows them,
// the reach narrowed upwards, pad = h / 100 + 2^-22 (max(|a|, |b|) + |reach|) in fp32 -- grid_ball_box's rule with the LARGER end
// on both edges, and its NaN rule (an upper edge that comes out NaN opens the box to that side; a NaN lower edge falls to cell 0 in
// cell_coord) -- clamped by cell_coord.  A candidate row can only be filed inside this box.  A candidate is a row whose COMPUTED d2
// passes, and the chain rounds: c_k = fl(fl(p_k - a_k) - fl(s e_k)) differs from the exact p_k - (a_k + s e_k) by at most
// 2^-52 (|p_k - a_k| + |e_k| + |c_k|), and |p_k - a_k| <= |p_k - x_k| + |e_k| for the point x = a + s e of the segment (s in [0, 1]).
// So per axis the row lies within reach (1 + 2^-49) + 2^-50 |e_k| of [min, max]: the second term is nothing on a 40 m world and
// 3e23 for a segment from the cloud to FLT_MAX away, where every row is a candidate of reach 0 (w and e round to the same double:
// d2 == 0 by the contract's own arithmetic).  |e_k| <= 2 max(|a_k|, |b_k|), so the pad's 2^-22 max(|a|, |b|) covers that term
// 2^27 times over on BOTH edges (with |v| of the edge's own end alone the lower edge of such an axis had none of it); the rounding of
// the reach and the 2^-24 (|v| + pad) of the fp32 edge sums it covers with h / 100 to spare, and the fp32 cell assignment errs by
// less than 4e-4 cells on grids of at most 1024 cells per axis (it is also monotone in the coordinate, and the edges go through the
// same cell_coord).
//
// The per-cell skip: seg_cell_skipped's predicate and argument.  The centre of cell (cx, cy, cz) is taken from the fp64 face
// positions, o + (c + 0.5) h per axis, and the cell is skipped when dist^2(segment, centre) > (reach + h)^2, by seg_point_d2.
// Why that is conservative: the fp32 assignment floor((v - o) * inv_h) errs by 2^-24 |v - o| in the difference and by 2^-23 in the
// product and inv_h, below 2e-4 cells at 1024 cells per axis, so a row filed in the cell lies within (0.5 + 4e-4) h of the centre
// per axis and within sqrt(3) * 0.5004 h < 0.8668 h of it; the distance to a segment is 1-Lipschitz, so every row of a skipped cell is
// farther than reach + h - 0.8668 h = reach + 0.1332 h from the segment.  Under the magnitude guard below (|o| + g h, the ends'
// offsets from o and the reach all under 2^30 h) the roundings of the centre (2^-53 (|o| + g h) < 2e-7 h), of dc2, of (reach + h)^2
// and of the row's own d2 (a few ulp of distances below 2^33 h: under 1e-5 h) stay four orders of magnitude below that slack, so
// such a row fails d2 <= reach^2 and skipping its cell loses no candidate.  Outside the guard nothing is skipped.  A cell on the
// grid's border (c == 0 or c == g - 1 on any axis) stands for everything the clamp sends there -- pct_cloud_build_grid: the last
// cell may hold everything from there on -- and is never skipped; (reach + h)^2 = +inf never skips.  Exactness never rests on the
// skip: every record that is read is judged by the fp64 test.
//
// Lanes.  Each trip the block's 256 threads take 256 consecutive box positions (x fastest, so a group's eight cells are neighbours
// in cell_start): every lane judges ONE cell and fetches its run bounds, then the group of kCoop lanes scans its eight runs in turn,
// eight records at a time.  A run is one cell: neighbouring cells of an x-row are not joined (the records read are the same either
// way, and a skipped cell in between would have to be read).  The count and the fill are this walk twice, so the fill meets exactly
// the rows the count reserved room for.
struct SsGridBox {
    int x0, y0, z0, nx, ny, nz, total;
    bool skip;               // the per-cell skip applies
    double skip2;            // (reach + h)^2
};

constexpr double kSsGuardCells = 1073741824.0;      // 2^30: the magnitudes the skip's rounding argument covers, in cells

__device__ __forceinline__ void ss_grid_axis(float a, float b, float rf, float h100, float o, float inv_h, int g, int &c0, int &n)
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    const float pad = (rf + h100) + 0x1p-22f * (fmaxf(fabsf(lo), fabsf(hi)) + rf);       // both edges: the larger end, see above
    const float e0 = lo - pad, e1 = hi + pad;
    c0 = cell_coord(e0, o, inv_h, g);
    const int c1 = e1 == e1 ? cell_coord(e1, o, inv_h, g) : g - 1;
    n = max(c1 - c0 + 1, 1);
}

// S: the segment (ends already narrowed and widened: the casts back are exact); ra >= 0: its reach
__device__ __forceinline__ SsGridBox ss_grid_box(const GridDesc &G, const SegGeom &S, double bx, double by, double bz, double ra)
{
    SsGridBox B;
    float rf = (float)ra;
    if ((double)rf < ra) rf = __uint_as_float(__float_as_uint(rf) + 1u);           // the next float up (rf >= 0, finite): never below the reach
    const float h100 = 0.01f * (1.0f / G.inv_h);
    ss_grid_axis((float)S.ax, (float)bx, rf, h100, G.ox, G.inv_h, G.gx, B.x0, B.nx);
    ss_grid_axis((float)S.ay, (float)by, rf, h100, G.oy, G.inv_h, G.gy, B.y0, B.ny);
    ss_grid_axis((float)S.az, (float)bz, rf, h100, G.oz, G.inv_h, G.gz, B.z0, B.nz);
    B.total = B.nx * B.ny * B.nz;                           // at most 2^30 cells
    const double rh = ra + G.hd, lim = kSsGuardCells * G.hd;
    B.skip2 = rh * rh;
    const auto small = [&](double o, int g, double a, double b) {
        return fabs(o) + (double)g * G.hd < lim && fabs(a - o) < lim && fabs(b - o) < lim;
    };
    B.skip = ra < lim && small(G.oxd, G.gx, S.ax, bx) && small(G.oyd, G.gy, S.ay, by) && small(G.ozd, G.gz, S.az, bz);
    return B;
}

__device__ __forceinline__ bool ss_grid_cell_skipped(const GridDesc &G, const SegGeom &S, const SsGridBox &B, int cx, int cy, int cz)
{
    if (!B.skip) return false;
    if (cx == 0 || cx == G.gx - 1 || cy == 0 || cy == G.gy - 1 || cz == 0 || cz == G.gz - 1) return false;
    double dc2, sc;
    seg_point_d2(S, G.oxd + ((double)cx + 0.5) * G.hd, G.oyd + ((double)cy + 0.5) * G.hd, G.ozd + ((double)cz + 0.5) * G.hd, dc2, sc);
    return dc2 > B.skip2;
}

// every record of the box's surviving cells, once: offer(px, py, pz, id).  npts: records read; ncells: cells opened.
template <typename F>
__device__ __forceinline__ void ss_grid_walk(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                             const SegGeom &S, const SsGridBox &B, uint32_t &npts, uint32_t &ncells, F offer)
{
    const uint32_t sub = threadIdx.x & (kCoop - 1);
    const int nxy = B.nx * B.ny;
    for (int base = 0; base < B.total; base += 256) {       // block-uniform trip count
        const int k = base + (int)threadIdx.x;
        uint32_t rs = 0, re = 0;
        if (k < B.total) {
            const int jz = k / nxy, rem = k - jz * nxy, jy = rem / B.nx, jx = rem - jy * B.nx;
            const int cx = B.x0 + jx, cy = B.y0 + jy, cz = B.z0 + jz;
            if (!ss_grid_cell_skipped(G, S, B, cx, cy, cz)) {
                const uint32_t cell = cell_lin(G, cx, cy, cz);
                rs = cell_start[cell]; re = cell_start[cell + 1];
                ncells++;
            }
        }
        if (!__builtin_amdgcn_ballot_w64(re > rs)) continue;          // wave-uniform: none of the wave's 64 cells holds a record
#pragma unroll
        for (int i = 0; i < kCoop; i++) {
            const uint32_t ps = (uint32_t)__shfl((int)rs, i, kCoop), pe = (uint32_t)__shfl((int)re, i, kCoop);
            for (uint32_t p = ps + sub; p < pe; p += kCoop) {
                const float4 P = pts[p];
                npts++;
                offer((double)P.x, (double)P.y, (double)P.z, __float_as_uint(P.w));
            }
        }
    }
}

struct SsGridWalk {
    const GridDesc &G;
    const float4 *pts;
    const uint32_t *cell_start;
    __device__ __forceinline__ bool live() const { return true; }
    template <typename F>
    __device__ __forceinline__ void operator()(const SegGeom &S, double bx, double by, double bz, double ra, uint32_t &npts, uint32_t &ncells,
                                               F offer) const
    {
        const SsGridBox B = ss_grid_box(G, S, bx, by, bz, ra);
        ss_grid_walk(G, pts, cell_start, S, B, npts, ncells, offer);
    }
};

__global__ __launch_bounds__(256) void ss_grid_count_kernel(GridDesc G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                            const double *__restrict__ seg, const double *__restrict__ reach,
                                                            uint32_t *__restrict__ count, WorkCounters *__restrict__ work)
{
    ss_count_body(SsGridWalk{ G, pts, cell_start }, seg, reach, count, work);
}

__global__ __launch_bounds__(256) void ss_grid_fill_kernel(GridDesc G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                           const double *__restrict__ seg, const double *__restrict__ reach, uint32_t Q,
                                                           uint32_t index_base, const long long *__restrict__ offsets, long long cap,
                                                           uint32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                           WorkCounters *__restrict__ work)
{
    ss_fill_body(SsGridWalk{ G, pts, cell_start }, seg, reach, Q, index_base, offsets, cap, out_idx, out_d2, work);
}

// ---- s, after the sort ----------------------------------------------------------------------------------------------------------
// out_s[e] = the closest-point parameter of entry e's row on its segment: seg_point_d2 on the segment of the entry's row and the
// coordinates the reported index names (x / y / z by position: the ring slot on a rolling map).  Blocks take the rows in turn.
__global__ __launch_bounds__(256) void ss_param_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                       uint32_t n, const double *__restrict__ seg, uint32_t Q, uint32_t index_base,
                                                       const long long *__restrict__ offsets, long long cap, const uint32_t *__restrict__ idx,
                                                       double *__restrict__ out_s)
{
    if (offsets[Q] > cap) return;
    for (uint32_t row = blockIdx.x; row < Q; row += gridDim.x) {
        const long long off0 = offsets[row], off1 = offsets[row + 1];
        if (off1 == off0) continue;
        SegGeom S;
        double bx, by, bz;
        (void)seg_load(seg, row, S, bx, by, bz);
        for (long long e = off0 + threadIdx.x; e < off1; e += 256) {
            const uint32_t i = idx[e] - index_base;
            double d2, s = 0.0;
            if (i < n) seg_point_d2(S, (double)x[i], (double)y[i], (double)z[i], d2, s);
            out_s[e] = s;
        }
    }
}

}  // namespace pct
