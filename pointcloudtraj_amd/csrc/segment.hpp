// segment.hpp -- nearest obstacle point to a LINE SEGMENT (pct_segment_nn_batch*, pct_segment_inflate_batch), for gfx950.
//
// The contract is the paragraph "Segment queries" of include/pct_engine.h; seg_point_d2 below is its arithmetic, operation for
// operation, and the only place it is written.  Everything is fp64 on float-widened operands, one rounding per operation, no
// contraction, `/` correctly rounded; there is no fp32 screen.  A row is a candidate iff d2 <= r2 with r2 = min(reach * reach,
// DBL_MAX): a NaN d2 compares false, an infinite one exceeds DBL_MAX, so a candidate's d2 is finite without a test of its own.
// A query that can have no candidate (non-finite endpoint, NaN or negative reach) carries r2 = -1, which no d2 is below.
// The winner is the best candidate by better() = (d2, then index); s travels with it.
//
// Two forms, same answers bit for bit:
//   * ring_segment_kernel    PCT_ALGO_RING: a 256-thread block per segment over the rolling-map index (ring.hpp, ring_search.hpp):
//                            the overflow queue exhaustively once, then the buckets of the world cells the capsule can touch.
//   * segment_stream_kernel  PCT_ALGO_STREAM: one pass over the SoA arrays per tile of kSegTile segments, per-lane running winners,
//                            per-block partials, segment_finish_kernel folds them.  A lane meets its rows in ascending index and
//                            every fold uses better(), so the result is a function of the data alone.
#pragma once
#include "ring_search.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr int kSegTile = 8;          // segments per block of the streaming kernel
constexpr int kSegParts = 256;       // its blocks along the cloud (the s partials borrow the filter's candidate buffer: <= kCandCap)
static_assert(kSegParts <= (int)kCandCap, "the s partials live in a buffer of kCandCap entries per query");

struct SegGeom { double ax, ay, az, ex, ey, ez, L2; };

// segment `i` of seg (Q x 6 fp64: a then b): both ends narrowed to fp32 as every planner point is, then widened.  bx..bz: the
// widened b.  false: an end is not finite after the narrowing (|v| > FLT_MAX narrows to infinity)
__device__ __forceinline__ bool seg_load(const double *__restrict__ seg, size_t i, SegGeom &S, double &bx, double &by, double &bz)
{
    const float a0 = (float)seg[6 * i], a1 = (float)seg[6 * i + 1], a2 = (float)seg[6 * i + 2];
    const float b0 = (float)seg[6 * i + 3], b1 = (float)seg[6 * i + 4], b2 = (float)seg[6 * i + 5];
    S.ax = (double)a0; S.ay = (double)a1; S.az = (double)a2;
    bx = (double)b0; by = (double)b1; bz = (double)b2;
    S.ex = bx - S.ax; S.ey = by - S.ay; S.ez = bz - S.az;
    S.L2 = (S.ex * S.ex + S.ey * S.ey) + S.ez * S.ez;
    const float finf = __builtin_huge_valf();
    return fabsf(a0) < finf && fabsf(a1) < finf && fabsf(a2) < finf && fabsf(b0) < finf && fabsf(b1) < finf && fabsf(b2) < finf;
}

// the candidate bound of a reach: reach * reach held at DBL_MAX (+inf: every finite d2); -1 for a NaN or negative reach
__device__ __forceinline__ double seg_reach2(double reach)
{
    if (!(reach >= 0.0)) return -1.0;
    const double r2 = reach * reach;
    return r2 < 1.7976931348623157e308 ? r2 : 1.7976931348623157e308;
}

// THE arithmetic: squared distance of the widened row p to the segment, and the parameter of the closest point
__device__ __forceinline__ void seg_point_d2(const SegGeom &S, double px, double py, double pz, double &d2, double &s)
{
    const double w0 = px - S.ax, w1 = py - S.ay, w2 = pz - S.az;
    const double dot = (w0 * S.ex + w1 * S.ey) + w2 * S.ez;
    s = S.L2 == 0.0 ? 0.0 : dot / S.L2;
    if (!(s > 0.0)) s = 0.0;                                // also NaN
    else if (s > 1.0) s = 1.0;
    const double c0 = w0 - s * S.ex, c1 = w1 - s * S.ey, c2 = w2 - s * S.ez;
    d2 = (c0 * c0 + c1 * c1) + c2 * c2;
}

// (d, i, s) of the wave's best lane in every lane
__device__ __forceinline__ void seg_wave_best(double &d, uint32_t &i, double &s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, kWave), os = __shfl_xor(s, off, kWave);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, off, kWave);
        if (better(od, oi, d, i)) { d = od; i = oi; s = os; }
    }
}

// ---- the rolling-map form -------------------------------------------------------------------------------------------------------
// One block per segment.  The overflow queue is scanned exhaustively once; then the box of world cells of the capsule (segment,
// reach): per axis cell(min(a, b) - reach) - 1 .. cell(max(a, b) + reach) + 1, the cell of slack of ring_box_axis on either side,
// folded onto the table.  On an axis where that span reaches the table size, or an end is wild (NaN, infinite, beyond the cell
// clamp -- reach = +inf always is), the axis' g positions are taken once each, as ring_for_ball does.
//
// The per-cell skip.  With no folded axis a box position is ONE world cell, the cube [c h, (c + 1) h]^3, and it is skipped when
//     dist(segment, centre of the cube) > reach + h,          tested on squares: dc2 > (reach + h)^2, dc2 by seg_point_d2.
// Why that is conservative: a row is filed in the cell floor(p * inv_h) per axis, an fp64 product whose rounding (and that of
// inv_h, and of the centre (c + 0.5) * h) is below 2^-51 * 10^9 cells = 5e-7 h for every cell inside the clamp, so a row of the cell
// is within sqrt(3) * (h / 2 + 5e-7 h) < 0.8661 h of the centre; the distance to a segment is 1-Lipschitz, so the row is farther
// than reach + h - 0.8661 h = reach + 0.1339 h from the segment.  The slack of 0.1339 h is five orders of magnitude above the
// rounding of dc2, of (reach + h)^2 and of the row's own d2 (all a few ulp of quantities below 10^9 h), so such a row fails
// d2 <= reach^2: skipping its cell loses no candidate.  (reach + h)^2 = +inf never skips.  Exactness never rests on the skip:
// every record that is read is judged by the fp64 test.  On a folded axis a bucket stands for several world cells and the skip is
// dropped for the whole query.  A bucket read twice would be harmless (the minimum is idempotent; s is a function of the record),
// but the box visits every position once.
__global__ __launch_bounds__(256) void ring_segment_kernel(RingView V, const double *__restrict__ seg, const double *__restrict__ reach,
                                                           double reach_all, uint32_t index_base, uint32_t *__restrict__ out_idx,
                                                           double *__restrict__ out_d2, double *__restrict__ out_s,
                                                           WorkCounters *__restrict__ work)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    const RingDesc &R = V.R;
    SegGeom S;
    double bx, by, bz;
    const bool finite = seg_load(seg, slot, S, bx, by, bz);
    const double ra = reach ? reach[slot] : reach_all;
    const double r2 = finite ? seg_reach2(ra) : -1.0;
    double bd = __builtin_huge_val(), bs = __builtin_nan("");
    uint32_t bi = kNoIndex, npts = 0, nbuckets = 0;
    const auto offer = [&](double px, double py, double pz, uint32_t id) {
        double d2, s;
        seg_point_d2(S, px, py, pz, d2, s);
        if (d2 <= r2 && better(d2, id, bd, bi)) { bd = d2; bi = id; bs = s; }
    };
    if (V.st->count != 0 && r2 >= 0.0) {                    // block-uniform
        const uint32_t oh = V.st->ovf_head;
        ring_for_live_records(V.ovf, oh, V.st->ovf_tail - oh, R.ovf_mask, threadIdx.x, 256u, npts, offer);
        RingBox B;
        ring_box_axis_ends(fmin(S.ax, bx) - ra, fmax(S.ax, bx) + ra, R.inv_h, R.gx, B.x0, B.nx);
        ring_box_axis_ends(fmin(S.ay, by) - ra, fmax(S.ay, by) + ra, R.inv_h, R.gy, B.y0, B.ny);
        ring_box_axis_ends(fmin(S.az, bz) - ra, fmax(S.az, bz) + ra, R.inv_h, R.gz, B.z0, B.nz);
        const bool folded = B.nx == R.gx || B.ny == R.gy || B.nz == R.gz;      // an unfolded axis has fewer than g positions
        const double rh = ra + R.h, skip2 = rh * rh;
        const int total = B.nx * B.ny * B.nz;               // at most the table: 2^24 buckets
        // grown buckets: the skip leaves a fraction of a capsule's box, and what it leaves are fat buckets among empty ones -- eight lanes
        // share a bucket in boxes eight times as large as a ball's (ring_for_ball), whose every cell is read
        const int lanes = R.K > kRingK && total <= 65536 ? 8 : ring_lanes_per_bucket(R, total);
        const uint32_t part = threadIdx.x % (uint32_t)lanes;
        for (int k = (int)threadIdx.x / lanes; k < total; k += 256 / lanes) {
            const int jx = k % B.nx, jy = (k / B.nx) % B.ny, jz = k / (B.nx * B.ny);
            if (!folded) {                                  // the same answer in every lane that shares the bucket
                double dc2, sc;
                seg_point_d2(S, ((double)(B.x0 + jx) + 0.5) * R.h, ((double)(B.y0 + jy) + 0.5) * R.h, ((double)(B.z0 + jz) + 0.5) * R.h, dc2, sc);
                if (dc2 > skip2) continue;
            }
            const uint32_t b = ring_lin(R, B.x0 + jx, B.y0 + jy, B.z0 + jz);
            const uint2 m = V.ht[b];
            if (part == 0) nbuckets++;
            ring_for_live_records(V.slots + (size_t)b * R.K, m.x, m.y - m.x, R.K - 1, part, (uint32_t)lanes, npts, offer);
        }
    }
    const double md = bd;
    const uint32_t mi = bi;
    block_argmin256(bd, bi, s_d, s_i);
    // a thread that holds the winner hands out its s (two threads can hold the same record only with the same s)
    if (out_s && bi != kNoIndex && mi == bi && md == bd) out_s[slot] = bs;
    if (threadIdx.x == 0) {
        out_idx[slot] = reported_index(bd, bi, index_base);
        if (out_d2) out_d2[slot] = bd;
        if (out_s && bi == kNoIndex) out_s[slot] = __builtin_nan("");
    }
    if (work) ring_add_work(work, npts, nbuckets, s_w);
}

// ---- the streaming form ---------------------------------------------------------------------------------------------------------
// grid (parts, tiles): block (p, t) measures rows p * 256 + lane, + parts * 256, .. against segments t * kSegTile .. of the slice
// and writes one partial winner per segment: part_*[q * parts + p] for the slice's segment q.
__global__ __launch_bounds__(256) void segment_stream_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                             uint32_t n, const double *__restrict__ seg, const double *__restrict__ reach,
                                                             double reach_all, uint32_t Q, double *__restrict__ part_d2,
                                                             uint32_t *__restrict__ part_idx, double *__restrict__ part_s)
{
    __shared__ double s_g[kSegTile][8];                     // ax ay az ex ey ez L2 r2
    __shared__ double s_rd[4][kSegTile], s_rs[4][kSegTile];
    __shared__ uint32_t s_ri[4][kSegTile];
    const uint32_t q0 = blockIdx.y * (uint32_t)kSegTile;
    if (threadIdx.x < (uint32_t)kSegTile) {
        const uint32_t q = q0 + threadIdx.x;
        SegGeom S{};
        double r2 = -1.0, bx, by, bz;
        if (q < Q) {
            const bool finite = seg_load(seg, q, S, bx, by, bz);
            r2 = finite ? seg_reach2(reach ? reach[q] : reach_all) : -1.0;
        }
        double *g = s_g[threadIdx.x];
        g[0] = S.ax; g[1] = S.ay; g[2] = S.az; g[3] = S.ex; g[4] = S.ey; g[5] = S.ez; g[6] = S.L2; g[7] = r2;
    }
    __syncthreads();
    double bd[kSegTile], bs[kSegTile];
    uint32_t bi[kSegTile];
#pragma unroll
    for (int t = 0; t < kSegTile; t++) { bd[t] = __builtin_huge_val(); bs[t] = __builtin_nan(""); bi[t] = kNoIndex; }
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += step) {
        const double px = (double)x[i], py = (double)y[i], pz = (double)z[i];
#pragma unroll
        for (int t = 0; t < kSegTile; t++) {
            const SegGeom S{ s_g[t][0], s_g[t][1], s_g[t][2], s_g[t][3], s_g[t][4], s_g[t][5], s_g[t][6] };
            double d2, s;
            seg_point_d2(S, px, py, pz, d2, s);
            if (d2 <= s_g[t][7] && d2 < bd[t]) { bd[t] = d2; bi[t] = (uint32_t)i; bs[t] = s; }     // ascending i: the first of equals stays
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < kSegTile; t++) {
        seg_wave_best(bd[t], bi[t], bs[t]);
        if (lane == 0) { s_rd[wave][t] = bd[t]; s_ri[wave][t] = bi[t]; s_rs[wave][t] = bs[t]; }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSegTile && q0 + threadIdx.x < Q) {
        const int t = (int)threadIdx.x;
        double d = s_rd[0][t], s = s_rs[0][t];
        uint32_t i = s_ri[0][t];
        for (int w = 1; w < 4; w++)
            if (better(s_rd[w][t], s_ri[w][t], d, i)) { d = s_rd[w][t]; i = s_ri[w][t]; s = s_rs[w][t]; }
        const size_t o = (size_t)(q0 + threadIdx.x) * gridDim.x + blockIdx.x;
        part_d2[o] = d; part_idx[o] = i; part_s[o] = s;
    }
}

// one wave per segment folds its `parts` partial winners; d2 / s may be NULL
__global__ __launch_bounds__(64) void segment_finish_kernel(const double *__restrict__ part_d2, const uint32_t *__restrict__ part_idx,
                                                            const double *__restrict__ part_s, uint32_t parts, uint32_t index_base,
                                                            uint32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_s)
{
    const size_t q = blockIdx.x;
    double d = __builtin_huge_val(), s = __builtin_nan("");
    uint32_t i = kNoIndex;
    for (uint32_t p = threadIdx.x; p < parts; p += 64) {
        const size_t o = q * parts + p;
        if (better(part_d2[o], part_idx[o], d, i)) { d = part_d2[o]; i = part_idx[o]; s = part_s[o]; }
    }
    seg_wave_best(d, i, s);
    if (threadIdx.x == 0) {
        out_idx[q] = reported_index(d, i, index_base);
        if (out_d2) out_d2[q] = d;
        if (out_s) out_s[q] = i == kNoIndex ? __builtin_nan("") : s;
    }
}

// "no candidate" for every segment (an empty cloud)
__global__ __launch_bounds__(256) void segment_fill_none_kernel(uint32_t *__restrict__ idx, double *__restrict__ d2, double *__restrict__ s, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    idx[i] = kNoIndex;
    if (d2) d2[i] = __builtin_huge_val();
    if (s) s[i] = __builtin_nan("");
}

// ---- capsule inflation ----------------------------------------------------------------------------------------------------------
// radius = min(sqrt(d2*) - search_margin, max_radius) from the winner the search left in (idx, d2, s); a radius that reaches
// max_radius names no point.  empty: the cloud holds no row -- the engine's empty-cloud rule, nothing is read.
__global__ __launch_bounds__(256) void segment_inflate_epilogue_kernel(InflateParams P, uint32_t Q, int empty, uint32_t *__restrict__ idx,
                                                                       const double *__restrict__ d2, double *__restrict__ s,
                                                                       double *__restrict__ radius)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    if (empty) { radius[i] = P.max_radius - P.search_margin; idx[i] = kNoIndex; s[i] = __builtin_nan(""); return; }
    const double rr = sqrt(d2[i]) - P.search_margin;
    if (rr < P.max_radius) { radius[i] = rr; return; }
    radius[i] = P.max_radius;
    idx[i] = kNoIndex;
    s[i] = __builtin_nan("");
}

}  // namespace pct
