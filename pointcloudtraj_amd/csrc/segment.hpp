// segment.hpp -- nearest obstacle point to a LINE SEGMENT (pct_segment_nn_batch*, pct_segment_inflate_batch) and the first contact of
// a sphere swept along one (pct_segment_sweep_batch*), for gfx950.
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
//
// Segment sweeps (paragraph "Segment sweeps" of the header) put another measure on the same rows: seg_entry_t, the parameter at which
// a sphere of radius r moving from a to b first touches the row, on top of the same w, dot, s and d2; a row blocks iff it is a
// candidate under reach = r.  The streaming kernels take the measure as a template parameter (SWEEP: the value is t, there is no s);
// the rolling-map form is ring_sweep_kernel, which shares the capsule's box and the per-cell skip with ring_segment_kernel
// (seg_capsule_box, seg_cell_skipped) and walks the box along the segment so that it can stop.
#pragma once
#include "bernstein.hpp"
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

// segment `i` with its reach (reach[i], or reach_all when reach is NULL): the geometry, the reach in ra, and the candidate bound r2 --
// -1 when nothing can be a candidate (an end that is not finite, a NaN or negative reach).  The one place that is decided, for the
// segment queries and for the sweeps, whose "invalid sweep" it is.
__device__ __forceinline__ double seg_load_r2(const double *__restrict__ seg, const double *__restrict__ reach, double reach_all, size_t i,
                                              SegGeom &S, double &bx, double &by, double &bz, double &ra)
{
    const bool finite = seg_load(seg, i, S, bx, by, bz);
    ra = reach ? reach[i] : reach_all;
    return finite ? seg_reach2(ra) : -1.0;
}

// THE arithmetic: squared distance of the widened row p to the segment, and the parameter of the closest point; dot and ww = |w|^2
// as well, for the sweep's entry parameter (seg_entry_t)
__device__ __forceinline__ void seg_point_terms(const SegGeom &S, double px, double py, double pz, double &d2, double &s, double &dot, double &ww)
{
    const double w0 = px - S.ax, w1 = py - S.ay, w2 = pz - S.az;
    dot = (w0 * S.ex + w1 * S.ey) + w2 * S.ez;
    s = S.L2 == 0.0 ? 0.0 : dot / S.L2;
    if (!(s > 0.0)) s = 0.0;                                // also NaN
    else if (s > 1.0) s = 1.0;
    const double c0 = w0 - s * S.ex, c1 = w1 - s * S.ey, c2 = w2 - s * S.ez;
    d2 = (c0 * c0 + c1 * c1) + c2 * c2;
    ww = (w0 * w0 + w1 * w1) + w2 * w2;
}

__device__ __forceinline__ void seg_point_d2(const SegGeom &S, double px, double py, double pz, double &d2, double &s)
{
    double dot, ww;
    seg_point_terms(S, px, py, pz, d2, s, dot, ww);
}

// The sweep's measure ("Segment sweeps"): is the row a blocker of the sphere (segment, r) -- d2 <= r2, the candidate test under
// reach = r -- and if so the parameter t in [0, s] at which the sphere first touches it.  ww <= r2: in contact at the start (this
// covers L2 == 0, where d2 == ww).  Otherwise the smaller root of |w - t e|^2 = r2, held into [0, s]: the entry never lies behind
// the closest approach, and only rounding can ask for the clamp.
__device__ __forceinline__ bool seg_entry_t(const SegGeom &S, double r2, double px, double py, double pz, double &t)
{
    double d2, s, dot, ww;
    seg_point_terms(S, px, py, pz, d2, s, dot, ww);
    if (!(d2 <= r2)) return false;
    if (ww <= r2) { t = 0.0; return true; }
    const double g = ww - r2;
    double disc = dot * dot - S.L2 * g;
    if (!(disc > 0.0)) disc = 0.0;
    t = (dot - sqrt(disc)) / S.L2;
    if (!(t > 0.0)) t = 0.0;
    else if (t > s) t = s;
    return true;
}

// r2 of sweep i, -1 for an invalid one
__device__ __forceinline__ double sweep_r2(const double *__restrict__ seg, const double *__restrict__ radius, size_t i)
{
    SegGeom S;
    double bx, by, bz, ra;
    return seg_load_r2(seg, radius, 0.0, i, S, bx, by, bz, ra);
}

// what a sweep reports when nothing blocks it: the whole segment can be flown (t = 1) -- or NaN for an invalid sweep (a non-finite
// end, a NaN or negative radius: r2 = -1), never "free"
__device__ __forceinline__ double sweep_unblocked_t(double r2) { return r2 >= 0.0 ? 1.0 : __builtin_nan(""); }

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
struct SegBox {
    RingBox B;
    int total, lanes;        // positions of the box (at most the table: 2^24 buckets); threads that share one bucket
    bool folded;             // an axis takes its g positions: a bucket stands for several world cells, no skip
    double skip2;            // (reach + h)^2
};

__device__ __forceinline__ SegBox seg_capsule_box(const RingDesc &R, const SegGeom &S, double bx, double by, double bz, double ra)
{
    SegBox C;
    ring_box_axis_ends(fmin(S.ax, bx) - ra, fmax(S.ax, bx) + ra, R.inv_h, R.gx, C.B.x0, C.B.nx);
    ring_box_axis_ends(fmin(S.ay, by) - ra, fmax(S.ay, by) + ra, R.inv_h, R.gy, C.B.y0, C.B.ny);
    ring_box_axis_ends(fmin(S.az, bz) - ra, fmax(S.az, bz) + ra, R.inv_h, R.gz, C.B.z0, C.B.nz);
    C.folded = C.B.nx == R.gx || C.B.ny == R.gy || C.B.nz == R.gz;             // an unfolded axis has fewer than g positions
    const double rh = ra + R.h;
    C.skip2 = rh * rh;
    C.total = C.B.nx * C.B.ny * C.B.nz;
    // grown buckets: the skip leaves a fraction of a capsule's box, and what it leaves are fat buckets among empty ones -- eight lanes
    // share a bucket in boxes eight times as large as a ball's (ring_for_ball), whose every cell is read
    C.lanes = R.K > kRingK && C.total <= 65536 ? 8 : ring_lanes_per_bucket(R, C.total);
    return C;
}

// the per-cell skip of box position (jx, jy, jz): the same answer in every lane that shares the bucket
__device__ __forceinline__ bool seg_cell_skipped(const RingDesc &R, const SegGeom &S, const SegBox &C, int jx, int jy, int jz)
{
    if (C.folded) return false;
    double dc2, sc;
    seg_point_d2(S, ((double)(C.B.x0 + jx) + 0.5) * R.h, ((double)(C.B.y0 + jy) + 0.5) * R.h, ((double)(C.B.z0 + jz) + 0.5) * R.h, dc2, sc);
    return dc2 > C.skip2;
}

// One position (jx, jy, jz) of the capsule's box: unless the skip drops it, this lane's share (part of C.lanes) of its bucket.
template <typename F>
__device__ __forceinline__ void seg_ring_visit(const RingView &V, const SegGeom &S, const SegBox &C, int jx, int jy, int jz, uint32_t part,
                                               uint32_t &npts, uint32_t &nbuckets, F offer)
{
    const RingDesc &R = V.R;
    if (seg_cell_skipped(R, S, C, jx, jy, jz)) return;
    const uint32_t b = ring_lin(R, C.B.x0 + jx, C.B.y0 + jy, C.B.z0 + jz);
    const uint2 m = V.ht[b];
    if (part == 0) nbuckets++;
    ring_for_live_records(V.slots + (size_t)b * R.K, m.x, m.y - m.x, R.K - 1, part, (uint32_t)C.lanes, npts, offer);
}

// The capsule walk of a 256-thread block on the rolling map: every live record of the overflow queue, then of the capsule's box,
// once -- offer(px, py, pz, slot).  The box visits every position once, so a count is as safe there as a minimum.
template <typename F>
__device__ __forceinline__ void seg_ring_walk(const RingView &V, const SegGeom &S, double bx, double by, double bz, double ra, uint32_t &npts,
                                              uint32_t &nbuckets, F offer)
{
    const RingDesc &R = V.R;
    const uint32_t oh = V.st->ovf_head;
    ring_for_live_records(V.ovf, oh, V.st->ovf_tail - oh, R.ovf_mask, threadIdx.x, 256u, npts, offer);
    const SegBox C = seg_capsule_box(R, S, bx, by, bz, ra);
    const RingBox &B = C.B;
    const int lanes = C.lanes;
    const uint32_t part = threadIdx.x % (uint32_t)lanes;
    for (int k = (int)threadIdx.x / lanes; k < C.total; k += 256 / lanes)
        seg_ring_visit(V, S, C, k % B.nx, (k / B.nx) % B.ny, k / (B.nx * B.ny), part, npts, nbuckets, offer);
}

__global__ __launch_bounds__(256) void ring_segment_kernel(RingView V, const double *__restrict__ seg, const double *__restrict__ reach,
                                                           double reach_all, uint32_t index_base, uint32_t *__restrict__ out_idx,
                                                           double *__restrict__ out_d2, double *__restrict__ out_s,
                                                           WorkCounters *__restrict__ work)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    __shared__ unsigned long long s_w[8];
    const size_t slot = blockIdx.x;
    SegGeom S;
    double bx, by, bz, ra;
    const double r2 = seg_load_r2(seg, reach, reach_all, slot, S, bx, by, bz, ra);
    double bd = __builtin_huge_val(), bs = __builtin_nan("");
    uint32_t bi = kNoIndex, npts = 0, nbuckets = 0;
    const auto offer = [&](double px, double py, double pz, uint32_t id) {
        double d2, s;
        seg_point_d2(S, px, py, pz, d2, s);
        if (d2 <= r2 && better(d2, id, bd, bi)) { bd = d2; bi = id; bs = s; }
    };
    if (V.st->count != 0 && r2 >= 0.0) seg_ring_walk(V, S, bx, by, bz, ra, npts, nbuckets, offer);      // block-uniform
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

// ---- the rolling-map form of the sweep ------------------------------------------------------------------------------------------
// One block per sweep: the overflow queue exhaustively once, then the capsule's box (seg_capsule_box) with the per-cell skip, every
// record judged by seg_entry_t, the block's winner by block_argmin256 with t in the place of d2.
//
// The ordered walk.  A minimum distance can sit anywhere in the capsule, a first contact cannot: it lies towards a.  When no axis is
// folded, L2 > 0 and r + |e| < 2^20 h, the box is visited in LAYERS along the dominant axis k of e (largest |e_k|), from a's side,
// in rounds of whole layers; after a round the block agrees on the best t it holds (tb) and stops before layer c when
//     tb * |e_k|  <  dist_k(a, near face of layer c) - r - h / 8.
// Why nothing unseen can then win.  Let P be a row filed in layer c or beyond, D = r + |e| and u = 2^-53.
//   * Geometry.  Its cell coordinate along k is at or beyond c's, so (cell placement, 5e-7 h, as for the skip above) its offset from
//     a along the direction of travel is w_k >= dist_k - 5e-7 h.  Let tau = dot / L2 and dp = its distance from the LINE, as real
//     numbers.  If P passes d2 <= r2 it is within r + 1e-9 h of the segment (the rounding of d2 and r2: a few u D), so dp <= r + 1e-9 h
//     and w_k <= |e_k| + r + 1e-9 h.  f = tau - sqrt(max(r^2 - dp^2, 0)) / |e| is what step 5 computes in real numbers; the centre
//     a + f e is at distance max(r, dp) from P, so f |e_k| >= w_k - r - 1e-9 h.  The right side of the stop test is positive, so
//     w_k > r + 0.12 h: P is not in contact at the start (step 2 does not apply) and f > 0.
//   * Rounding.  With E = |w| |e| <= D^2 (a blocker has |w| <= |e| + r): dot, L2, ww, r2 carry relative errors of a few u, g = ww - r2
//     an absolute one below 6 u ww, and disc = dot*dot - L2*g one below 40 u E^2 -- the cancellation the clamp of step 4 is for.
//     |sqrt(x) - sqrt(y)| <= sqrt|x - y| turns that into sqrt(40 u) E = 6.7e-8 E in the numerator, hence, after the division by L2,
//     |t - f| |e| <= 6.8e-8 |w| <= 6.8e-8 D < 0.072 h under the cap.  Step 6 can only raise t to 0 or lower it to s, and
//     s >= min(tau, 1) - 1e-9 >= min(f, 1) - 1e-9, with |e_k| >= w_k - r - 1e-9 h for the case s = 1.
//   Together the t that P is given satisfies t |e_k| >= dist_k - r - (0.072 + 5e-7 + 3e-9) h > dist_k - r - h / 8 > tb |e_k|, with
//   0.05 h to spare for the roundings of the test itself (a_k up to 1e9 cells: 1e-7 h): P loses to the held winner strictly, ties
//   included.  Rows outside the box are no blockers at all, and the overflow queue has been read in full before the first layer.
// Outside those conditions the walk is one round over the whole box.  Exactness never rests on the order of the layers: only the
// stop does, and every record that is read is judged by seg_entry_t.
//
// The round is what the block reads in one trip of its loop anyway (256 / lanes positions, at least one layer): finer rounds would
// add dependent memory trips without adding loads in flight.  The agreement costs one barrier per round: every thread folds the best
// t it has met so far into s_tb[round & 1] (t >= 0 orders as its bit pattern; the minimum is cumulative, so the words are never
// reset), and a thread that is a round ahead writes the other word while a slower one still reads this one; it cannot get two ahead,
// the next barrier needs them all.  The loop and its exit are block-uniform.
constexpr double kSweepCapCells = 1048576.0;     // r + |e| below 2^20 cells for the early stop
constexpr double kSweepSlack = 0.125;            // cells

__global__ __launch_bounds__(256) void ring_sweep_kernel(RingView V, const double *__restrict__ seg, const double *__restrict__ radius,
                                                         uint32_t index_base, uint32_t *__restrict__ out_idx, double *__restrict__ out_t,
                                                         WorkCounters *__restrict__ work)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    __shared__ unsigned long long s_w[8];
    __shared__ unsigned long long s_tb[2];
    const size_t slot = blockIdx.x;
    const RingDesc &R = V.R;
    SegGeom S;
    double bx, by, bz, ra;
    const double r2 = seg_load_r2(seg, radius, 0.0, slot, S, bx, by, bz, ra);
    double bt = __builtin_huge_val();
    uint32_t bi = kNoIndex, npts = 0, nbuckets = 0;
    const auto offer = [&](double px, double py, double pz, uint32_t id) {
        double t;
        if (seg_entry_t(S, r2, px, py, pz, t) && better(t, id, bt, bi)) { bt = t; bi = id; }
    };
    if (threadIdx.x < 2) s_tb[threadIdx.x] = (unsigned long long)__double_as_longlong(__builtin_huge_val());
    __syncthreads();
    if (V.st->count != 0 && r2 >= 0.0) {                    // block-uniform
        const uint32_t oh = V.st->ovf_head;
        ring_for_live_records(V.ovf, oh, V.st->ovf_tail - oh, R.ovf_mask, threadIdx.x, 256u, npts, offer);
        const SegBox C = seg_capsule_box(R, S, bx, by, bz, ra);
        const RingBox &B = C.B;
        const int k = fabs(S.ex) >= fabs(S.ey) && fabs(S.ex) >= fabs(S.ez) ? 0 : fabs(S.ey) >= fabs(S.ez) ? 1 : 2;
        const double ek = k == 0 ? S.ex : k == 1 ? S.ey : S.ez, ak = k == 0 ? S.ax : k == 1 ? S.ay : S.az;
        const int nk = k == 0 ? B.nx : k == 1 ? B.ny : B.nz, k0 = k == 0 ? B.x0 : k == 1 ? B.y0 : B.z0;
        const int nu = k == 0 ? B.ny : B.nx, nv = k == 2 ? B.ny : B.nz, nuv = nu * nv;     // the layer's two axes: the others, in x y z order
        const bool ordered = !C.folded && S.L2 > 0.0 && ra + sqrt(S.L2) < kSweepCapCells * R.h;
        const bool fwd = ek >= 0.0;
        const int lanes = C.lanes, per = 256 / lanes;
        const int W = ordered ? max(1, per / nuv) : nk;     // layers per round
        const double aek = fabs(ek), margin = ra + kSweepSlack * R.h;
        const uint32_t part = threadIdx.x % (uint32_t)lanes;
        int round = 0;
        for (int c = 0; c < nk; c += W) {
            const int end = min(c + W, nk) * nuv;
            for (int m = c * nuv + (int)threadIdx.x / lanes; m < end; m += per) {
                const int layer = m / nuv, rem = m - layer * nuv, ju = rem % nu, jv = rem / nu;
                const int jk = fwd ? layer : nk - 1 - layer;
                seg_ring_visit(V, S, C, k == 0 ? jk : ju, k == 0 ? ju : k == 1 ? jk : jv, k == 2 ? jk : jv, part, npts, nbuckets, offer);
            }
            const int cn = c + W;                           // the next round's first layer
            if (cn >= nk) break;                            // block-uniform, as everything the stop test reads
            if (bt < __builtin_huge_val()) atomicMin(&s_tb[round & 1], (unsigned long long)__double_as_longlong(bt));
            __syncthreads();
            const double tb = __longlong_as_double((long long)s_tb[round & 1]);
            round++;
            const double dist = fwd ? (double)(k0 + cn) * R.h - ak : ak - (double)(k0 + nk - cn) * R.h;
            if (tb * aek < dist - margin) break;
        }
    }
    block_argmin256(bt, bi, s_d, s_i);
    if (threadIdx.x == 0) {
        out_idx[slot] = reported_index(bt, bi, index_base);
        if (out_t) out_t[slot] = bi != kNoIndex ? bt : sweep_unblocked_t(r2);
    }
    if (work) ring_add_work(work, npts, nbuckets, s_w);
}

// ---- the streaming form ---------------------------------------------------------------------------------------------------------
// grid (parts, tiles): block (p, t) measures rows p * 256 + lane, + parts * 256, .. against segments t * kSegTile .. of the slice
// and writes one partial winner per segment: part_*[q * parts + p] for the slice's segment q.  SWEEP: the value is the entry
// parameter t of seg_entry_t instead of d2, `reach` is the sweep's radius and there is no s (part_s is not touched).
template <bool SWEEP>
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
        double r2 = -1.0, bx, by, bz, ra;
        if (q < Q) r2 = seg_load_r2(seg, reach, reach_all, q, S, bx, by, bz, ra);
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
            double v, s;
            bool in;
            if (SWEEP) { s = 0.0; in = seg_entry_t(S, s_g[t][7], px, py, pz, v); }
            else { seg_point_d2(S, px, py, pz, v, s); in = v <= s_g[t][7]; }
            if (in && v < bd[t]) { bd[t] = v; bi[t] = (uint32_t)i; bs[t] = s; }      // ascending i: the first of equals stays
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
        part_d2[o] = d; part_idx[o] = i;
        if (!SWEEP) part_s[o] = s;
    }
}

// one wave per segment folds its `parts` partial winners; d2 / s may be NULL.  SWEEP: out_d2 receives t -- 1, or NaN for an invalid
// sweep, when nothing blocks (seg / radius: the slice's, read again for that) -- and there is no s
template <bool SWEEP>
__global__ __launch_bounds__(64) void segment_finish_kernel(const double *__restrict__ part_d2, const uint32_t *__restrict__ part_idx,
                                                            const double *__restrict__ part_s, uint32_t parts, uint32_t index_base,
                                                            const double *__restrict__ seg, const double *__restrict__ radius,
                                                            uint32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_s)
{
    const size_t q = blockIdx.x;
    double d = __builtin_huge_val(), s = __builtin_nan("");
    uint32_t i = kNoIndex;
    for (uint32_t p = threadIdx.x; p < parts; p += 64) {
        const size_t o = q * parts + p;
        if (better(part_d2[o], part_idx[o], d, i)) { d = part_d2[o]; i = part_idx[o]; if (!SWEEP) s = part_s[o]; }
    }
    seg_wave_best(d, i, s);
    if (threadIdx.x == 0) {
        out_idx[q] = reported_index(d, i, index_base);
        if (SWEEP) {
            if (out_d2) out_d2[q] = i != kNoIndex ? d : sweep_unblocked_t(sweep_r2(seg, radius, q));
        } else {
            if (out_d2) out_d2[q] = d;
            if (out_s) out_s[q] = i == kNoIndex ? __builtin_nan("") : s;
        }
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

// every sweep unblocked (an empty cloud): t = 1, or NaN for an invalid sweep
__global__ __launch_bounds__(256) void sweep_fill_none_kernel(const double *__restrict__ seg, const double *__restrict__ radius,
                                                              uint32_t *__restrict__ idx, double *__restrict__ t, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    idx[i] = kNoIndex;
    if (t) t[i] = sweep_unblocked_t(sweep_r2(seg, radius, i));
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
    if (empty) { radius[i] = inflate_skipped_radius(P); idx[i] = kNoIndex; s[i] = __builtin_nan(""); return; }
    const double r = inflate_radius(P, d2[i]);
    radius[i] = r;
    if (r < P.max_radius) return;
    idx[i] = kNoIndex;
    s[i] = __builtin_nan("");
}

}  // namespace pct
