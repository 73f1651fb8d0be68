// bezier_certify.hpp -- the certified Bezier check: whole curves proven free, or shown to collide, by subdivision
// (pct_bezier_certify_batch*, contract in include/pct_engine.h, paragraph "Certified Bezier check"; included by engine.hip behind
// segment_search.hpp and bezier_batch.hpp).
//
// A PIECE is a control polygon of order n that stands for u in [k / 2^d, (k + 1) / 2^d] of one segment.  All live pieces of a round
// have the same depth d = the round's number, lie in one buffer ordered by (trajectory, segment, k), and are examined together:
//   bc_init_kernel      a lane per trajectory: the certificate's defaults, the trajectory's state, the call's control words
//   bc_valid_kernel     a lane per segment: a bad seg_time or a world control point beyond FLT_MAX marks its trajectory INVALID
//   bc_seed_kernel      a lane per segment: the world control points P[j] = c[j] * T as the piece of depth 0 at slot = segment
//   -- the window forms (pct_bezier_*_window_batch*, paragraph "Windows of a trajectory") put in the place of bc_seed_kernel --
//   bc_window_kernel    a lane per segment: u0, u1 of its part of [t0, t1] into win[segment], NaN for a segment outside the window;
//                       behind them a lane per trajectory: a bad t0 or horizon marks it INVALID
//   bc_seed_window_kernel  a lane per segment: bc_seed_kernel's polygon restricted to [u0, u1] by up to two de Casteljau cuts
//   -- per round --
//   bc_geometry_kernel  a lane per piece: chord ends a, b (fp32), rho, reach, and the three queries it poses: the capsule
//                       (a, b, reach) and the two nearest-neighbour queries a and b; a dead slot poses NaN queries, which the
//                       searches answer "nothing" without a walk
//   (engine.hip)        the capsule count and the nearest-neighbour batch on the path `algo` selects: the existing searches
//   bc_classify_kernel  a lane per piece: pieces, depth and min_d2 of its trajectory, the lowest hit (an atomicMin over 2 * slot + end:
//                       the slots are in (segment, k) order and a comes before b), blocked or not
//   bc_mark_kernel      a lane per piece, behind the round's hits: the winner of a hit writes the hit's fields; a blocked piece of
//                       a trajectory without a hit either splits or, at max_depth, makes the trajectory UNDECIDED; the ranks of the
//                       splitting pieces inside their tile of 256 (scan.hpp) and the tile's total
//   scan_tile_sums_kernel (scan.hpp)   tile totals -> tile offsets; BcScanDone turns the grand total into the next round's live
//                       count, or -- twice the total exceeds piece_cap -- into the capped flag and no live piece
//   bc_split_kernel     a lane per child: de Casteljau at 1/2 with the polygon in registers; child 2 * rank + side: the compaction is
//                       stable, so the order (trajectory, segment, k) is kept.  In a capped round it marks the owners UNDECIDED.
//   -- behind the last round --
//   bc_finish_kernel    a lane per trajectory: the status from the state; lane 0: the call's stats
// The device form launches every per-piece kernel over piece_cap slots for max_depth + 1 rounds and every lane guards on the
// device-side live count; the host form reads that count once per round, sizes its launches by it and stops at zero.  A lane
// beyond the live count does nothing, so both forms give the same bytes.
//
// WHAT FREE PROVES, and the slack in `reach`.  Let P be the fp64 polygon of a piece as stored, C its exact Bezier curve, and (a, b)
// its chord ends as the searches see them (fp32).
// (1) dist(., segment(a, b)) is a convex function and C(u) is a convex combination of the P[j], so every point of C is within
//     rho* = max_j dist(P[j], segment) of the chord -- whatever a and b are: narrowing them to fp32 moves the chord, and rho is taken
//     from the moved chord, P[0] and P[n] included.
// (2) rho is that maximum in the arithmetic of "Segment queries".  There w, e and c = w - s*e carry absolute errors of a few
//     2^-53 * (|P[j]| + |a| + |b|) <= 2^-50 * cmax (the closest point being a minimum, the rounding of s enters only in second
//     order), the sums of squares and sqrt a relative 2^-51: rho >= rho* * (1 - 2^-50) - 2^-49 * cmax.
// (3) A row x within `margin` of C is within margin + rho* of the chord (1).  Its d2 in the capsule search carries the same errors
//     as (2) with |x| <= cmax + reach in cmax's place, and reach * reach a relative 2^-52.  So x is counted whenever
//     reach >= (margin + rho*) * (1 + 2^-49) + 2^-47 * (cmax + reach), which reach = (margin + rho) * (1 + 2^-20) + cmax * 2^-40
//     satisfies with (margin + rho) * (2^-20 - 2^-46) + cmax * (2^-40 - 2^-45) to spare: the piece-local roundings of rho, reach^2
//     and d2 are covered unconditionally.
// (4) The halvings.  q = (p + p') * 0.5 rounds once, in the sum (the halving is exact short of underflow, 2^-1075): an absolute
//     error of at most 2^-53 * |q|.  Every value of every level is a convex combination of the parent's points, so after the n <= 12
//     levels of one split a child's point is off the exact subdivision of its parent's stored polygon by at most 12 * 2^-53 * M, M
//     the largest |coordinate| of the parent; a curve moves by no more than its control points.  Over the d <= 20 splits above a
//     piece, C differs from the true curve of the segment on the piece's interval by at most E = 240 * 2^-53 * M0 < 2^-45 * M0,
//     M0 the largest |world control coordinate| of the segment (the hull only shrinks, up to the same errors).
//     E is inherited: it scales with M0, not with the piece's own cmax, which may be far smaller for a piece near the origin of a
//     curve that reaches far from it.  The spare of (3) covers E when cmax >= M0 / 16, and otherwise when
//     margin + rho >= 2^-25 * M0 -- 30 micrometres of margin per kilometre of |coordinate|.  Under that condition FREE is a proof:
//     no row of the window lies within `margin` of any point of the curve.  Below it (a margin of nanometres on kilometre
//     coordinates) the slack of the contract does not cover E for such pieces, and no claim is made.
// (5) Windows (bc_seed_window_kernel).  A first piece that was cut stands for u in [u0, u1] of its segment, u0 and u1 as bc_window_kernel
//     computed them: the window IS that interval (t0, t1 and the segment's time enter through one rounded subtraction, division and
//     the sequential sums).  A cut at t computes q = w * p + t * p' with w = 1 - t rounded once: two products and a sum, each off by
//     at most 2^-53 of a value that is at most M0 in magnitude, and w + t differs from 1 by at most 2^-54: 3.5 * 2^-53 * M0 per
//     level, 12 levels, two cuts: 84 * 2^-53 * M0.  The second cut is at t = u0 / u1 rounded, so the right part starts at
//     u0' = t * u1, within 2^-53 of u0; every control point of a restriction is a value of the segment's blossom, which moves by
//     at most 2 * M0 per unit of each of its n <= 12 arguments: another 24 * 2^-53 * M0, and a curve point with u between u0 and u0'
//     is that near the piece's own end.  Together the stored first piece is within 108 * 2^-53 * M0 of the exact restriction, and
//     with the halvings of (4) E <= 348 * 2^-53 * M0 < 0.68 * 2^-44 * M0.  That no longer fits under 2^-45 * M0.  The spare of (3)
//     still covers it when cmax >= M0 / 16 (cmax * (2^-40 - 2^-45) >= 0.96 * 2^-44 * M0), and otherwise when
//     margin + rho >= 2^-24 * M0 -- 60 micrometres per kilometre of |coordinate|, twice the whole-curve condition.  Under it FREE
//     of a window form is a proof for the points of the curve with u in [u0, u1] of every segment the window touches.  reach itself
//     is unchanged.  A segment the window covers whole is not cut and keeps (4) as it stands.
// HIT needs no argument: the end of a piece is a point the sampled check could have sampled, judged by its test.
#pragma once
#include "../../include/pct_engine.h"
#include "bernstein.hpp"
#include "scan.hpp"
#include "segment.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr int kBcPts = kMaxBezierOrder + 1;      // control points of a piece
constexpr int kBcPoly = 3 * kBcPts;              // doubles of a stored polygon: x y z of P[0], of P[1], ...
constexpr int kBcTile = 256;                     // pieces per scan tile (one block of bc_mark_kernel)
constexpr int kBcMaxDepth = 20;                  // pct_engine.h: "max_depth (0..20)"
constexpr long long kBcMaxPieces = 1ll << 24;    // piece_cap's upper limit: 2 * slot + end stays a uint32, a buffer below 6 GB
constexpr uint32_t kBcNoHit = 0xFFFFFFFFu;
constexpr uint32_t kBcInvalid = 1u, kBcUndecided = 2u;
constexpr double kBcFltMax = 3.4028234663852886e38;

struct BcMeta { int32_t traj, seg, order; uint32_t k; };       // traj < 0: a dead slot (the segment of an INVALID trajectory)
struct BcTraj { uint32_t hitkey, flags; };                     // 2 * slot + end of the lowest hit | kBcInvalid, kBcUndecided
struct BcCtl {
    uint32_t live;            // pieces of the current round
    uint32_t capped;          // the call's flag
    uint32_t capped_now;      // this round's splits were refused
    uint32_t rounds;          // rounds that examined a piece
    uint32_t examined;        // this round examined one
    uint32_t pad;
    unsigned long long pieces;
};

// the batch as the kernels read it: device pointers of pct_bezier_batch (t_start is not read)
struct BcDesc {
    const double *coef;
    long long row_stride;
    const double *seg_time;
    const int32_t *orders;
    const int32_t *seg_offsets;
    long long B;
};

// the trajectory that owns segment i: the largest b with seg_offsets[b] <= i, or -1 when that trajectory's range does not hold i
__device__ __forceinline__ long long bc_owner(const BcDesc &D, int i)
{
    long long lo = 0, hi = D.B - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (D.seg_offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return D.seg_offsets[lo] <= i && i < D.seg_offsets[lo + 1] ? lo : -1;
}

// the number of segments the call seeds: seg_offsets[B], nothing when it exceeds piece_cap (the host form has refused that)
__device__ __forceinline__ long long bc_total_seg(const BcDesc &D, long long piece_cap)
{
    const long long t = D.seg_offsets[D.B];
    return t < 0 || t > piece_cap ? 0 : t;
}

// lane b <= B of an init kernel: the state of trajectory b, or (b == B) the control words; false for lane B
__device__ __forceinline__ bool bc_init_state(const BcDesc &D, long long piece_cap, long long b, BcTraj *__restrict__ traj, BcCtl *__restrict__ ctl)
{
    const bool over = (long long)D.seg_offsets[D.B] > piece_cap;      // device form only: more segments than pieces
    if (b == D.B) {
        ctl->live = (uint32_t)bc_total_seg(D, piece_cap);
        ctl->capped = over ? 1u : 0u;
        ctl->capped_now = 0;
        ctl->rounds = 0;
        ctl->examined = 0;
        ctl->pad = 0;
        ctl->pieces = 0;
        return false;
    }
    int s0, s1;      // an unsound range (the host form has refused it): INVALID, and none of its rows is read
    const bool sound = bezier_range_sound(D.seg_offsets, D.orders, D.row_stride, D.B, b, s0, s1);
    traj[b].hitkey = kBcNoHit;
    traj[b].flags = !sound ? kBcInvalid : over ? kBcUndecided : 0u;
    return true;
}

// lane b < B: certificate defaults and state; lane B: the control words
__global__ __launch_bounds__(256) void bc_init_kernel(BcDesc D, long long piece_cap, pct_traj_certificate *__restrict__ cert,
                                                      BcTraj *__restrict__ traj, BcCtl *__restrict__ ctl)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > D.B) return;
    if (!bc_init_state(D, piece_cap, b, traj, ctl)) return;
    cert[b].status = PCT_CERT_FREE;
    cert[b].depth = 0;
    cert[b].hit_seg = -1;
    cert[b].hit_idx = PCT_NO_INDEX;
    cert[b].hit_u = __builtin_nan("");
    cert[b].hit_d2 = __builtin_huge_val();
    cert[b].min_d2 = __builtin_huge_val();
    cert[b].pieces = 0;
}

// lane i < total_seg: INVALID for the owner of a segment whose time is not finite and > 0 or whose world control points leave fp32
__global__ __launch_bounds__(256) void bc_valid_kernel(BcDesc D, long long piece_cap, BcTraj *__restrict__ traj)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bc_total_seg(D, piece_cap)) return;
    const long long b = bc_owner(D, (int)i);
    if (b < 0 || (traj[b].flags & kBcInvalid)) return;       // kBcInvalid here: an unsound range, set before this launch
    const double T = D.seg_time[i];
    bool bad = !(T > 0.0) || !(T <= 1.7976931348623157e308);
    const int m = D.orders[i] + 1;
    const double *c = D.coef + (size_t)i * D.row_stride;
    for (int j = 0; j < 3 * m; j++) bad |= !(fabs(c[j] * T) <= kBcFltMax);
    if (bad) atomicOr(&traj[b].flags, kBcInvalid);
}

// lane i < total_seg: the piece of depth 0 at slot i, dead when its trajectory is not examined
__global__ __launch_bounds__(256) void bc_seed_kernel(BcDesc D, long long piece_cap, const BcTraj *__restrict__ traj, double *__restrict__ poly,
                                                      BcMeta *__restrict__ meta)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bc_total_seg(D, piece_cap)) return;
    const long long b = bc_owner(D, (int)i);
    if (b < 0 || traj[b].flags != 0) { meta[i] = BcMeta{ -1, 0, 0, 0 }; return; }
    const int n = D.orders[i], m = n + 1;
    const double T = D.seg_time[i];
    const double *c = D.coef + (size_t)i * D.row_stride;
    double *p = poly + (size_t)i * kBcPoly;
    for (int j = 0; j < m; j++)
        for (int k = 0; k < 3; k++) p[3 * j + k] = c[k * m + j] * T;
    meta[i] = BcMeta{ (int32_t)b, (int32_t)i, n, 0u };
}

// ---- windows of a trajectory (pct_engine.h, "Windows of a trajectory") --------------------------------------------------------------
// what the window forms read beside the batch: device pointers, t_start and horizon B doubles each or NULL (0 and +inf for all), and
// win[segment] = {u0, u1}, the part of the segment inside its trajectory's window, u0 = NaN for a segment with none
struct BcWinDesc {
    const double *t_start;
    const double *horizon;
    double *win;
};

// the window [t0, t1) of trajectory b as the contract's step 1 has it; false: the trajectory is INVALID
__device__ __forceinline__ bool bc_window_of(const BcWinDesc &W, long long b, double &t0, double &t1)
{
    t0 = W.t_start ? W.t_start[b] : 0.0;
    const double h = W.horizon ? W.horizon[b] : __builtin_huge_val();
    t1 = t0 + h;
    return t0 >= 0.0 && t0 <= 1.7976931348623157e308 && h > 0.0;
}

// lane i < total_seg: win[i], behind bc_valid_kernel (a trajectory that is INVALID already has only dead slots, and its times are not
// summed).  Lane seg_lanes + b, b < B: the window's own INVALID rule.
__global__ __launch_bounds__(256) void bc_window_kernel(BcDesc D, BcWinDesc W, long long piece_cap, long long seg_lanes, BcTraj *__restrict__ traj)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double t0, t1;
    if (i >= seg_lanes) {
        const long long b = i - seg_lanes;
        if (b < D.B && !bc_window_of(W, b, t0, t1)) atomicOr(&traj[b].flags, kBcInvalid);
        return;
    }
    if (i >= bc_total_seg(D, piece_cap)) return;
    double *w = W.win + 2 * (size_t)i;
    w[0] = w[1] = __builtin_nan("");
    const long long b = bc_owner(D, (int)i);
    if (b < 0 || traj[b].flags != 0 || !bc_window_of(W, b, t0, t1)) return;
    double c = 0.0;
    for (int s = D.seg_offsets[b]; s < (int)i; s++) c = c + D.seg_time[s];
    const double T = D.seg_time[i], cn = c + T;
    if (!(t0 < cn && t1 > c)) return;
    const double u0 = t0 <= c ? 0.0 : (t0 - c) / T;
    const double u1 = t1 >= cn ? 1.0 : (t1 - c) / T;
    if (!(u0 < u1)) return;
    w[0] = u0;
    w[1] = u1;
}

// One de Casteljau cut of p[0..n] at t, level by level q[i] = w * p[i] + t * p[i + 1] with w = 1 - t, in place: what is left in p[] is
// the right part (the last point of every level, reversed); the left part (p[0] of every level) replaces it unless `right`.
// Constant bounds, unrolled: p[] and l[] are registers and n only predicates, as in bc_split_kernel.
__device__ __forceinline__ void bc_cut(double (&p)[kBcPts], int n, double t, bool right)
{
    const double w = 1.0 - t;
    double l[kBcPts];
    l[0] = p[0];
#pragma unroll
    for (int lev = 1; lev < kBcPts; lev++) {
#pragma unroll
        for (int i = 0; i + lev < kBcPts; i++)
            if (i + lev <= n) p[i] = w * p[i] + t * p[i + 1];
        l[lev] = p[0];
    }
    if (!right) {
#pragma unroll
        for (int j = 0; j < kBcPts; j++) p[j] = l[j];
    }
}

// lane i < total_seg: bc_seed_kernel's piece restricted to [u0, u1] = win[i]: cut at u1 and keep the left part, then cut at u0 / u1
// and keep the right part; an end the window covers (u1 == 1, u0 == 0) is not cut, so a segment inside the window gets bc_seed_kernel's
// bytes.  A segment outside the window is a dead slot.
__global__ __launch_bounds__(256) void bc_seed_window_kernel(BcDesc D, long long piece_cap, const BcTraj *__restrict__ traj,
                                                             const double *__restrict__ win, double *__restrict__ poly, BcMeta *__restrict__ meta)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bc_total_seg(D, piece_cap)) return;
    const long long b = bc_owner(D, (int)i);
    const double u0 = win[2 * (size_t)i], u1 = win[2 * (size_t)i + 1];
    if (b < 0 || traj[b].flags != 0 || !(u0 < u1)) { meta[i] = BcMeta{ -1, 0, 0, 0 }; return; }
    const int n = D.orders[i], m = n + 1;
    const double T = D.seg_time[i];
    const double *c = D.coef + (size_t)i * D.row_stride;
    double *dst = poly + (size_t)i * kBcPoly;
    const double t = u0 / u1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double p[kBcPts];
#pragma unroll
        for (int j = 0; j < kBcPts; j++) p[j] = j <= n ? c[k * m + j] * T : 0.0;
        if (u1 < 1.0) bc_cut(p, n, u1, false);
        if (u0 > 0.0) bc_cut(p, n, t, true);
#pragma unroll
        for (int j = 0; j < kBcPts; j++)
            if (j <= n) dst[3 * j + k] = p[j];
    }
    meta[i] = BcMeta{ (int32_t)b, (int32_t)i, n, 0u };
}

// the parameter v of a piece end inside its first piece -> the segment's own u (step 5 there): v itself for an uncut segment
__device__ __forceinline__ double bc_window_u(const double *__restrict__ win, int seg, double v)
{
    const double u0 = win[2 * (size_t)seg], u1 = win[2 * (size_t)seg + 1];
    return (1.0 - v) * u0 + v * u1;
}

// Step (4) of the contract for the polygon p of order n: the chord ends narrowed to fp32 into q[0..5] (a, then b) and widened into
// ends[0..5], rho = the largest distance of a control point from segment (a, b), cmax = the largest |coordinate|.  The certified
// check and the clearance (bezier_clearance.hpp) both take their geometry from here.
__device__ __forceinline__ void bc_chord(const double *__restrict__ p, int n, float *__restrict__ q, double (&ends)[6], double &rho, double &cmax)
{
    for (int k = 0; k < 3; k++) {
        const float a = (float)p[k], b = (float)p[3 * n + k];
        q[k] = a; q[3 + k] = b;
        ends[k] = (double)a; ends[3 + k] = (double)b;
    }
    SegGeom S;
    double bx, by, bz;
    seg_load(ends, 0, S, bx, by, bz);
    double rho2 = 0.0;
    cmax = 0.0;
    for (int j = 0; j <= n; j++) {
        double d2, s;
        seg_point_d2(S, p[3 * j], p[3 * j + 1], p[3 * j + 2], d2, s);
        if (d2 > rho2) rho2 = d2;
        for (int k = 0; k < 3; k++) cmax = fmax(cmax, fabs(p[3 * j + k]));
    }
    rho = sqrt(rho2);
}

// lane slot < nslots: the queries of a live piece; NaN queries for any other slot
__global__ __launch_bounds__(256) void bc_geometry_kernel(const double *__restrict__ poly, const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl,
                                                          uint32_t nslots, double margin, double *__restrict__ seg, double *__restrict__ reach,
                                                          float *__restrict__ q)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots) return;
    double *sg = seg + 6 * (size_t)slot;
    float *qq = q + 6 * (size_t)slot;
    if (slot >= ctl->live || meta[slot].traj < 0) {
        for (int k = 0; k < 6; k++) { sg[k] = __builtin_nan(""); qq[k] = __builtin_nanf(""); }
        reach[slot] = 0.0;
        return;
    }
    const int n = meta[slot].order;
    const double *p = poly + (size_t)slot * kBcPoly;
    double ends[6], rho, cmax;
    bc_chord(p, n, qq, ends, rho, cmax);
    for (int k = 0; k < 6; k++) sg[k] = ends[k];
    reach[slot] = ((margin + rho) * (1.0 + 0x1p-20)) + cmax * 0x1p-40;
}

__device__ __forceinline__ bool bc_is_hit(double d2, double margin) { return sqrt(d2) - margin < 0.0; }

// lane slot < nslots: a live piece adds itself to its trajectory and to the call, offers its hits, and notes whether it is blocked
__global__ __launch_bounds__(256) void bc_classify_kernel(const BcMeta *__restrict__ meta, BcCtl *__restrict__ ctl, uint32_t nslots, double margin,
                                                          int round, const uint32_t *__restrict__ count, const double *__restrict__ nn_d2,
                                                          pct_traj_certificate *__restrict__ cert, BcTraj *__restrict__ traj,
                                                          uint32_t *__restrict__ flag)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots) return;
    if (slot >= ctl->live || meta[slot].traj < 0) { flag[slot] = 0; return; }
    const int b = meta[slot].traj;
    atomicAdd(reinterpret_cast<unsigned long long *>(&cert[b].pieces), 1ull);
    atomicAdd(&ctl->pieces, 1ull);
    cert[b].depth = round;                                    // every live piece of the round stores the same value
    ctl->examined = 1u;
    const double da = nn_d2[2 * (size_t)slot], db = nn_d2[2 * (size_t)slot + 1];
    // a d2 is >= 0 or +inf: the order of the bit patterns is the order of the values
    atomicMin(reinterpret_cast<unsigned long long *>(&cert[b].min_d2), (unsigned long long)__double_as_longlong(da < db ? da : db));
    if (bc_is_hit(da, margin)) atomicMin(&traj[b].hitkey, 2u * slot);
    else if (bc_is_hit(db, margin)) atomicMin(&traj[b].hitkey, 2u * slot + 1u);
    flag[slot] = count[slot] != 0 ? 1u : 0u;
}

// One tile of kBcTile slots per block, behind bc_classify_kernel.  flag in: blocked; flag out: 1 + the rank of a splitting piece inside
// its tile, 0 for every other slot; tile_sum[block] = the tile's splitting pieces.  kWindow: hit_u goes through win[] (the window forms).
template <bool kWindow>
__global__ __launch_bounds__(kBcTile) void bc_mark_kernel(const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl, uint32_t nslots, int round,
                                                          int max_depth, const uint32_t *__restrict__ nn_idx, const double *__restrict__ nn_d2,
                                                          pct_traj_certificate *__restrict__ cert, BcTraj *__restrict__ traj,
                                                          uint32_t *__restrict__ flag, uint32_t *__restrict__ tile_sum,
                                                          const double *__restrict__ win)
{
    const uint32_t slot = blockIdx.x * kBcTile + threadIdx.x;
    uint32_t split = 0;
    if (slot < nslots && slot < ctl->live && meta[slot].traj >= 0) {
        const BcMeta M = meta[slot];
        const uint32_t key = traj[M.traj].hitkey;
        if (key != kBcNoHit) {                                // the trajectory is HIT in this round and retired
            if ((key >> 1) == slot) {
                const uint32_t end = key & 1u;
                cert[M.traj].hit_seg = M.seg;
                cert[M.traj].hit_idx = nn_idx[key];
                cert[M.traj].hit_d2 = nn_d2[key];
                const double v = ldexp((double)(M.k + end), -round);
                cert[M.traj].hit_u = kWindow ? bc_window_u(win, M.seg, v) : v;
            }
        } else if (flag[slot]) {
            if (round >= max_depth) atomicOr(&traj[M.traj].flags, kBcUndecided);
            else split = 1;
        }
    }
    uint32_t total;
    const uint32_t rank = block_exclusive<uint32_t, kBcTile>(split, total);
    if (slot < nslots) flag[slot] = split ? rank + 1u : 0u;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// the grand total of the splitting pieces -> the next round
struct BcScanDone {
    BcCtl *ctl;
    uint32_t piece_cap;
    __device__ void operator()(uint32_t total) const
    {
        if (ctl->examined) ctl->rounds++;
        ctl->examined = 0;
        const bool over = 2ull * total > piece_cap;
        ctl->capped_now = over ? 1u : 0u;
        if (over) ctl->capped = 1u;
        ctl->live = over ? 0u : 2u * total;
    }
};

// lane t < 2 * nslots: child `side` of slot t / 2.  Level by level q[i] = (p[i] + p[i + 1]) * 0.5, in place: the left child is p[0] of
// every level, and what is left in p[] at the end is the last point of every level, reversed -- the right child.  The loops have
// constant bounds and are unrolled, so p[] and l[] are registers; the order n only predicates.
__global__ __launch_bounds__(256) void bc_split_kernel(const double *__restrict__ poly_in, const BcMeta *__restrict__ meta_in,
                                                       double *__restrict__ poly_out, BcMeta *__restrict__ meta_out,
                                                       const uint32_t *__restrict__ flag, const uint32_t *__restrict__ tile_off,
                                                       const BcCtl *__restrict__ ctl, uint32_t nslots, BcTraj *__restrict__ traj)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t slot = t >> 1, side = t & 1u;
    if (slot >= nslots) return;
    const uint32_t f = flag[slot];
    if (!f) return;
    const BcMeta M = meta_in[slot];
    if (ctl->capped_now) {
        if (!side) atomicOr(&traj[M.traj].flags, kBcUndecided);
        return;
    }
    const uint32_t out = 2u * (tile_off[slot / kBcTile] + f - 1u) + side;      // < 2 * total <= piece_cap (BcScanDone)
    const int n = M.order;
    const double *src = poly_in + (size_t)slot * kBcPoly;
    double *dst = poly_out + (size_t)out * kBcPoly;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double p[kBcPts], l[kBcPts];
#pragma unroll
        for (int j = 0; j < kBcPts; j++) p[j] = j <= n ? src[3 * j + k] : 0.0;
        l[0] = p[0];
#pragma unroll
        for (int lev = 1; lev < kBcPts; lev++) {
#pragma unroll
            for (int i = 0; i + lev < kBcPts; i++)
                if (i + lev <= n) p[i] = (p[i] + p[i + 1]) * 0.5;
            l[lev] = p[0];
        }
#pragma unroll
        for (int j = 0; j < kBcPts; j++)
            if (j <= n) dst[3 * j + k] = side ? p[j] : l[j];
    }
    meta_out[out] = BcMeta{ M.traj, M.seg, n, 2u * M.k + side };
}

// lane b < B: the status; lane 0: stats = {rounds run, pieces examined, capped}
__global__ __launch_bounds__(256) void bc_finish_kernel(long long B, const BcTraj *__restrict__ traj, const BcCtl *__restrict__ ctl,
                                                        pct_traj_certificate *__restrict__ cert, long long *__restrict__ stats)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && stats) {
        stats[0] = ctl->rounds;
        stats[1] = (long long)ctl->pieces;
        stats[2] = ctl->capped;
    }
    if (b >= B) return;
    const BcTraj t = traj[b];
    cert[b].status = (t.flags & kBcInvalid) ? PCT_CERT_INVALID : t.hitkey != kBcNoHit ? PCT_CERT_HIT : (t.flags & kBcUndecided) ? PCT_CERT_UNDECIDED
                                                                                                                                  : PCT_CERT_FREE;
}

}  // namespace pct
