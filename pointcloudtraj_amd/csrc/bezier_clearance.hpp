// bezier_clearance.hpp -- the trajectory clearance: each curve's distance to the cloud bracketed by subdivision
// (pct_bezier_clearance_batch*, contract in include/pct_engine.h, paragraph "Trajectory clearance"; included by engine.hip behind
// bezier_certify.hpp, whose pieces, seed, validity, compaction and halving it uses as they are).
//
// The certified check asks of a piece "is a row within the margin?" through the capsule count.  This call asks for a number and takes
// it from the two nearest-neighbour answers at the ends of the piece: hi, the smallest end distance seen so far, bounds the clearance
// from above, and L below bounds it from below on the piece.  A piece whose L is within tol of hi (or beyond cap) retires; the others
// are halved.  No capsule search is involved, so every index that answers a nearest-neighbour batch serves the call.
//   cl_init_kernel      a lane per trajectory: the record's defaults, the trajectory's state, the call's control words
//   bc_valid_kernel, bc_seed_kernel (bezier_certify.hpp); the window forms: bc_window_kernel and bc_seed_window_kernel in the seed's place
//   -- per round --
//   cl_geometry_kernel  a lane per piece: a, b (fp32) as the two queries, and ell, rho, cmax into the piece scalars; a dead slot poses
//                       NaN queries
//   (engine.hip)        the nearest-neighbour batch on the path `algo` selects
//   cl_fold_kernel      a lane per piece: pieces and depth of its trajectory, both end d2 into U2 (atomicMin on the bit pattern)
//   cl_attain_kernel    a lane per piece, behind the whole fold: where U2 fell in this round, the ends that equal it offer
//                       2 * slot + end (atomicMin): the lowest (segment, u) of the round; U2 unchanged keeps the earlier round's end
//   cl_mark_kernel      a lane per piece: the winner writes the at_* fields; L; retire (fold L into lo), OPEN (fold, flag) or split; the
//                       ranks of the splitting pieces inside their tile of 256 and the tile's total
//   scan_tile_sums_kernel with BcScanDone (scan.hpp, bezier_certify.hpp): the next live count, or the capped flag
//   cl_capped_kernel    a lane per piece: in a capped round every would-be splitter folds its L into lo
//   bc_split_kernel     (bezier_certify.hpp) the halving; in a capped round it marks the owners (kBcUndecided = OPEN here)
//   -- behind the last round --
//   cl_finish_kernel    a lane per trajectory: status, lo, hi; lane 0: the call's stats
// Host and device form differ as in the certified check: the first reads the live count once per round, the second runs
// max_depth + 1 rounds over piece_cap slots whose lanes guard on the device-side count.  Same bytes.
//
// WHAT lo PROVES, and the slack in L.  Let P be the fp64 polygon of a piece as stored, C its exact curve, a and b its chord ends as
// the searches see them (fp32), e = b - a, and da*, db*, ell*, rho* the exact values of which da, db, ell, rho are the computed ones.
// (1) Every point x of C is within rho* of a chord point a + s*e ((1) of bezier_certify.hpp), so |x - a| <= rho* + s*ell* and
//     |x - b| <= rho* + (1 - s)*ell*.  The distance d(.) to the nearest row is 1-Lipschitz: d(x) >= max(da* - s*ell*,
//     db* - (1 - s)*ell*) - rho* >= (da* + db* - ell*) / 2 - rho*, the two arguments of the max crossing at their mean.
// (2) Roundings local to the piece.  A nearest-neighbour d2 is the minimum of ((dx*dx + dy*dy) + dz*dz) over the rows: each within a
//     relative 2^-51 of the exact square (the differences of fp32 values round once, nothing underflows: a difference of fp32
//     denormals squared is above 2^-300), and so is their minimum against the exact minimum; sqrt halves that and rounds once:
//     |da - da*| <= 2^-51 * da*, the same for db and, by the same count, for ell.  The two sums, the halving (exact) and the
//     subtraction of rho add 3 * 2^-53 of their results: the computed t = ((da + db) - ell) * 0.5 - rho is off the same expression
//     in da*, db*, ell* and the computed rho by at most 2^-50 * (da + db + ell + rho).  rho* <= rho * (1 + 2^-49) + 2^-48 * cmax
//     ((2) of bezier_certify.hpp).  The slack S = ((da + db) + ell + rho) * 2^-20 + cmax * 2^-40 is itself within a relative 2^-51,
//     and t - S rounds once more, by at most 2^-54 * (da + db).  Together
//         L <= (da* + db* - ell*) / 2 - rho* - [ (da + db + ell + rho) * (2^-20 - 2^-48) + cmax * (2^-40 - 2^-47) ]:
//     the piece-local roundings are covered unconditionally, with the bracket to spare.
// (3) The inherited error.  By (4) of bezier_certify.hpp, C differs from the true curve of the segment on the piece's interval by at
//     most E < 2^-45 * M0, M0 the largest |world control coordinate| of the segment, after up to 20 halvings.  d is 1-Lipschitz,
//     so the true curve's clearance on the interval is at least that of C minus E.  The spare of (2) covers E when
//     cmax >= M0 / 16, and otherwise when da + db + ell + rho >= 2^-24 * M0 -- 60 micrometres per kilometre of |coordinate|.
//     Under that condition lo is a proof: no point of the curve is nearer than lo to any row of the window.  Below it (a piece
//     within micrometres of a row and far nearer the origin than its curve reaches) L is itself below 2^-25 * M0 and may exceed
//     the truth by at most E; no claim is made there.
// (4) Windows.  A first piece cut by bc_seed_window_kernel adds to E as (5) of bezier_certify.hpp counts it: E <= 348 * 2^-53 * M0
//     < 0.68 * 2^-44 * M0.  The spare of (2) covers that under the same condition as (3): cmax >= M0 / 16 gives
//     cmax * (2^-40 - 2^-47) >= 0.99 * 2^-44 * M0, and da + db + ell + rho >= 2^-24 * M0 gives (2^-20 - 2^-48) * 2^-24 * M0.  lo of a
//     window form is then a proof for the points with u in [u0, u1] of every segment the window touches.  L is unchanged.
// hi needs no argument: it is the distance the sampled check would measure at a point it could have sampled (an end of a piece,
// a curve point rounded to fp32).
// The slack is about 2^-20 of twice the distance: a tol below ~ 2 * d * 1e-6 cannot be met and ends OPEN at max_depth.
#pragma once
#include "bezier_certify.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr int kClGeom = 4;      // doubles per piece in the piece scalars: ell, rho, cmax, and L once cl_mark_kernel has it

// a trajectory's running minima as bit patterns of doubles >= 0 (their order as unsigned integers is the order of the values)
struct ClTraj {
    unsigned long long u2;         // U2: the smallest end d2 examined so far
    unsigned long long u2_seen;    // U2 as of the round that named the attaining end
    unsigned long long lo;         // the smallest L folded so far
};

__device__ __forceinline__ unsigned long long cl_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double cl_value(unsigned long long b) { return __longlong_as_double((long long)b); }

// The bound of the contract, in its order of operations.
__device__ __forceinline__ double cl_lower(double da, double db, double ell, double rho, double cmax)
{
    if (!(da <= 1.7976931348623157e308) || !(db <= 1.7976931348623157e308)) return __builtin_huge_val();      // a d2 of +inf
    const double sum = da + db;
    const double t = ((sum - ell) * 0.5 - rho) - (((sum + ell) + rho) * 0x1p-20 + cmax * 0x1p-40);
    return t > 0.0 ? t : 0.0;
}

// lane b < B: record defaults and state; lane B: the control words
__global__ __launch_bounds__(256) void cl_init_kernel(BcDesc D, long long piece_cap, pct_traj_clearance *__restrict__ out, BcTraj *__restrict__ traj,
                                                      BcCtl *__restrict__ ctl, ClTraj *__restrict__ st)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > D.B) return;
    if (!bc_init_state(D, piece_cap, b, traj, ctl)) return;
    const unsigned long long inf = cl_bits(__builtin_huge_val());
    st[b] = ClTraj{ inf, inf, inf };
    out[b].status = PCT_CLR_DONE;
    out[b].depth = 0;
    out[b].at_seg = -1;
    out[b].at_idx = PCT_NO_INDEX;
    out[b].at_u = __builtin_nan("");
    out[b].lo = __builtin_huge_val();
    out[b].hi = __builtin_huge_val();
    out[b].pieces = 0;
}

// lane slot < nslots: the two queries and the scalars of a live piece; NaN queries for any other slot
__global__ __launch_bounds__(256) void cl_geometry_kernel(const double *__restrict__ poly, const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl,
                                                          uint32_t nslots, double *__restrict__ geom, float *__restrict__ q)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots) return;
    float *qq = q + 6 * (size_t)slot;
    double *g = geom + kClGeom * (size_t)slot;
    if (slot >= ctl->live || meta[slot].traj < 0) {
        for (int k = 0; k < 6; k++) qq[k] = __builtin_nanf("");
        for (int k = 0; k < kClGeom; k++) g[k] = 0.0;
        return;
    }
    double ends[6], rho, cmax;
    bc_chord(poly + (size_t)slot * kBcPoly, meta[slot].order, qq, ends, rho, cmax);
    const double e0 = ends[3] - ends[0], e1 = ends[4] - ends[1], e2 = ends[5] - ends[2];
    g[0] = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    g[1] = rho;
    g[2] = cmax;
    g[3] = 0.0;
}

// lane slot < nslots: a live piece adds itself to its trajectory and to the call and folds its two end d2 into U2
__global__ __launch_bounds__(256) void cl_fold_kernel(const BcMeta *__restrict__ meta, BcCtl *__restrict__ ctl, uint32_t nslots, int round,
                                                      const double *__restrict__ nn_d2, pct_traj_clearance *__restrict__ out, ClTraj *__restrict__ st)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots || slot >= ctl->live || meta[slot].traj < 0) return;
    const int b = meta[slot].traj;
    atomicAdd(reinterpret_cast<unsigned long long *>(&out[b].pieces), 1ull);
    atomicAdd(&ctl->pieces, 1ull);
    out[b].depth = round;                                     // every live piece of the round stores the same value
    ctl->examined = 1u;
    const double da = nn_d2[2 * (size_t)slot], db = nn_d2[2 * (size_t)slot + 1];
    atomicMin(&st[b].u2, cl_bits(da < db ? da : db));
}

// lane slot < nslots, behind the whole fold: U2 fell in this round -> the ends that attain it offer themselves, the lowest wins
__global__ __launch_bounds__(256) void cl_attain_kernel(const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl, uint32_t nslots,
                                                        const double *__restrict__ nn_d2, const ClTraj *__restrict__ st, BcTraj *__restrict__ traj)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots || slot >= ctl->live || meta[slot].traj < 0) return;
    const int b = meta[slot].traj;
    const unsigned long long u2 = st[b].u2;
    if (u2 >= st[b].u2_seen) return;                          // an equal d2 of a later round does not displace the earlier end
    if (cl_bits(nn_d2[2 * (size_t)slot]) == u2) atomicMin(&traj[b].hitkey, 2u * slot);
    else if (cl_bits(nn_d2[2 * (size_t)slot + 1]) == u2) atomicMin(&traj[b].hitkey, 2u * slot + 1u);
}

// One tile of kBcTile slots per block, behind cl_attain_kernel.  flag out: 1 + the rank of a splitting piece inside its tile, 0 for
// every other slot; tile_sum[block] = the tile's splitting pieces; geom[.][3] = L of a splitting piece.  kWindow: at_u goes through
// win[] (the window forms, bc_window_u).
template <bool kWindow>
__global__ __launch_bounds__(kBcTile) void cl_mark_kernel(const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl, uint32_t nslots, int round,
                                                          int max_depth, double tol, double cap, const uint32_t *__restrict__ nn_idx,
                                                          const double *__restrict__ nn_d2, double *__restrict__ geom,
                                                          pct_traj_clearance *__restrict__ out, BcTraj *__restrict__ traj, ClTraj *__restrict__ st,
                                                          uint32_t *__restrict__ flag, uint32_t *__restrict__ tile_sum,
                                                          const double *__restrict__ win)
{
    const uint32_t slot = blockIdx.x * kBcTile + threadIdx.x;
    uint32_t split = 0;
    if (slot < nslots && slot < ctl->live && meta[slot].traj >= 0) {
        const BcMeta M = meta[slot];
        const unsigned long long u2 = st[M.traj].u2;
        const uint32_t key = traj[M.traj].hitkey;
        if ((key >> 1) == slot) {                             // this piece holds the end that attains the new U2; no other lane matches
            const uint32_t end = key & 1u;
            out[M.traj].at_seg = M.seg;
            out[M.traj].at_idx = nn_idx[key];
            const double v = ldexp((double)(M.k + end), -round);
            out[M.traj].at_u = kWindow ? bc_window_u(win, M.seg, v) : v;
            st[M.traj].u2_seen = u2;
            traj[M.traj].hitkey = kBcNoHit;                   // the next round's offers start afresh
        }
        double *g = geom + kClGeom * (size_t)slot;
        const double L = cl_lower(sqrt(nn_d2[2 * (size_t)slot]), sqrt(nn_d2[2 * (size_t)slot + 1]), g[0], g[1], g[2]);
        const double h = sqrt(cl_value(u2));
        if (L >= (h < cap ? h : cap) - tol) {
            atomicMin(&st[M.traj].lo, cl_bits(L));
        } else if (round >= max_depth || (g[0] == 0.0 && g[1] == 0.0)) {      // at the depth limit, or a single point: halving cannot improve it
            atomicMin(&st[M.traj].lo, cl_bits(L));
            atomicOr(&traj[M.traj].flags, kBcUndecided);
        } else {
            split = 1;
            g[3] = L;
        }
    }
    uint32_t total;
    const uint32_t rank = block_exclusive<uint32_t, kBcTile>(split, total);
    if (slot < nslots) flag[slot] = split ? rank + 1u : 0u;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// lane slot < nslots, behind the scan: in a round whose splits piece_cap refused, every would-be splitter folds its L
// (bc_split_kernel marks the owners)
__global__ __launch_bounds__(256) void cl_capped_kernel(const BcMeta *__restrict__ meta, const BcCtl *__restrict__ ctl, uint32_t nslots,
                                                        const uint32_t *__restrict__ flag, const double *__restrict__ geom, BcTraj *__restrict__ traj,
                                                        ClTraj *__restrict__ st)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nslots || !ctl->capped_now || !flag[slot]) return;
    const int b = meta[slot].traj;
    atomicMin(&st[b].lo, cl_bits(geom[kClGeom * (size_t)slot + 3]));
    atomicOr(&traj[b].flags, kBcUndecided);
}

// lane b < B: status, lo and hi; lane 0: stats = {rounds run, pieces examined, capped}
__global__ __launch_bounds__(256) void cl_finish_kernel(long long B, const BcTraj *__restrict__ traj, const BcCtl *__restrict__ ctl,
                                                        const ClTraj *__restrict__ st, pct_traj_clearance *__restrict__ out,
                                                        long long *__restrict__ stats)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && stats) {
        stats[0] = ctl->rounds;
        stats[1] = (long long)ctl->pieces;
        stats[2] = ctl->capped;
    }
    if (b >= B) return;
    const uint32_t f = traj[b].flags;
    if (f & kBcInvalid) {
        out[b].status = PCT_CLR_INVALID;
        out[b].lo = __builtin_nan("");
        out[b].hi = __builtin_nan("");
        return;
    }
    const double hi = sqrt(cl_value(st[b].u2)), lo = cl_value(st[b].lo);
    out[b].status = (f & kBcUndecided) ? PCT_CLR_OPEN : PCT_CLR_DONE;
    out[b].hi = hi;
    out[b].lo = lo < hi ? lo : hi;
}

}  // namespace pct
