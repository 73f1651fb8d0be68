// bernstein.hpp -- the planner arithmetic the engine states ONCE, for its kernels and for its host code: the powers and binomials of a
// Bernstein term (traj.hip shares these two), the soundness test of a trajectory's segments, the reference's sample enumeration,
// getPosFromBezier as one thread and as one block compute it, and the radiusSearch inflation rule.  Everything is fp64 without
// contraction, so the host and the device give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace pct {

// x^n for a small non-negative integer n, CORRECTLY ROUNDED: repeated multiplication in double-double with error-free products
// (p + e = hi * x exactly through one FMA), renormalised after every step; the accumulated error stays below 2^-100 of the value,
// so the returned double is the nearest one to the exact power.  The reference evaluates its Bernstein terms with libm's
// pow(u, j) (sim_planning_demo.cpp:715-727), which is correctly rounded on glibc >= 2.28 except within ~2^-15 ulp of a rounding
// boundary; ocml's pow (the device's) is not -- with it 5-10 % of the sampled positions differed from the host's in the last bit.
// (The explicit FMAs are intended: -ffp-contract=off only forbids the compiler from fusing on its own.)
__host__ __device__ __forceinline__ double pow_uint_cr(double x, int n)
{
    if (n <= 0) return 1.0;
    double hi = x, lo = 0.0;
    for (int i = 1; i < n; i++) {
        const double p = hi * x;
        const double e = __builtin_fma(hi, x, -p);
        const double l = __builtin_fma(lo, x, e);
        const double s = p + l;
        lo = l - (s - p);
        hi = s;
    }
    return hi;
}

// n choose j as an exact double by the multiplicative recurrence (bezier_base.cpp:33-48 / :256-266 hold them as doubles computed from
// integer factorials; every intermediate here is an integer below 2^53, the rounding guard only absorbs the division).  The ONE
// definition every Bernstein evaluator of the engine uses; pinned against the reference's compiled table (tests/golden/binomials.npz).
__host__ __device__ __forceinline__ double bernstein_binom(int n, int j)
{
    double b = 1.0;
    for (int i = 1; i <= j; i++) b = floor(b * (double)(n - i + 1) / (double)i + 0.5);
    return b;
}

// ---- orders and segment ranges -----------------------------------------------------------------------------------------------------
constexpr int kMaxBezierOrder = 12;

// a segment the evaluators accept: order 0..12 and a row that holds its 3 * (order + 1) coefficients
__host__ __device__ __forceinline__ bool bezier_order_ok(int order, long long row_stride)
{
    return order >= 0 && order <= kMaxBezierOrder && 3ll * (order + 1) <= row_stride;
}

// segments [s0, s1) of trajectory b of a pct_bezier_batch, or false when the range is empty, descending or outside [0, seg_offsets[B]]
// or a segment fails bezier_order_ok: none of such a trajectory's rows is read (the batched check reports nsamples = -1, the certified
// check INVALID)
__host__ __device__ __forceinline__ bool bezier_range_sound(const int32_t *__restrict__ seg_offsets, const int32_t *__restrict__ orders,
                                                            long long row_stride, long long B, long long b, int &s0, int &s1)
{
    s0 = seg_offsets[b];
    s1 = seg_offsets[b + 1];
    if (s0 < 0 || s1 <= s0 || s1 > seg_offsets[B]) return false;
    for (int i = s0; i < s1; i++)
        if (!bezier_order_ok(orders[i], row_stride)) return false;
    return true;
}

// ---- the sample enumeration (checkSafeTrajectory, sim_planning_demo.cpp:729-771) ---------------------------------------------------
// the segment of [s0, s1) that holds t_start, and in t_s the time into it: the reference's segment search with its strict `>`
__host__ __device__ __forceinline__ int bezier_first_segment(const double *__restrict__ seg_time, int s0, int s1, double t_start, double &t_s)
{
    t_s = t_start;
    int first;
    for (first = s0; first < s1; ++first) {
        if (t_s > seg_time[first] && first + 1 < s1) t_s -= seg_time[first];
        else break;
    }
    return first;
}

constexpr long long kBezierNoBound = -1;      // `bound` of a caller whose loop needs no limit

// The reference's nested loops over the segments [s0, s1) of one trajectory, with their sequential fp64 additions t += dt and
// t_accu += dt.  emit(k, t, segment) for the samples k < room; FILL stops once they are out.  Returns the unclipped count, or -1 when
// more than `bound` samples come (bound >= 0): the loop then ends there, whatever dt and the segment times are.  The reference leaves
// only the inner loop when t_accu passes stop_time; t_accu never shrinks (dt > 0), so no later segment yields a sample and returning at
// once counts the same.
template <bool FILL, typename Emit>
__host__ __device__ __forceinline__ long long bezier_enumerate(const double *__restrict__ seg_time, int s0, int s1, double t_start,
                                                               double stop_time, double dt, long long room, long long bound, Emit emit)
{
    double t_s;
    const int first = bezier_first_segment(seg_time, s0, s1, t_start, t_s);
    long long n = 0;
    double t_accu = 0.0;
    for (int i = first; i < s1; i++) {
        const double T = seg_time[i];
        for (double t = (i == first) ? t_s : 0.0; t < T; t += dt) {
            t_accu += dt;
            if (t_accu > stop_time) return n;
            if (FILL && n >= room) return n;
            if (bound >= 0 && n >= bound) return -1;
            if (n < room) emit(n, t, i);
            n++;
        }
    }
    return n;
}

// ---- getPosFromBezier (sim_planning_demo.cpp:715-727, scaled by the segment time as :752-753) --------------------------------------
// One thread: out[d] = (sum over j ascending of ((C(order, j) * c[d*m + j]) * u^j) * (1 - u)^(order - j)) * T for the segment's row c,
// m = order + 1.  The binomials are exact doubles (bezier_base.cpp:33-48 computes them with integer factorials).
__host__ __device__ __forceinline__ void bezier_point(const double *__restrict__ row, int order, double T, double u, double out[3])
{
    const int m = order + 1;
    double binom[kMaxBezierOrder + 1];
    for (int j = 0; j <= order; j++) binom[j] = bernstein_binom(order, j);
    for (int d = 0; d < 3; d++) {
        double acc = 0.0;
        for (int j = 0; j < m; j++) acc += binom[j] * row[d * m + j] * pow_uint_cr(u, j) * pow_uint_cr(1.0 - u, order - j);
        out[d] = acc * T;
    }
}

// One block: a thread per Bernstein term (two powers each) into s_term[3 * (kMaxBezierOrder + 1)], then three threads sum the terms of
// their axis in the reference's j order into s_pos[3]; every thread of the block calls it and reads s_pos behind its last barrier.
__device__ __forceinline__ void bezier_point_block(const double *__restrict__ row, int order, double T, double u, double *s_term, double *s_pos)
{
    const int m = order + 1;
    if ((int)threadIdx.x < 3 * m) {
        const int d = (int)threadIdx.x / m, j = (int)threadIdx.x % m;
        const double c = row[d * m + j];      // first: the row may lie in host-mapped memory, and the bus read then runs beside the rest
        s_term[d * m + j] = bernstein_binom(order, j) * c * pow_uint_cr(u, j) * pow_uint_cr(1.0 - u, order - j);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (int j = 0; j < m; j++) acc += s_term[threadIdx.x * m + j];
        s_pos[threadIdx.x] = acc * T;
    }
    __syncthreads();
}

// ---- the inflation rule of radiusSearch (corridor_finder.cpp:113-133) ---------------------------------------------------------------
struct InflateParams { double sx, sy, sz, sample_range, search_margin, max_radius; };

// the early-out (:115-116), in fp64 on the planner's Vector3d before the query is narrowed to fp32: getDis(p, start) beyond reach
__host__ __device__ __forceinline__ bool inflate_skips(const InflateParams &P, double px, double py, double pz)
{
    const double dx = px - P.sx, dy = py - P.sy, dz = pz - P.sz;
    return sqrt(dx * dx + dy * dy + dz * dz) > P.sample_range + P.max_radius;
}

// the radius of a point the early-out skipped, or of any point against an empty cloud (with it: no index, d2 = +inf)
__host__ __device__ __forceinline__ double inflate_skipped_radius(const InflateParams &P) { return P.max_radius - P.search_margin; }

// :130-132: min(sqrt(d2) - search_margin, max_radius) of the nearest obstacle's d2; a NaN becomes max_radius
__host__ __device__ __forceinline__ double inflate_radius(const InflateParams &P, double d2)
{
    const double rr = sqrt(d2) - P.search_margin;
    return rr < P.max_radius ? rr : P.max_radius;
}

}  // namespace pct
