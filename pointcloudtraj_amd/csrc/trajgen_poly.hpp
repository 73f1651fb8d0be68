// trajgen_poly.hpp -- the polyhedral corridor of the trajectory generator (include/pct_trajgen.h, "Trajectory generation in
// polyhedra"): the set that trajgen.hpp's generate<Set> keeps the control points of a segment in, as half-spaces.
//
// Everything else -- the factors, the block and banded solves, the equality steps, the velocity and acceleration boxes, the
// residuals, the rho rule and the final pass -- is trajgen.hpp's, shared with the sphere form through the Set parameter.  Here:
// the planes of a candidate normalised once into LDS (16 segments x 24 planes x 32 bytes = 12 KiB behind GenCore; sizeof(PolyLds)
// is 84000 bytes, one workgroup per CU -- DESIGN section 4 says why), the exact projection of a point onto the intersection of a
// segment's half-spaces, run by the lane that owns the control point inside the projection step (no barrier of its own), and
// the slack.  Plain C++ over the HIP built-ins (tests/host/trajgen_poly_check.cpp runs the same text on the CPU).
#pragma once
#include "trajgen.hpp"

namespace pct_trajgen {

constexpr int kMaxPlanes = 24;
constexpr double kPolyAccept = 1e-9;      // a candidate may stand this far (metres) outside a plane that is not in its active set
constexpr double kPolyDet = 1e-8;         // Gram determinants below this: the pair or triple is skipped as near-parallel

__device__ inline double pdot(const double *p, const double y[3]) { return (p[0] * y[0] + p[1] * y[1]) + p[2] * y[2]; }
// how far y is outside plane q of the shrunk set (<= 0: inside); recomputed where it is needed, not kept in a per-lane array
__device__ inline double pviol(const double *pl, int q, double two_eps, const double y[3]) { return pdot(pl + 4 * q, y) - (pl[4 * q + 3] - two_eps); }

// The largest violation of y over the planes other than i, j, k, given up (a value >= stop is returned) once it reaches stop.
__device__ inline double poly_worst(const double *pl, int cnt, double two_eps, const double y[3], int i, int j, int k, double stop)
{
    double w = -INFINITY;
    for (int q = 0; q < cnt; q++) {
        if (q == i || q == j || q == k) continue;
        const double g = pviol(pl, q, two_eps, y);
        if (g > w) {
            w = g;
            if (w >= stop) return w;
        }
    }
    return w;
}

// z = the point of { y : nh_q . y <= o_q - two_eps, q < cnt } nearest v; pl holds nh0 nh1 nh2 o per plane.  The header pins the order:
// v itself; then the active sets of one, two and three planes in ascending order, the first whose multipliers are >= 0 and whose
// point is within kPolyAccept of every other plane; else the candidate with the smallest worst violation (a later candidate takes
// the place of the kept one only when it is better by more than kPolyAccept, so that rounding does not decide between equals).
__device__ inline void poly_project(const double *pl, int cnt, double two_eps, const double v[3], double z[3])
{
    bool inside = true;
    for (int q = 0; q < cnt; q++)
        if (pviol(pl, q, two_eps, v) > 0.0) inside = false;
    z[0] = v[0]; z[1] = v[1]; z[2] = v[2];
    if (inside) return;
    double best = INFINITY;
    for (int i = 0; i < cnt; i++) {
        const double gi = pviol(pl, i, two_eps, v);
        if (!(gi >= 0.0)) continue;
        const double *ni = pl + 4 * i;
        const double y[3] = {v[0] - gi * ni[0], v[1] - gi * ni[1], v[2] - gi * ni[2]};
        const double w = poly_worst(pl, cnt, two_eps, y, i, -1, -1, best - kPolyAccept);
        if (w < best - kPolyAccept) {
            best = w; z[0] = y[0]; z[1] = y[1]; z[2] = y[2];
            if (w <= kPolyAccept) return;
        }
    }
    for (int i = 0; i < cnt; i++) {
        const double gi = pviol(pl, i, two_eps, v);
        for (int j = i + 1; j < cnt; j++) {
            const double *ni = pl + 4 * i, *nj = pl + 4 * j;
            const double a = pdot(ni, nj), det = 1.0 - a * a;
            if (!(det >= kPolyDet)) continue;
            const double gj = pviol(pl, j, two_eps, v);
            const double li = (gi - a * gj) / det, lj = (gj - a * gi) / det;
            if (!(li >= 0.0 && lj >= 0.0)) continue;
            double y[3];
            for (int c = 0; c < 3; c++) y[c] = (v[c] - li * ni[c]) - lj * nj[c];
            const double w = poly_worst(pl, cnt, two_eps, y, i, j, -1, best - kPolyAccept);
            if (w < best - kPolyAccept) {
                best = w; z[0] = y[0]; z[1] = y[1]; z[2] = y[2];
                if (w <= kPolyAccept) return;
            }
        }
    }
    for (int i = 0; i < cnt; i++) {
        const double gi = pviol(pl, i, two_eps, v);
        for (int j = i + 1; j < cnt; j++) {
            const double *ni = pl + 4 * i, *nj = pl + 4 * j;
            const double a = pdot(ni, nj);
            if (!(1.0 - a * a >= kPolyDet)) continue;
            const double gj = pviol(pl, j, two_eps, v);
            for (int k = j + 1; k < cnt; k++) {
                const double *nk = pl + 4 * k;
                const double b = pdot(ni, nk), c = pdot(nj, nk);
                const double det = ((1.0 + 2.0 * ((a * b) * c)) - (a * a + b * b)) - c * c;
                if (!(det >= kPolyDet)) continue;
                const double gk = pviol(pl, k, two_eps, v);
                // the adjugate of [[1 a b] [a 1 c] [b c 1]] on (g_i, g_j, g_k)
                const double li = (((1.0 - c * c) * gi + (b * c - a) * gj) + (a * c - b) * gk) / det;
                const double lj = (((b * c - a) * gi + (1.0 - b * b) * gj) + (a * b - c) * gk) / det;
                const double lk = (((a * c - b) * gi + (a * b - c) * gj) + (1.0 - a * a) * gk) / det;
                if (!(li >= 0.0 && lj >= 0.0 && lk >= 0.0)) continue;
                double y[3];
                for (int d = 0; d < 3; d++) y[d] = ((v[d] - li * ni[d]) - lj * nj[d]) - lk * nk[d];
                const double w = poly_worst(pl, cnt, two_eps, y, i, j, k, best - kPolyAccept);
                if (w < best - kPolyAccept) {
                    best = w; z[0] = y[0]; z[1] = y[1]; z[2] = y[2];
                    if (w <= kPolyAccept) return;
                }
            }
        }
    }
}

struct PolySet {
    using Batch = pct_trajgen_poly_batch;
    struct Data {
        double pl[kMaxSeg * kMaxPlanes * 4];      // nh0 nh1 nh2 o, o = off / |n| - margin
        double anc[3 * kMaxSeg];
        int cnt[kMaxSeg];
    };

    __device__ static bool bad(const Batch &in, int64_t g, const pct_trajgen_params &)
    {
        if (!(isfinite(in.anchors[3 * g]) && isfinite(in.anchors[3 * g + 1]) && isfinite(in.anchors[3 * g + 2]))) return true;
        const int64_t p0 = in.plane_offsets[g], p1 = in.plane_offsets[g + 1];
        if (p1 < p0 || p1 - p0 > kMaxPlanes) return true;
        for (int64_t q = p0; q < p1; q++) {
            const double *p = in.planes + 4 * q;
            const double len = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
            if (!(isfinite(len) && len > 0.0 && isfinite(p[3]))) return true;
        }
        return false;
    }
    __device__ static void load(Data &D, const Batch &in, int64_t s0, int m, const pct_trajgen_params &prm)
    {
        const int tid = (int)threadIdx.x;
        if (tid < m) {
            const int64_t g = s0 + tid;
            D.cnt[tid] = (int)(in.plane_offsets[g + 1] - in.plane_offsets[g]);
            D.anc[3 * tid] = in.anchors[3 * g]; D.anc[3 * tid + 1] = in.anchors[3 * g + 1]; D.anc[3 * tid + 2] = in.anchors[3 * g + 2];
        }
        for (int e = tid; e < m * kMaxPlanes; e += kThreads) {
            const int s = e / kMaxPlanes, q = e % kMaxPlanes;
            const int64_t p0 = in.plane_offsets[s0 + s];
            if (q >= (int)(in.plane_offsets[s0 + s + 1] - p0)) continue;
            const double *p = in.planes + 4 * (p0 + q);
            const double len = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
            double *o = D.pl + 4 * e;
            o[0] = p[0] / len; o[1] = p[1] / len; o[2] = p[2] / len;
            o[3] = p[3] / len - prm.margin;
        }
    }
    __device__ static double start(const Data &D, int s, int a) { return D.anc[3 * s + a]; }
    __device__ static void project(const Data &D, int s, double eps, const double v[3], double z[3])
    {
        poly_project(D.pl + 4 * kMaxPlanes * s, D.cnt[s], 2.0 * eps, v, z);
    }
    __device__ static double slack(const Data &D, int s, const double p[3])
    {
        double sl = INFINITY;
        for (int q = 0; q < D.cnt[s]; q++) {
            const double *pq = D.pl + 4 * (kMaxPlanes * s + q);
            const double d = pq[3] - pdot(pq, p);
            sl = (d < sl || d != d) ? d : sl;
        }
        return sl;
    }
};

using PolyLds = Lds<PolySet>;
static_assert(sizeof(PolyLds) == 84000, "DESIGN section 4 states this size");

__global__ __launch_bounds__(kThreads) void trajgen_poly_kernel(pct_trajgen_poly_batch in, pct_trajgen_params prm, double *__restrict__ polycoef,
                                                                int64_t row_stride, pct_trajgen_result *__restrict__ res)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    generate<PolySet>(*reinterpret_cast<PolyLds *>(smem), in, prm, polycoef, row_stride, res);
}

}  // namespace pct_trajgen
