// trajgen.hpp -- the kernel of the trajectory generator (include/pct_trajgen.h); trajgen.hip holds the host side.
//
// One workgroup of 256 lanes per candidate; the whole problem and every iterate live in LDS (sizeof(GenLds), about 72 KiB, asked
// for as dynamic LDS: two candidates fit the 160 KiB of a CU).  What makes that possible: H = Q + rho A^T A is block diagonal with
// one (n+1) x (n+1) block per segment and the same for the three axes, and the equalities couple neighbouring segments only, so
// their Schur complement S = E H^-1 E^T has half bandwidth 5.  Storage is one stride-13 slot per control point, [axis][segment][13].
// An iteration is seven barriers: right-hand side, block solves, E w - b, the banded solve, E^T nu, block solves, projections.
// fp64 throughout, -ffp-contract=off; every reduction is a max or runs in a fixed order, so a candidate's bytes do not depend on
// the batch around it.  Plain C++ over the HIP built-ins only (tests/host/trajgen_check.cpp runs the same text on the CPU).
// The body is generate<Set>: the set the control points of a segment are kept in -- a ball (BallSet, here) or a polytope (PolySet,
// trajgen_poly.hpp) -- supplies its LDS arrays and five steps; everything else is one text for both.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/pct_trajgen.h"

namespace pct_trajgen {

constexpr int kMinOrder = 5, kMaxOrder = 12, kMaxSeg = 16;
constexpr int kSlot = kMaxOrder + 1;             // control points per segment slot
constexpr int kRows = kMaxSeg * kSlot;           // 208 slots per axis
constexpr int kTri = kSlot * (kSlot + 1) / 2;    // packed lower triangle of a block
constexpr int kMaxEq = 3 * (kMaxSeg + 1);        // equalities per axis
constexpr int kBand = 6;                         // diagonal + half bandwidth 5
constexpr int kThreads = 256;
constexpr double kAlpha = 1.6, kRhoAuto = 1e-5, kRhoMin = 1e-9, kRhoMax = 1e3, kRhoStep = 5.0;

// What every constraint set shares; Lds<Set> adds the set's own arrays behind it.
struct __attribute__((aligned(16))) GenCore {
    double Lf[kMaxSeg * kTri];        // Cholesky factors of the blocks of H (packed rows)
    double Qm[kMaxSeg * kTri];        // the blocks of Q = P / max|P|
    double Sb[kMaxEq * kBand];        // banded Cholesky factor of S: Sb[r][j] = L[r][r - 5 + j]
    double x[3 * kRows], t[3 * kRows];
    double z1[3 * kRows], u1[3 * kRows], zv[3 * kRows], uv[3 * kRows], za[3 * kRows], ua[3 * kRows];
    double nu[3 * kMaxEq], bb[3 * kMaxEq];
    double red[kThreads];
    double T[kMaxSeg], bv[kMaxSeg], ba[kMaxSeg], fv[kMaxSeg], fa[kMaxSeg];
    double gam[3 * kMaxSeg];          // gam[3 g + rt]: joint g's factor on the right segment's value / first / second difference
    int n[kMaxSeg];
};

template <class Set>
struct __attribute__((aligned(16))) Lds : GenCore {
    typename Set::Data set;
};

// The set the control points of a segment are kept in.  A set names its batch (Batch), its LDS arrays (Data) and five steps:
//   bad(in, g, prm)           lane s of the candidate: is segment g's part of the set unusable?
//   load(D, in, s0, m, prm)   all lanes: fill D (a barrier follows)
//   start(D, s, a)            the start iterate of segment s on axis a
//   project(D, s, eps, v, z)  z = the projection of v onto the set of segment s, shrunk by 2 eps
//   slack(D, s, p)            how far p is inside the set of segment s (the margin taken off, no 2 eps)
struct BallSet {
    using Batch = pct_trajgen_batch;
    struct Data { double cen[3 * kMaxSeg], rb[kMaxSeg], rfull[kMaxSeg]; };

    __device__ static bool bad(const Batch &in, int64_t g, const pct_trajgen_params &prm)
    {
        const double r = in.radius[g];
        if (!(isfinite(r) && isfinite(in.centres[3 * g]) && isfinite(in.centres[3 * g + 1]) && isfinite(in.centres[3 * g + 2]))) return true;
        return !(r - prm.margin - 2.0 * prm.eps > 0.0);
    }
    __device__ static void load(Data &D, const Batch &in, int64_t s0, int m, const pct_trajgen_params &prm)
    {
        const int tid = (int)threadIdx.x;
        if (tid >= m) return;
        const int64_t g = s0 + tid;
        const double r = in.radius[g];
        D.cen[3 * tid] = in.centres[3 * g]; D.cen[3 * tid + 1] = in.centres[3 * g + 1]; D.cen[3 * tid + 2] = in.centres[3 * g + 2];
        D.rfull[tid] = r - prm.margin;
        D.rb[tid] = r - prm.margin - 2.0 * prm.eps;
    }
    __device__ static double start(const Data &D, int s, int a) { return D.cen[3 * s + a]; }
    __device__ static void project(const Data &D, int s, double, const double v[3], double z[3])
    {
        double d[3];
        for (int a = 0; a < 3; a++) d[a] = v[a] - D.cen[3 * s + a];
        const double dist = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const bool out = dist > D.rb[s];
        const double f = out ? D.rb[s] / dist : 1.0;
        for (int a = 0; a < 3; a++) z[a] = out ? D.cen[3 * s + a] + d[a] * f : v[a];
    }
    __device__ static double slack(const Data &D, int s, const double p[3])
    {
        const double dx = p[0] - D.cen[3 * s], dy = p[1] - D.cen[3 * s + 1], dz = p[2] - D.cen[3 * s + 2];
        return D.rfull[s] - sqrt((dx * dx + dy * dy) + dz * dz);
    }
};

using GenLds = Lds<BallSet>;
static_assert(sizeof(GenLds) == 71904, "the sphere form's LDS is what it was");

__device__ inline int tri(int r, int c) { return r * (r + 1) / 2 + c; }       // r >= c

__device__ inline double binom(int n, int k)
{
    if (k < 0 || k > n) return 0.0;
    unsigned long long c = 1;
    for (int i = 1; i <= k; i++) c = c * (unsigned long long)(n - k + i) / (unsigned long long)i;     // exact: every prefix is a binomial
    return (double)c;
}

// value, first and second difference at a segment's start (pos = control point index) and at its end (pos counted back from the last)
__device__ inline double base_l(int rt, int pos) { return rt == 0 ? (pos == 0 ? 1.0 : 0.0) : rt == 1 ? (pos == 0 ? -1.0 : pos == 1 ? 1.0 : 0.0) : (pos == 1 ? -2.0 : 1.0); }
__device__ inline double base_r(int rt, int pos) { return rt == 0 ? (pos == 0 ? 1.0 : 0.0) : rt == 1 ? (pos == 0 ? 1.0 : pos == 1 ? -1.0 : 0.0) : (pos == 1 ? -2.0 : 1.0); }

// coefficient of equality row (group g, kind rt) on control point l of segment s
__device__ inline double ecoef(const GenCore &L, int m, int g, int rt, int s, int l)
{
    if (s == g - 1) {
        const int e = L.n[s] - l;
        return (e >= 0 && e <= 2) ? base_r(rt, e) : 0.0;
    }
    if (s == g && g < m) {
        if (l > 2) return 0.0;
        return (g == 0 ? 1.0 : -L.gam[3 * g + rt]) * base_l(rt, l);
    }
    return 0.0;
}

__device__ inline double block_max(GenCore &L, double v)
{
    const int tid = (int)threadIdx.x;
    L.red[tid] = v;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) L.red[tid] = fmax(L.red[tid], L.red[tid + w]);      // fmax drops a NaN: the callers carry NaN by hand where it matters
        __syncthreads();
    }
    const double r = L.red[0];
    __syncthreads();
    return r;
}

__device__ inline double block_sum(GenCore &L, double v)
{
    const int tid = (int)threadIdx.x;
    L.red[tid] = v;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) L.red[tid] = L.red[tid] + L.red[tid + w];
        __syncthreads();
    }
    const double r = L.red[0];
    __syncthreads();
    return r;
}

// A^T y at control point l of a segment of order n; y1 / yv / ya point at the segment's slot of one axis
__device__ inline double at_gather(const double *y1, const double *yv, const double *ya, int l, int n, bool use_v, bool use_a)
{
    double g = y1[l];
    if (use_v) g += (l >= 1 ? yv[l - 1] : 0.0) - (l <= n - 1 ? yv[l] : 0.0);
    if (use_a) g += ((l >= 2 ? ya[l - 2] : 0.0) - 2.0 * ((l >= 1 && l <= n - 1) ? ya[l - 1] : 0.0)) + (l <= n - 2 ? ya[l] : 0.0);
    return g;
}

// y <- (L L^T)^-1 y on one block
__device__ inline void block_solve(const double *Lf, double *y, int cnt)
{
    for (int r = 0; r < cnt; r++) {
        double acc = y[r];
        for (int c = 0; c < r; c++) acc -= Lf[tri(r, c)] * y[c];
        y[r] = acc / Lf[tri(r, r)];
    }
    for (int r = cnt - 1; r >= 0; r--) {
        double acc = y[r];
        for (int c = r + 1; c < cnt; c++) acc -= Lf[tri(c, r)] * y[c];
        y[r] = acc / Lf[tri(r, r)];
    }
}

// H = Q + rho (I + Gv^T Gv + Ga^T Ga) block by block, its Cholesky factors, S = E H^-1 E^T and its banded factor
__device__ void factor(GenCore &L, int m, double rho, bool use_v, bool use_a)
{
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < m * kTri; e += kThreads) {
        const int s = e / kTri, k = e % kTri;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= k) r++;
        const int c = k - r * (r + 1) / 2, n = L.n[s];
        double h = 0.0;
        if (r <= n) {
            double a = r == c ? 1.0 : 0.0;
            if (use_v)        // (D1^T D1)[r][c]: rows l hold -1 at l, +1 at l + 1, l = 0..n-1
                for (int l = (r >= 1 ? r - 1 : 0); l <= c && l <= n - 1; l++)
                    a += (r == l ? -1.0 : 1.0) * (c == l ? -1.0 : c == l + 1 ? 1.0 : 0.0);
            if (use_a)        // (D2^T D2)[r][c]: rows l hold 1, -2, 1 at l..l + 2, l = 0..n-2
                for (int l = (r >= 2 ? r - 2 : 0); l <= c && l <= n - 2; l++)
                    a += (r - l == 1 ? -2.0 : 1.0) * (c - l == 1 ? -2.0 : 1.0);
            h = L.Qm[e] + rho * a;
        }
        L.Lf[e] = h;
    }
    __syncthreads();
    if (tid < m) {
        double *A = L.Lf + tid * kTri;
        const int cnt = L.n[tid] + 1;
        for (int j = 0; j < cnt; j++) {
            double d = A[tri(j, j)];
            for (int k = 0; k < j; k++) d -= A[tri(j, k)] * A[tri(j, k)];
            d = sqrt(d);
            A[tri(j, j)] = d;
            for (int i = j + 1; i < cnt; i++) {
                double v = A[tri(i, j)];
                for (int k = 0; k < j; k++) v -= A[tri(i, k)] * A[tri(j, k)];
                A[tri(i, j)] = v / d;
            }
        }
    }
    __syncthreads();
    const int ne = 3 * (m + 1);
    if (tid < ne) {
        const int c = tid, gc = c / 3, rtc = c % 3;
        double y[2][kSlot];                       // H^-1 E^T e_c on segments gc - 1 and gc
        for (int part = 0; part < 2; part++) {
            const int s = gc - 1 + part;
            if (s < 0 || s >= m) continue;
            const int cnt = L.n[s] + 1;
            for (int l = 0; l < cnt; l++) y[part][l] = ecoef(L, m, gc, rtc, s, l);
            block_solve(L.Lf + s * kTri, y[part], cnt);
        }
        for (int r = c; r < ne && r <= c + 5; r++) {
            const int gr = r / 3, rtr = r % 3;
            double acc = 0.0;
            for (int part = 0; part < 2; part++) {
                const int s = gc - 1 + part;
                if (s < 0 || s >= m || (s != gr - 1 && s != gr)) continue;
                const int cnt = L.n[s] + 1;
                for (int l = 0; l < cnt; l++) acc += ecoef(L, m, gr, rtr, s, l) * y[part][l];
            }
            L.Sb[r * kBand + (c - r + 5)] = acc;
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 0; j < ne; j++) {
            double d = L.Sb[j * kBand + 5];
            for (int k = (j >= 5 ? j - 5 : 0); k < j; k++) d -= L.Sb[j * kBand + (k - j + 5)] * L.Sb[j * kBand + (k - j + 5)];
            d = sqrt(d);
            L.Sb[j * kBand + 5] = d;
            for (int i = j + 1; i < ne && i <= j + 5; i++) {
                double v = L.Sb[i * kBand + (j - i + 5)];
                for (int k = (i >= 5 ? i - 5 : 0); k < j; k++) v -= L.Sb[i * kBand + (k - i + 5)] * L.Sb[j * kBand + (k - j + 5)];
                L.Sb[i * kBand + (j - i + 5)] = v / d;
            }
        }
    }
    __syncthreads();
}

template <class Set>
__device__ inline void generate(Lds<Set> &L, const typename Set::Batch &in, const pct_trajgen_params &prm, double *__restrict__ polycoef,
                                int64_t row_stride, pct_trajgen_result *__restrict__ res)
{
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t s0 = in.seg_offsets[b], s1 = in.seg_offsets[b + 1];
    const int64_t mm = s1 - s0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int k = prm.minimize_order;
    const double eps = prm.eps;

    // ---- validate
    int bad = (mm < 1 || mm > kMaxSeg) ? 1 : 0;
    if (!bad) {
        if (tid < (int)mm) {
            const int64_t g = s0 + tid;
            const double T = in.seg_time[g];
            const int n = in.orders[g];
            if (!isfinite(T) || !(T > 0.0) || n < kMinOrder || n > kMaxOrder || n - 2 < k || 3 * (int64_t)(n + 1) > row_stride) bad = 1;
            if (Set::bad(in, g, prm)) bad = 1;
        }
        if (tid >= 64 && tid < 73 && !isfinite(in.start_state[9 * b + tid - 64])) bad = 1;
        if (tid >= 128 && tid < 137 && !isfinite(in.end_state[9 * b + tid - 128])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (mm >= 1)
            for (int64_t e = tid; e < mm * row_stride; e += kThreads) polycoef[s0 * row_stride + e] = nan;
        if (tid == 0) {
            pct_trajgen_result r;
            r.status = PCT_GEN_INVALID; r.iterations = 0;
            r.cost = r.duration = r.r_prim = r.r_dual = r.sphere_slack = r.max_vel_ctrl = r.max_acc_ctrl = nan;
            res[b] = r;
        }
        return;
    }
    const int m = (int)mm;
    const bool use_v = isfinite(prm.max_vel) && prm.max_vel > 0.0, use_a = isfinite(prm.max_acc) && prm.max_acc > 0.0;
    const bool adaptive = !(prm.rho > 0.0);

    // ---- the segments' scalars
    if (tid < m) {
        const int64_t g = s0 + tid;
        const int n = in.orders[g];
        const double T = in.seg_time[g];
        L.n[tid] = n; L.T[tid] = T;
        L.fv[tid] = (double)n / T;
        L.fa[tid] = (double)(n * (n - 1)) / (T * T);
        L.bv[tid] = use_v ? prm.max_vel / L.fv[tid] : 0.0;
        L.ba[tid] = use_a ? prm.max_acc / L.fa[tid] : 0.0;
        L.gam[3 * tid] = 1.0; L.gam[3 * tid + 1] = 1.0; L.gam[3 * tid + 2] = 1.0;
        if (tid >= 1) {
            const int np = in.orders[g - 1];
            const double Tp = in.seg_time[g - 1];
            L.gam[3 * tid + 1] = ((double)n / T) * (Tp / (double)np);
            L.gam[3 * tid + 2] = ((double)(n * (n - 1)) / (T * T)) * (Tp * Tp / (double)(np * (np - 1)));
        }
    }
    Set::load(L.set, in, s0, m, prm);
    __syncthreads();

    // ---- P = 2 T^(1-2k) M_k(n), block by block; then Q = P / max|P|
    double pmax = 0.0;
    for (int e = tid; e < m * kTri; e += kThreads) {
        const int s = e / kTri, kk = e % kTri;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= kk) r++;
        const int c = kk - r * (r + 1) / 2, n = L.n[s], q = n - k;
        double v = 0.0;
        if (r <= n) {
            // M[r][c] = f^2 sum_a sum_b D[a][r] G[a][b] D[b][c],  D[a][i] = (-1)^(k - (i - a)) C(k, i - a) for 0 <= i - a <= k
            double acc = 0.0;
            for (int a = (r - k > 0 ? r - k : 0); a <= q && a <= r; a++) {
                const double da = (((k - (r - a)) & 1) ? -1.0 : 1.0) * binom(k, r - a);
                double row = 0.0;
                for (int bb = (c - k > 0 ? c - k : 0); bb <= q && bb <= c; bb++) {
                    const double db = (((k - (c - bb)) & 1) ? -1.0 : 1.0) * binom(k, c - bb);
                    row += binom(q, a) * binom(q, bb) / binom(2 * q, a + bb) / (double)(2 * q + 1) * db;
                }
                acc += da * row;
            }
            double f = 1.0;
            for (int i = 0; i < k; i++) f *= (double)(n - i);
            double tp = 1.0;
            for (int i = 0; i < 2 * k - 1; i++) tp *= L.T[s];
            v = 2.0 / tp * (f * f * acc);
        }
        L.Qm[e] = v;
        pmax = fmax(pmax, fabs(v));
    }
    pmax = block_max(L, pmax);
    const double scale = 1.0 / pmax;
    for (int e = tid; e < m * kTri; e += kThreads) L.Qm[e] *= scale;

    // ---- right-hand sides of the equalities and the start x = the set's start iterate, z = A x, u = 0
    const int ne = 3 * (m + 1);
    for (int e = tid; e < 3 * ne; e += kThreads) {
        const int a = e / ne, row = e % ne, g = row / 3, rt = row % 3;
        double v = 0.0;
        if (g == 0) {
            const double st = in.start_state[9 * b + 3 * rt + a];
            v = rt == 0 ? st : rt == 1 ? st * (1.0 / L.fv[0]) : st * (1.0 / L.fa[0]);
        } else if (g == m) {
            const double en = in.end_state[9 * b + 3 * rt + a];
            v = rt == 0 ? en : rt == 1 ? en * (1.0 / L.fv[m - 1]) : en * (1.0 / L.fa[m - 1]);
        }
        L.bb[a * kMaxEq + row] = v;
    }
    for (int e = tid; e < 3 * kRows; e += kThreads) {
        const int a = e / kRows, s = (e % kRows) / kSlot;
        const double c = s < m ? Set::start(L.set, s, a) : 0.0;
        L.x[e] = c; L.z1[e] = c; L.u1[e] = 0.0;
        L.zv[e] = 0.0; L.uv[e] = 0.0; L.za[e] = 0.0; L.ua[e] = 0.0; L.t[e] = 0.0;
    }
    double rho = adaptive ? kRhoAuto : prm.rho;
    __syncthreads();
    factor(L, m, rho, use_v, use_a);

    // ---- the iteration
    double r_prim = INFINITY, r_dual = INFINITY;
    int it = 0;
    bool done = false;
    while (it < prm.max_iter && !done) {
        it++;
        // w = H^-1 rho A^T (z - u)
        for (int e = tid; e < 3 * kRows; e += kThreads) {
            const int s = (e % kRows) / kSlot, l = e % kSlot;
            if (s >= m || l > L.n[s]) continue;
            const int o = e - l;
            L.x[e] = rho * (at_gather(L.z1 + o, L.zv + o, L.za + o, l, L.n[s], use_v, use_a) - at_gather(L.u1 + o, L.uv + o, L.ua + o, l, L.n[s], use_v, use_a));
        }
        __syncthreads();
        if (tid < 3 * m) {
            const int a = tid / m, s = tid % m;
            block_solve(L.Lf + s * kTri, L.x + a * kRows + s * kSlot, L.n[s] + 1);
        }
        __syncthreads();
        // S nu = E w - b
        if (tid < 3 * ne) {
            const int a = tid / ne, row = tid % ne, g = row / 3, rt = row % 3;
            double acc = 0.0;
            if (g >= 1) {
                const double *w = L.x + a * kRows + (g - 1) * kSlot + L.n[g - 1];
                acc = (base_r(rt, 0) * w[0] + base_r(rt, 1) * w[-1]) + base_r(rt, 2) * w[-2];
            }
            if (g < m) {
                const double *w = L.x + a * kRows + g * kSlot;
                const double cl = g == 0 ? 1.0 : -L.gam[3 * g + rt];
                acc += cl * ((base_l(rt, 0) * w[0] + base_l(rt, 1) * w[1]) + base_l(rt, 2) * w[2]);
            }
            L.nu[a * kMaxEq + row] = acc - L.bb[a * kMaxEq + row];
        }
        __syncthreads();
        if (tid < 3) {
            double *y = L.nu + tid * kMaxEq;
            for (int r = 0; r < ne; r++) {
                double acc = y[r];
                for (int c = (r >= 5 ? r - 5 : 0); c < r; c++) acc -= L.Sb[r * kBand + (c - r + 5)] * y[c];
                y[r] = acc / L.Sb[r * kBand + 5];
            }
            for (int r = ne - 1; r >= 0; r--) {
                double acc = y[r];
                for (int c = r + 1; c < ne && c <= r + 5; c++) acc -= L.Sb[c * kBand + (r - c + 5)] * y[c];
                y[r] = acc / L.Sb[r * kBand + 5];
            }
        }
        __syncthreads();
        // x = w - H^-1 E^T nu
        for (int e = tid; e < 3 * kRows; e += kThreads) {
            const int a = e / kRows, s = (e % kRows) / kSlot, l = e % kSlot;
            if (s >= m || l > L.n[s]) continue;
            const double *nu = L.nu + a * kMaxEq;
            double acc = 0.0;
            if (l <= 2) {
                const int g = s;
                for (int rt = 0; rt < 3; rt++) acc += (g == 0 ? 1.0 : -L.gam[3 * g + rt]) * base_l(rt, l) * nu[3 * g + rt];
            }
            const int back = L.n[s] - l;
            if (back <= 2)
                for (int rt = 0; rt < 3; rt++) acc += base_r(rt, back) * nu[3 * (s + 1) + rt];
            L.t[e] = acc;
        }
        __syncthreads();
        if (tid < 3 * m) {
            const int a = tid / m, s = tid % m, o = a * kRows + s * kSlot;
            block_solve(L.Lf + s * kTri, L.t + o, L.n[s] + 1);
            for (int l = 0; l <= L.n[s]; l++) L.x[o + l] -= L.t[o + l];
        }
        __syncthreads();
        const bool check = it % prm.check_every == 0 || it == prm.max_iter;
        if (check) {      // A^T z before the projection, for the dual residual
            for (int e = tid; e < 3 * kRows; e += kThreads) {
                const int s = (e % kRows) / kSlot, l = e % kSlot;
                if (s >= m || l > L.n[s]) continue;
                const int o = e - l;
                L.t[e] = at_gather(L.z1 + o, L.zv + o, L.za + o, l, L.n[s], use_v, use_a);
            }
            __syncthreads();
        }
        // z = projection of alpha A x + (1 - alpha) z + u, u = what the projection took off
        double rp = 0.0, nax = 0.0, nz = 0.0;
        if (tid < kRows) {
            const int s = tid / kSlot, l = tid % kSlot;
            if (s < m && l <= L.n[s]) {
                double v[3], zp[3];
                for (int a = 0; a < 3; a++) {
                    const int e = a * kRows + tid;
                    v[a] = (kAlpha * L.x[e] + (1.0 - kAlpha) * L.z1[e]) + L.u1[e];
                }
                Set::project(L.set, s, eps, v, zp);
                for (int a = 0; a < 3; a++) {
                    const int e = a * kRows + tid;
                    const double z = zp[a];
                    L.z1[e] = z;
                    L.u1[e] = v[a] - z;
                    const double df = fabs(L.x[e] - z);
                    rp = (df > rp || df != df) ? df : rp;
                    nax = fmax(nax, fabs(L.x[e]));
                    nz = fmax(nz, fabs(z));
                }
            }
        }
        if (use_v || use_a) {
            for (int e = tid; e < 3 * kRows; e += kThreads) {
                const int s = (e % kRows) / kSlot, l = e % kSlot;
                if (s >= m) continue;
                const int n = L.n[s];
                if (use_v && l < n) {
                    const double d = L.x[e + 1] - L.x[e];
                    const double v = (kAlpha * d + (1.0 - kAlpha) * L.zv[e]) + L.uv[e];
                    const double z = fmin(fmax(v, -L.bv[s]), L.bv[s]);
                    L.zv[e] = z;
                    L.uv[e] = v - z;
                    const double df = fabs(d - z);
                    rp = (df > rp || df != df) ? df : rp;
                    nax = fmax(nax, fabs(d));
                    nz = fmax(nz, fabs(z));
                }
                if (use_a && l < n - 1) {
                    const double d = (L.x[e + 2] - 2.0 * L.x[e + 1]) + L.x[e];
                    const double v = (kAlpha * d + (1.0 - kAlpha) * L.za[e]) + L.ua[e];
                    const double z = fmin(fmax(v, -L.ba[s]), L.ba[s]);
                    L.za[e] = z;
                    L.ua[e] = v - z;
                    const double df = fabs(d - z);
                    rp = (df > rp || df != df) ? df : rp;
                    nax = fmax(nax, fabs(d));
                    nz = fmax(nz, fabs(z));
                }
            }
        }
        __syncthreads();
        if (!check) continue;

        double rd = 0.0, nq = 0.0, ny = 0.0;
        for (int e = tid; e < 3 * kRows; e += kThreads) {
            const int s = (e % kRows) / kSlot, l = e % kSlot;
            if (s >= m || l > L.n[s]) continue;
            const int o = e - l, n = L.n[s];
            rd = fmax(rd, fabs(at_gather(L.z1 + o, L.zv + o, L.za + o, l, n, use_v, use_a) - L.t[e]));
            if (adaptive) {
                double acc = 0.0;
                for (int c = 0; c <= n; c++) acc += L.Qm[s * kTri + (l >= c ? tri(l, c) : tri(c, l))] * L.x[o + c];
                nq = fmax(nq, fabs(acc));
                ny = fmax(ny, fabs(at_gather(L.u1 + o, L.uv + o, L.ua + o, l, n, use_v, use_a)));
            }
        }
        const double rp_nan = block_max(L, rp != rp ? 1.0 : 0.0);
        r_prim = block_max(L, rp);
        if (rp_nan > 0.0) r_prim = nan;
        r_dual = rho * block_max(L, rd);
        if (r_prim <= eps && r_dual <= eps) {
            done = true;
        } else if (adaptive && it < prm.max_iter) {
            nax = block_max(L, nax); nz = block_max(L, nz); nq = block_max(L, nq); ny = rho * block_max(L, ny);
            const double num = r_prim / fmax(fmax(nax, nz), 1e-300), den = r_dual / fmax(fmax(nq, ny), 1e-300);
            double next = kRhoMax;
            if (den > 0.0) {
                const double ratio = sqrt(num / den);
                next = isfinite(ratio) ? fmin(fmax(rho * ratio, kRhoMin), kRhoMax) : (ratio != ratio ? rho : kRhoMax);
            }
            if (next > rho * kRhoStep || next * kRhoStep < rho) {
                const double f = rho / next;
                for (int e = tid; e < 3 * kRows; e += kThreads) { L.u1[e] *= f; L.uv[e] *= f; L.ua[e] *= f; }
                rho = next;
                __syncthreads();
                factor(L, m, rho, use_v, use_a);
            }
        }
    }

    // ---- the final pass on x itself
    double cost = 0.0, slack = INFINITY, vmax = 0.0, amax = 0.0;
    for (int e = tid; e < 3 * kRows; e += kThreads) {
        const int s = (e % kRows) / kSlot, l = e % kSlot;
        if (s >= m || l > L.n[s]) continue;
        const int o = e - l, n = L.n[s];
        double acc = 0.0;
        for (int c = 0; c <= n; c++) acc += L.Qm[s * kTri + (l >= c ? tri(l, c) : tri(c, l))] * L.x[o + c];
        cost += L.x[e] * acc;
        if (l < n) vmax = fmax(vmax, fabs(L.x[e + 1] - L.x[e]) * L.fv[s]);
        if (l < n - 1) amax = fmax(amax, fabs((L.x[e + 2] - 2.0 * L.x[e + 1]) + L.x[e]) * L.fa[s]);
    }
    if (tid < kRows) {
        const int s = tid / kSlot, l = tid % kSlot;
        if (s < m && l <= L.n[s]) {
            const double p[3] = {L.x[tid], L.x[kRows + tid], L.x[2 * kRows + tid]};
            slack = Set::slack(L.set, s, p);
        }
    }
    cost = 0.5 * block_sum(L, cost) / scale;
    const double slack_nan = block_max(L, slack != slack ? 1.0 : 0.0);
    slack = -block_max(L, -slack);
    if (slack_nan > 0.0) slack = nan;
    vmax = block_max(L, vmax);
    amax = block_max(L, amax);
    double dur = 0.0;
    for (int s = 0; s < m; s++) dur += L.T[s];

    for (int e = tid; e < m * (int)row_stride; e += kThreads) {
        const int s = e / (int)row_stride, j = e % (int)row_stride, cnt = L.n[s] + 1;
        polycoef[(s0 + s) * row_stride + j] = j < 3 * cnt ? L.x[(j / cnt) * kRows + s * kSlot + j % cnt] / L.T[s] : 0.0;
    }
    if (tid == 0) {
        pct_trajgen_result r;
        r.status = (r_prim <= eps && r_dual <= eps && slack >= 0.0) ? PCT_GEN_OK : PCT_GEN_NOT_CONVERGED;
        r.iterations = it;
        r.cost = cost; r.duration = dur; r.r_prim = r_prim; r.r_dual = r_dual; r.sphere_slack = slack; r.max_vel_ctrl = vmax; r.max_acc_ctrl = amax;
        res[b] = r;
    }
}

__global__ __launch_bounds__(kThreads) void trajgen_kernel(pct_trajgen_batch in, pct_trajgen_params prm, double *__restrict__ polycoef,
                                                           int64_t row_stride, pct_trajgen_result *__restrict__ res)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    generate<BallSet>(*reinterpret_cast<GenLds *>(smem), in, prm, polycoef, row_stride, res);
}

}  // namespace pct_trajgen
