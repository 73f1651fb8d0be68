// trajgen.hip -- the trajectory generator (include/pct_trajgen.h), part of libpct_engine.so: minimum-jerk piecewise Bezier curves
// inside a chain of spheres or of polytopes, B candidates per launch, solved by ADMM.
//
// The kernel is trajgen.hpp, the polytopes' part of it trajgen_poly.hpp; here are the launches, the host form (staging copies, the device form, one wait) and the reference's
// time allocation restated on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/pct_trajgen.h"
#include "engine_internal.hpp"
#include "trajgen.hpp"
#include "trajgen_poly.hpp"

using pct_internal::fail;
using namespace pct_trajgen;

namespace {

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(PCT_ERR_HIP, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define PCTCHK(call)                    \
    do {                                \
        int s_ = (call);                \
        if (s_ != PCT_OK) return s_;    \
    } while (0)

int check_params(const pct_trajgen_params *p)
{
    if (!p) return fail(PCT_ERR_INVALID, "null params");
    if (p->minimize_order < 1 || p->minimize_order > 4) return fail(PCT_ERR_INVALID, "minimize_order %d (supported: 1..4)", p->minimize_order);
    if (p->max_iter <= 0 || p->check_every <= 0) return fail(PCT_ERR_INVALID, "max_iter and check_every must be positive");
    if (!(p->eps > 0.0) || !std::isfinite(p->eps)) return fail(PCT_ERR_INVALID, "eps must be positive");
    if (std::isnan(p->max_vel) || std::isnan(p->max_acc) || !std::isfinite(p->margin) || !std::isfinite(p->rho) || p->rho < 0.0)
        return fail(PCT_ERR_INVALID, "a limit, margin or rho is not a number, or rho < 0");
    return PCT_OK;
}

}  // namespace

extern "C" {

int pct_bezier_generate_batch_dev(const pct_trajgen_batch *d, const pct_trajgen_params *params, double *d_polycoef, int64_t row_stride,
                                  pct_trajgen_result *d_res, void *stream)
{
    PCTCHK(check_params(params));
    if (!d || d->B < 0) return fail(PCT_ERR_INVALID, "bad batch");
    if (d->B == 0) return PCT_OK;
    if (!d->centres || !d->radius || !d->seg_time || !d->orders || !d->seg_offsets || !d->start_state || !d->end_state || !d_polycoef || !d_res)
        return fail(PCT_ERR_INVALID, "null array");
    if (row_stride < 3 * (kMinOrder + 1) || row_stride > (1 << 20)) return fail(PCT_ERR_INVALID, "row_stride %lld", (long long)row_stride);
    if (d->B > 0x7fffffff) return fail(PCT_ERR_INVALID, "too many candidates");
    PCTCHK(pct_internal::require_init());
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(trajgen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GenLds)));
        attr_set = true;
    }
    trajgen_kernel<<<(unsigned)d->B, kThreads, sizeof(GenLds), (hipStream_t)stream>>>(*d, *params, d_polycoef, row_stride, d_res);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_bezier_generate_batch(const pct_trajgen_batch *h, const pct_trajgen_params *params, double *polycoef, int64_t row_stride,
                              pct_trajgen_result *result)
{
    PCTCHK(check_params(params));
    if (!h || h->B < 0) return fail(PCT_ERR_INVALID, "bad batch");
    if (h->B == 0) return PCT_OK;
    if (!h->centres || !h->radius || !h->seg_time || !h->orders || !h->seg_offsets || !h->start_state || !h->end_state || !polycoef || !result)
        return fail(PCT_ERR_INVALID, "null array");
    const int64_t B = h->B;
    if (h->seg_offsets[0] != 0) return fail(PCT_ERR_INVALID, "seg_offsets[0] must be 0");
    for (int64_t b = 0; b < B; b++)
        if (h->seg_offsets[b + 1] < h->seg_offsets[b]) return fail(PCT_ERR_INVALID, "seg_offsets must not descend");
    const int64_t total = h->seg_offsets[B];
    for (int64_t s = 0; s < total; s++)
        if (h->orders[s] >= kMinOrder && h->orders[s] <= kMaxOrder && 3 * (int64_t)(h->orders[s] + 1) > row_stride)
            return fail(PCT_ERR_INVALID, "row_stride %lld too small for order %d", (long long)row_stride, h->orders[s]);
    if (row_stride < 3 * (kMinOrder + 1)) return fail(PCT_ERR_INVALID, "row_stride %lld", (long long)row_stride);
    PCTCHK(pct_internal::require_init());
    hipStream_t s = pct_internal::stream();
    const size_t nt = (size_t)total, nb = (size_t)B;
    pct_internal::DevBuf<double> d_in, d_out;
    pct_internal::DevBuf<int32_t> d_int;
    pct_internal::DevBuf<pct_trajgen_result> d_res;
    PCTCHK(d_in.reset(5 * nt + 18 * nb));      // centres | radius | seg_time | start | end
    PCTCHK(d_out.reset(nt * (size_t)row_stride));
    PCTCHK(d_int.reset(nt + nb + 1));           // orders | seg_offsets
    PCTCHK(d_res.reset(nb));
    double *dc = d_in, *dr = dc + 3 * nt, *dT = dr + nt, *ds = dT + nt, *de = ds + 9 * nb;
    int32_t *dorders = d_int, *doffs = dorders + nt;
    if (nt) {
        HIPCHK(hipMemcpyAsync(dc, h->centres, sizeof(double) * 3 * nt, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dr, h->radius, sizeof(double) * nt, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dT, h->seg_time, sizeof(double) * nt, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dorders, h->orders, sizeof(int32_t) * nt, hipMemcpyHostToDevice, s));
        // the caller's rows come back as they were wherever the kernel writes nothing (a candidate without segments)
        HIPCHK(hipMemcpyAsync(d_out, polycoef, sizeof(double) * nt * (size_t)row_stride, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(ds, h->start_state, sizeof(double) * 9 * nb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(de, h->end_state, sizeof(double) * 9 * nb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(doffs, h->seg_offsets, sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice, s));
    pct_trajgen_batch d = {dc, dr, dT, dorders, doffs, ds, de, B};
    PCTCHK(pct_bezier_generate_batch_dev(&d, params, d_out, row_stride, d_res, s));
    if (nt) HIPCHK(hipMemcpyAsync(polycoef, d_out, sizeof(double) * nt * (size_t)row_stride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(result, d_res, sizeof(pct_trajgen_result) * nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PCT_OK;
}

int pct_trajgen_max_planes(void) { return kMaxPlanes; }

int pct_bezier_generate_poly_batch_dev(const pct_trajgen_poly_batch *d, const pct_trajgen_params *params, double *d_polycoef, int64_t row_stride,
                                       pct_trajgen_result *d_res, void *stream)
{
    PCTCHK(check_params(params));
    if (!d || d->B < 0) return fail(PCT_ERR_INVALID, "bad batch");
    if (d->B == 0) return PCT_OK;
    if (!d->anchors || !d->planes || !d->plane_offsets || !d->seg_time || !d->orders || !d->seg_offsets || !d->start_state || !d->end_state || !d_polycoef || !d_res)
        return fail(PCT_ERR_INVALID, "null array");
    if (row_stride < 3 * (kMinOrder + 1) || row_stride > (1 << 20)) return fail(PCT_ERR_INVALID, "row_stride %lld", (long long)row_stride);
    if (d->B > 0x7fffffff) return fail(PCT_ERR_INVALID, "too many candidates");
    PCTCHK(pct_internal::require_init());
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(trajgen_poly_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PolyLds)));
        attr_set = true;
    }
    trajgen_poly_kernel<<<(unsigned)d->B, kThreads, sizeof(PolyLds), (hipStream_t)stream>>>(*d, *params, d_polycoef, row_stride, d_res);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_bezier_generate_poly_batch(const pct_trajgen_poly_batch *h, const pct_trajgen_params *params, double *polycoef, int64_t row_stride,
                                   pct_trajgen_result *result)
{
    PCTCHK(check_params(params));
    if (!h || h->B < 0) return fail(PCT_ERR_INVALID, "bad batch");
    if (h->B == 0) return PCT_OK;
    if (!h->anchors || !h->planes || !h->plane_offsets || !h->seg_time || !h->orders || !h->seg_offsets || !h->start_state || !h->end_state || !polycoef || !result)
        return fail(PCT_ERR_INVALID, "null array");
    const int64_t B = h->B;
    if (h->seg_offsets[0] != 0) return fail(PCT_ERR_INVALID, "seg_offsets[0] must be 0");
    for (int64_t b = 0; b < B; b++)
        if (h->seg_offsets[b + 1] < h->seg_offsets[b]) return fail(PCT_ERR_INVALID, "seg_offsets must not descend");
    const int64_t total = h->seg_offsets[B];
    if (h->plane_offsets[0] != 0) return fail(PCT_ERR_INVALID, "plane_offsets[0] must be 0");
    for (int64_t s = 0; s < total; s++) {
        if (h->plane_offsets[s + 1] < h->plane_offsets[s]) return fail(PCT_ERR_INVALID, "plane_offsets must not descend");
        if (h->orders[s] >= kMinOrder && h->orders[s] <= kMaxOrder && 3 * (int64_t)(h->orders[s] + 1) > row_stride)
            return fail(PCT_ERR_INVALID, "row_stride %lld too small for order %d", (long long)row_stride, h->orders[s]);
    }
    if (row_stride < 3 * (kMinOrder + 1)) return fail(PCT_ERR_INVALID, "row_stride %lld", (long long)row_stride);
    PCTCHK(pct_internal::require_init());
    hipStream_t s = pct_internal::stream();
    const size_t nt = (size_t)total, nb = (size_t)B, np = (size_t)h->plane_offsets[total];
    pct_internal::DevBuf<double> d_in, d_out;
    pct_internal::DevBuf<int32_t> d_int;
    pct_internal::DevBuf<pct_trajgen_result> d_res;
    PCTCHK(d_in.reset(4 * nt + 18 * nb + 4 * np + 4));      // anchors | seg_time | start | end | planes
    PCTCHK(d_out.reset(nt * (size_t)row_stride));
    PCTCHK(d_int.reset(2 * nt + nb + 2));                   // orders | seg_offsets | plane_offsets
    PCTCHK(d_res.reset(nb));
    double *da = d_in, *dT = da + 3 * nt, *ds = dT + nt, *de = ds + 9 * nb, *dp = de + 9 * nb;
    int32_t *dorders = d_int, *doffs = dorders + nt, *dpo = doffs + nb + 1;
    if (nt) {
        HIPCHK(hipMemcpyAsync(da, h->anchors, sizeof(double) * 3 * nt, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dT, h->seg_time, sizeof(double) * nt, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dorders, h->orders, sizeof(int32_t) * nt, hipMemcpyHostToDevice, s));
        // the caller's rows come back as they were wherever the kernel writes nothing (a candidate without segments)
        HIPCHK(hipMemcpyAsync(d_out, polycoef, sizeof(double) * nt * (size_t)row_stride, hipMemcpyHostToDevice, s));
    }
    if (np) HIPCHK(hipMemcpyAsync(dp, h->planes, sizeof(double) * 4 * np, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dpo, h->plane_offsets, sizeof(int32_t) * (nt + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ds, h->start_state, sizeof(double) * 9 * nb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(de, h->end_state, sizeof(double) * 9 * nb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(doffs, h->seg_offsets, sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice, s));
    pct_trajgen_poly_batch d = {da, dp, dpo, dT, dorders, doffs, ds, de, B};
    PCTCHK(pct_bezier_generate_poly_batch_dev(&d, params, d_out, row_stride, d_res, s));
    if (nt) HIPCHK(hipMemcpyAsync(polycoef, d_out, sizeof(double) * nt * (size_t)row_stride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(result, d_res, sizeof(pct_trajgen_result) * nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PCT_OK;
}

int pct_time_allocation(const double *centres, const double *radius, int64_t n, const double start[3], const double end[3],
                        const double init_vel[3], double vel_mean, double acc_mean, double *seg_time)
{
    if (!centres || !radius || !start || !end || !init_vel || !seg_time || n < 1) return fail(PCT_ERR_INVALID, "bad arguments");
    if (!(vel_mean > 0.0) || !(acc_mean > 0.0)) return fail(PCT_ERR_INVALID, "vel_mean and acc_mean must be positive");
    std::vector<double> pts(3 * (size_t)(n + 1));
    for (int d = 0; d < 3; d++) { pts[(size_t)d] = start[d]; pts[3 * (size_t)n + d] = end[d]; }
    for (int64_t i = 1; i < n; i++) {                       // :623-637, the joint between spheres i - 1 and i
        const double *lc = centres + 3 * (i - 1), *c = centres + 3 * i;
        const double dx = c[0] - lc[0], dy = c[1] - lc[1], dz = c[2] - lc[2];
        const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
        const double w = dist + radius[i - 1] - radius[i];
        pts[3 * (size_t)i] = dx * w / (2.0 * dist) + lc[0];
        pts[3 * (size_t)i + 1] = dy * w / (2.0 * dist) + lc[1];
        pts[3 * (size_t)i + 2] = dz * w / (2.0 * dist) + lc[2];
    }
    for (int64_t k = 0; k < n; k++) {                       // :647-683
        const double *p0 = &pts[3 * (size_t)k], *p1 = p0 + 3;
        const double d[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double v0[3] = {k == 0 ? init_vel[0] : 0.0, k == 0 ? init_vel[1] : 0.0, k == 0 ? init_vel[2] : 0.0};
        const double D = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double V0 = v0[0] * (d[0] / D) + v0[1] * (d[1] / D) + v0[2] * (d[2] / D);
        const double aV0 = std::fabs(V0);
        const double sgn = vel_mean > V0 ? 1.0 : -1.0;
        const double acct = (vel_mean - V0) / acc_mean * sgn;
        const double accd = V0 * acct + (acc_mean * acct * acct / 2) * sgn;
        const double dcct = vel_mean / acc_mean;
        const double dccd = acc_mean * dcct * dcct / 2;
        double dt;
        if (D < aV0 * aV0 / (2 * acc_mean)) {
            const double t1 = V0 < 0 ? 2.0 * aV0 / acc_mean : 0.0, t2 = aV0 / acc_mean;
            dt = t1 + t2;
        } else if (D < accd + dccd) {
            const double t1 = V0 < 0 ? 2.0 * aV0 / acc_mean : 0.0;
            const double t2 = (-aV0 + std::sqrt(aV0 * aV0 + acc_mean * D - aV0 * aV0 / 2)) / acc_mean;
            const double t3 = (aV0 + acc_mean * t2) / acc_mean;
            dt = t1 + t2 + t3;
        } else {
            dt = acct + (D - accd - dccd) / vel_mean + dcct;
        }
        seg_time[k] = dt;
    }
    return PCT_OK;
}

}  // extern "C"
