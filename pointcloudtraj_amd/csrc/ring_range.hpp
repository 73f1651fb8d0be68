// ring_range.hpp -- lidar range images as an input of the ROLLING obstacle map (pct_cloud_ring_carve_range, pct_cloud_append_range,
// pct_range_classify): the projection of include/pct_engine.h, paragraph "Range images", stated once for the device and the host.
//
//   range_pseudo_angle   a monotone stand-in for atan2 on [0, 4): one division, no transcendental function (host and device)
//   range_project        a cloud row (fp32) -> is it in the image, its pixel (two binary searches in the edge tables), its squared range
//   range_seen_through   the carve's and the classifier's predicate: in the image, a finite pixel, strictly nearer than it - margin
//   range_unproject      a pixel of a range image -> the fp32 point it shows, from the caller's direction tables
// Everything is fp64 from float-widened operands, one rounding per operation, no contraction, in the order the header writes the
// expressions; tests/helpers/range_model.py restates them in numpy and the GPU tests hold the two equal bit for bit.
//
// Kernels: the carve is ring_remove_kernel (ring_remove.hpp) with RangeSeenThrough for a predicate.  The edge tables (at most
// 4097 + 1025 doubles) are read with plain loads: the two searches of a point touch <= 13 + <= 11 entries, the first steps of every
// search are the same few lines for every wave, and the tables stay in L2 beside the image.  range_valid_kernel /
// range_unproject_kernel stand on either side of the de-dup filter's rank and scan kernels (ring_dedup.hpp), as their depth twins do.
#pragma once
#include "../../include/pct_engine.h"
#include "ring_dedup.hpp"
#include "ring_remove.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace pct {

constexpr int kRangeMaxViews = 16;
constexpr int kRangeMaxWidth = 4096, kRangeMaxHeight = 1024;

// den = |x| + |y|; NaN when den is 0 or not finite; p = y / den; x < 0: 2 - p; else y < 0: 4 + p; else p.  0 = +x, 1 = +y, 2 = -x, 3 = -y
__host__ __device__ inline double range_pseudo_angle(double x, double y)
{
    const double den = fabs(x) + fabs(y);
    if (den == 0.0 || !(den < (double)INFINITY)) return (double)NAN;
    const double p = y / den;
    if (x < 0.0) return 2.0 - p;
    if (y < 0.0) return 4.0 + p;
    return p;
}

__host__ __device__ inline bool range_finite(double v) { return fabs(v) < (double)INFINITY; }      // false for NaN

// pct_range_view as the kernels take it: the pose, the sizes and DEVICE pointers to the two edge tables
struct RangeViewDev {
    double t[3], R[9], near_range;
    int32_t width, height;
    const double *col_edge, *row_edge;
};

// (number of entries of e[0..n] that are <= a) - 1, for e[0] <= a < e[n]: a plain binary search over a strictly ascending table
__device__ __forceinline__ int range_cell(const double *__restrict__ e, int n, double a)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= a) lo = mid; else hi = mid;
    }
    return lo;
}

// d = (double)p - t; r2 = (d0*d0 + d1*d1) + d2*d2; s_k = (d0*R[0][k] + d1*R[1][k]) + d2*R[2][k]; h = sqrt(s0*s0 + s1*s1);
// a = pa(s0, s1); q = s2 / h.  In the image iff near_range^2 <= r2 < +inf, h > 0 and both a and q lie inside their tables (a NaN
// fails every test); a value equal to an edge belongs to the cell above it.
__device__ __forceinline__ bool range_project(const RangeViewDev &V, float px, float py, float pz, double &r2, int &row, int &col)
{
    const double d0 = (double)px - V.t[0], d1 = (double)py - V.t[1], d2 = (double)pz - V.t[2];
    r2 = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!(r2 >= V.near_range * V.near_range && r2 < (double)INFINITY)) return false;
    const double s0 = (d0 * V.R[0] + d1 * V.R[3]) + d2 * V.R[6];
    const double s1 = (d0 * V.R[1] + d1 * V.R[4]) + d2 * V.R[7];
    const double s2 = (d0 * V.R[2] + d1 * V.R[5]) + d2 * V.R[8];
    const double h = sqrt(s0 * s0 + s1 * s1);
    if (!(h > 0.0)) return false;
    const double a = range_pseudo_angle(s0, s1);
    if (!(a >= V.col_edge[0] && a < V.col_edge[V.width])) return false;
    const double q = s2 / h;
    if (!(q >= V.row_edge[0] && q < V.row_edge[V.height])) return false;
    col = range_cell(V.col_edge, V.width, a);
    row = range_cell(V.row_edge, V.height, q);
    return true;
}

// Seen through: in the image, the pixel finite (+inf = no return, NaN and -inf likewise: they prove nothing), and with
// w = val - margin: w > 0 && r2 < w*w.  No square root; strict: a point at exactly val - margin stays.
__device__ __forceinline__ bool range_seen_through(const RangeViewDev &V, const float *__restrict__ image, double margin, float px, float py, float pz)
{
    double r2;
    int row, col;
    if (!range_project(V, px, py, pz, r2, row, col)) return false;
    const double val = (double)image[(size_t)row * (size_t)V.width + (size_t)col];
    if (!range_finite(val)) return false;
    const double w = val - margin;
    return w > 0.0 && r2 < w * w;
}

// the carve's predicate of ring_remove_kernel (ring_remove.hpp): the row is seen through in this view of this image
struct RangeSeenThrough {
    RangeViewDev V;
    const float *image;
    double margin;
    __device__ __forceinline__ bool operator()(uint32_t, float px, float py, float pz) const { return range_seen_through(V, image, margin, px, py, pz); }
};

// ---- un-projection ----------------------------------------------------------------------------------------------------------------
// valid iff rho is finite, rho >= near_range and rho <= max_range (a NaN fails all three)
__global__ __launch_bounds__(256) void range_valid_kernel(double near_range, const float *__restrict__ image, uint32_t npix, double max_range,
                                                          uint8_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double rho = (double)image[i];
    flags[i] = (range_finite(rho) && rho >= near_range && rho <= max_range) ? 1 : 0;
}

// e0 = row_dir[r][0]*col_dir[c][0], e1 = row_dir[r][0]*col_dir[c][1], e2 = row_dir[r][1];
// p_k = t[k] + rho*((e0*R[k][0] + e1*R[k][1]) + e2*R[k][2]), narrowed to fp32 (round to nearest); valid pixels land in row-major order
// at tile_off[tile] + rank (dd_rank_kernel / scan_tile_sums_kernel with DdPublish)
__global__ __launch_bounds__(256) void range_unproject_kernel(RangeViewDev V, const double *__restrict__ col_dir, const double *__restrict__ row_dir,
                                                              const float *__restrict__ image, uint32_t npix, const uint8_t *__restrict__ flags,
                                                              const uint32_t *__restrict__ rank, const uint32_t *__restrict__ tile_off,
                                                              float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix || !flags[i]) return;
    const uint32_t c = i % (uint32_t)V.width, r = i / (uint32_t)V.width;
    const double rho = (double)image[i];
    const double e0 = row_dir[2 * r] * col_dir[2 * c], e1 = row_dir[2 * r] * col_dir[2 * c + 1], e2 = row_dir[2 * r + 1];
    float *o = out + 3 * (size_t)(tile_off[i / kDdTile] + rank[i]);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (float)(V.t[k] + rho * ((e0 * V.R[3 * k] + e1 * V.R[3 * k + 1]) + e2 * V.R[3 * k + 2]));
}

// ---- classification of planner points against a buffer of scans -------------------------------------------------------------------
struct RangeViews {
    RangeViewDev v[kRangeMaxViews];
    const float *image[kRangeMaxViews];
    int n;
};

// One thread per planner point, narrowed to fp32 first (|p| > FLT_MAX becomes infinite and is in no image).  seen_by = the lowest
// view that sees the point through, or -1; pixel = (c, r) in the LAST view, or (-1, -1) when the point is not in that image.
__global__ __launch_bounds__(256) void range_classify_kernel(RangeViews S, const double *__restrict__ pts, uint32_t n, double margin,
                                                             int32_t *__restrict__ seen_by, int32_t *__restrict__ pixel)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float px = (float)pts[3 * (size_t)i], py = (float)pts[3 * (size_t)i + 1], pz = (float)pts[3 * (size_t)i + 2];
    int32_t first = -1;
    for (int k = 0; k < S.n; k++)
        if (range_seen_through(S.v[k], S.image[k], margin, px, py, pz)) { first = k; break; }
    seen_by[i] = first;
    if (pixel) {
        double r2;
        int row = -1, col = -1;
        if (!range_project(S.v[S.n - 1], px, py, pz, r2, row, col)) row = col = -1;
        pixel[2 * (size_t)i] = col; pixel[2 * (size_t)i + 1] = row;
    }
}

}  // namespace pct
