// ring_depth.hpp -- depth images as an input of the ROLLING obstacle map (pct_cloud_ring_carve_depth, pct_cloud_append_depth,
// pct_depth_classify): the projection of include/pct_engine.h, paragraph "Depth images", stated once for the device.
//
//   depth_project        a cloud row (fp32) -> is it in the image, its pixel, its z-depth and its offset from the camera
//   depth_seen_through   the carve's and the classifier's predicate: in the image, a finite pixel, strictly nearer than it - margin
//   depth_unproject      a pixel of a z-depth image -> the fp32 point it shows
// Everything is fp64 from float-widened operands, one rounding per operation, no contraction, in the order the header writes the
// expressions; tests/helpers/depth_model.py restates them in numpy and the GPU tests hold the two equal bit for bit.
//
// Kernels: the carve is ring_remove_kernel (ring_remove.hpp) with DepthSeenThrough for a predicate -- one pass over the
// slots below the window's size, 12 B per slot and one gather from an image that stays in L2 (1.2 MB at 640 x 480), the counts
// and the host word of every other removal.  depth_valid_kernel / depth_unproject_kernel stand on either side of the de-dup
// filter's rank and scan kernels (ring_dedup.hpp): flags of the valid pixels, their ranks, then every valid pixel un-projected
// straight into its place of the packed frame the insert kernel reads -- no point list is ever stored uncompacted.
#pragma once
#include "../../include/pct_engine.h"
#include "ring_dedup.hpp"
#include "ring_remove.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr int kDepthMaxViews = 16;

__device__ __forceinline__ bool depth_finite(double v) { return fabs(v) < (double)INFINITY; }      // false for NaN

// d = (double)p - t; c_k = (d0*R[0][k] + d1*R[1][k]) + d2*R[2][k]; in the image iff c_z >= near_z (a NaN fails) and the rounded pixel
// (half away from zero) lies inside, compared in fp64 before any conversion to int.  One scale for both axes, as the reference.
__device__ __forceinline__ bool depth_project(const pct_depth_view &V, float px, float py, float pz, double d[3], double &cz, int &ru, int &rv)
{
    d[0] = (double)px - V.t[0]; d[1] = (double)py - V.t[1]; d[2] = (double)pz - V.t[2];
    const double cx = (d[0] * V.R[0] + d[1] * V.R[3]) + d[2] * V.R[6];
    const double cy = (d[0] * V.R[1] + d[1] * V.R[4]) + d[2] * V.R[7];
    cz = (d[0] * V.R[2] + d[1] * V.R[5]) + d[2] * V.R[8];
    if (!(cz >= V.near_z)) return false;
    const double w = (double)V.width, h = (double)V.height;
    const double scale = V.focal / cz * w;
    const double u = cx * scale + w / 2.0, v = cy * scale + h / 2.0;
    const double fu = round(u), fv = round(v);
    if (!(fu >= 0.0 && fu <= w - 1.0 && fv >= 0.0 && fv <= h - 1.0)) return false;
    ru = (int)fu; rv = (int)fv;
    return true;
}

// Seen through: in the image, the pixel finite (+inf = nothing rendered, NaN and -inf likewise: they prove nothing), and with
// w = val - margin: c_z < w (metric Z) or w > 0 && |d|^2 < w*w (metric RANGE: no square root).  Strict: a point at val - margin stays.
__device__ __forceinline__ bool depth_seen_through(const pct_depth_view &V, const float *__restrict__ image, double margin, float px, float py, float pz)
{
    double d[3], cz;
    int ru, rv;
    if (!depth_project(V, px, py, pz, d, cz, ru, rv)) return false;
    const double val = (double)image[(size_t)rv * (size_t)V.width + (size_t)ru];
    if (!depth_finite(val)) return false;
    const double w = val - margin;
    if (V.metric == PCT_DEPTH_Z) return cz < w;
    return w > 0.0 && ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < w * w;
}

// the carve's predicate of ring_remove_kernel (ring_remove.hpp): the row is seen through in this view of this image
struct DepthSeenThrough {
    pct_depth_view V;
    const float *image;
    double margin;
    __device__ __forceinline__ bool operator()(uint32_t, float px, float py, float pz) const { return depth_seen_through(V, image, margin, px, py, pz); }
};

// ---- un-projection (metric Z) ---------------------------------------------------------------------------------------------------
// valid iff dep is finite, dep >= near_z and dep <= max_depth (a NaN fails all three)
__device__ __forceinline__ bool depth_pixel_valid(const pct_depth_view &V, double dep, double max_depth)
{
    return depth_finite(dep) && dep >= V.near_z && dep <= max_depth;
}

__global__ __launch_bounds__(256) void depth_valid_kernel(pct_depth_view V, const float *__restrict__ image, uint32_t npix, double max_depth,
                                                          uint8_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npix) flags[i] = depth_pixel_valid(V, (double)image[i], max_depth) ? 1 : 0;
}

// a = ((double)x/width - 0.5)/focal, b = ((double)y - 0.5*height)/width/focal, p_k = t[k] + dep*((a*R[k][0] + b*R[k][1]) + R[k][2]),
// narrowed to fp32 (round to nearest); valid pixels land in row-major order at tile_off[tile] + rank (dd_rank_kernel / scan_tile_sums_kernel with DdPublish)
__global__ __launch_bounds__(256) void depth_unproject_kernel(pct_depth_view V, const float *__restrict__ image, uint32_t npix,
                                                              const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank,
                                                              const uint32_t *__restrict__ tile_off, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix || !flags[i]) return;
    const uint32_t px = i % (uint32_t)V.width, py = i / (uint32_t)V.width;
    const double dep = (double)image[i];
    const double w = (double)V.width, h = (double)V.height;
    const double a = ((double)px / w - 0.5) / V.focal;
    const double b = ((double)py - 0.5 * h) / w / V.focal;
    float *o = out + 3 * (size_t)(tile_off[i / kDdTile] + rank[i]);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (float)(V.t[k] + dep * ((a * V.R[3 * k] + b * V.R[3 * k + 1]) + V.R[3 * k + 2]));
}

// ---- classification of planner points against a buffer of images (safety_controller::check_image_for_point for a batch) ----------
struct DepthViews {
    pct_depth_view v[kDepthMaxViews];
    const float *image[kDepthMaxViews];
    int n;
};

// One thread per planner point, narrowed to fp32 first (|p| > FLT_MAX becomes infinite and is in no image).  seen_by = the lowest
// view that sees the point through, or -1; pixel = (ru, rv) in the LAST view, or (-1, -1) when the point is not in that image.
__global__ __launch_bounds__(256) void depth_classify_kernel(DepthViews S, const double *__restrict__ pts, uint32_t n, double margin,
                                                             int32_t *__restrict__ seen_by, int32_t *__restrict__ pixel)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float px = (float)pts[3 * (size_t)i], py = (float)pts[3 * (size_t)i + 1], pz = (float)pts[3 * (size_t)i + 2];
    int32_t first = -1;
    for (int k = 0; k < S.n; k++)
        if (depth_seen_through(S.v[k], S.image[k], margin, px, py, pz)) { first = k; break; }
    seen_by[i] = first;
    if (pixel) {
        double d[3], cz;
        int ru = -1, rv = -1;
        if (!depth_project(S.v[S.n - 1], px, py, pz, d, cz, ru, rv)) ru = rv = -1;
        pixel[2 * (size_t)i] = ru; pixel[2 * (size_t)i + 1] = rv;
    }
}

}  // namespace pct
