// bezier_batch.hpp -- the sampled Bezier check for B candidate trajectories at once (pct_bezier_check_batch*, contract in
// include/pct_engine.h, paragraph "Batched Bezier check"; included by engine.hip behind kernels.hpp).
//
// The passes, all on one stream and without a host decision between them:
//   bb_count_kernel     one lane per trajectory runs the reference's nested sample loops (bezier_enumerate of bernstein.hpp; its adds
//                       are a dependent chain by definition, so the parallelism is across trajectories) and writes nsamples_b and
//                       m_b = min(nsamples_b, cap, 4096)
//   scan_tile_sums_kernel (scan.hpp)   m_b -> offsets, in place, B + 1 entries
//   bb_fill_kernel      the same lanes replay the loops and store (segment, t) of every evaluated sample at its slot
//   bb_eval_kernel      one thread per slot: getPosFromBezier (bezier_point of bernstein.hpp)
//   inflate_dev         (engine.hip) the sphere inflation of every slot, on whatever index the cloud has
//   bb_verdict_kernel   a wave per trajectory folds its row: first radius < 0, and the smallest radius with its lowest sample
//   bb_export_kernel    device form only: the rows from the cloud's workspaces into the caller's lists
// The device form sizes the per-slot launches from list_cap and every kernel guards on the device-side total offsets[B]; a slot
// behind the total is given the cloud's row 0 as its position -- a query that coincides with a point ends in the first cell
// it looks at -- and nothing of it leaves the workspaces.  No LDS beyond the scan's and the wave folds' few words.
#pragma once
#include "../../include/pct_engine.h"
#include "bernstein.hpp"
#include "scan.hpp"

namespace pct {

constexpr long long kBbLoopBound = 1ll << 20;   // samples a trajectory may enumerate on the device (pct_engine.h: "2^20")

// the batch as the kernels read it: device pointers of pct_bezier_batch
struct BbDesc {
    const double *coef;
    long long row_stride;
    const double *seg_time;
    const int32_t *orders;
    const int32_t *seg_offsets;
    const double *t_start;       // may be null: 0.0
    long long B;
    double stop_time, dt;
    long long cap;               // already clipped to kBezierCapMax (engine.hip)
};

// lane b < B: verdict[b].nsamples (-1: an unsound range, or more than kBbLoopBound + one per segment samples) and offsets[b] = m_b;
// lane B: offsets[B] = 0, so that the scan of B + 1 entries leaves the total there
__global__ __launch_bounds__(256) void bb_count_kernel(BbDesc D, pct_traj_verdict *__restrict__ verdict, long long *__restrict__ offsets)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > D.B) return;
    if (b == D.B) { offsets[b] = 0; return; }
    int s0, s1;
    long long n = -1;
    if (bezier_range_sound(D.seg_offsets, D.orders, D.row_stride, D.B, b, s0, s1))
        n = bezier_enumerate<false>(D.seg_time, s0, s1, D.t_start ? D.t_start[b] : 0.0, D.stop_time, D.dt, 0, kBbLoopBound + (s1 - s0),
                                    [](long long, double, int) {});
    verdict[b].nsamples = n;
    offsets[b] = n < 0 ? 0 : (n < D.cap ? n : D.cap);
}

// lane b: (segment, t) of its m_b evaluated samples at slots offsets[b] ..; nothing when the total exceeds list_cap
__global__ __launch_bounds__(256) void bb_fill_kernel(BbDesc D, const long long *__restrict__ offsets, long long list_cap,
                                                      uint32_t *__restrict__ slot_seg, double *__restrict__ slot_t)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.B || offsets[D.B] > list_cap) return;
    const long long o = offsets[b], m = offsets[b + 1] - o;
    if (m <= 0) return;
    const int s0 = D.seg_offsets[b], s1 = D.seg_offsets[b + 1];      // m > 0: bb_count_kernel found the range sound
    bezier_enumerate<true>(D.seg_time, s0, s1, D.t_start ? D.t_start[b] : 0.0, D.stop_time, D.dt, m, kBbLoopBound + (s1 - s0),
                           [&](long long k, double t, int seg) { slot_seg[o + k] = (uint32_t)seg; slot_t[o + k] = t; });
}

// one thread per slot < nslots (the host form: the total; the device form: list_cap).  A slot below the total: getPosFromBezier
// (bezier_point).  Any other slot: the cloud's row 0 (pad != null), whose search ends where it starts.
__global__ __launch_bounds__(128) void bb_eval_kernel(BbDesc D, const long long *__restrict__ offsets, long long list_cap, long long nslots,
                                                      const uint32_t *__restrict__ slot_seg, const double *__restrict__ slot_t,
                                                      const float *__restrict__ pad_x, const float *__restrict__ pad_y,
                                                      const float *__restrict__ pad_z, double *__restrict__ pos)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const long long total = offsets[D.B];
    if (total > list_cap || s >= total) {
        pos[3 * s] = pad_x ? (double)pad_x[0] : 0.0;
        pos[3 * s + 1] = pad_y ? (double)pad_y[0] : 0.0;
        pos[3 * s + 2] = pad_z ? (double)pad_z[0] : 0.0;
        return;
    }
    const int seg = (int)slot_seg[s];
    const double T = D.seg_time[seg];
    bezier_point(D.coef + (size_t)seg * D.row_stride, D.orders[seg], T, slot_t[s] / T, pos + 3 * s);
}

// A wave per trajectory (4 in a block).  Lane l reads the samples l, l + 64, .. of its row in ascending order, so `<` keeps the lowest
// index of a tie inside a lane; across lanes the fold compares (radius, index).  Not evaluated (the total exceeds list_cap):
// -2, -2, NaN.  nsamples is bb_count_kernel's.
__global__ __launch_bounds__(256) void bb_verdict_kernel(long long B, const long long *__restrict__ offsets, long long list_cap,
                                                         const double *__restrict__ radius, pct_traj_verdict *__restrict__ verdict)
{
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    if (offsets[B] > list_cap) {
        if (lane == 0) { verdict[b].first_hit = -2; verdict[b].min_sample = -2; verdict[b].min_radius = __builtin_nan(""); }
        return;
    }
    const long long o = offsets[b], m = offsets[b + 1] - o;
    long long hit = 0x7FFFFFFFFFFFFFFFll, mi = 0x7FFFFFFFFFFFFFFFll;
    double mr = __builtin_huge_val();
    for (long long k = lane; k < m; k += 64) {
        const double r = radius[o + k];
        if (r < 0.0 && k < hit) hit = k;
        if (r < mr || mi == 0x7FFFFFFFFFFFFFFFll) { mr = r; mi = k; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long oh = __shfl_xor(hit, off, 64), oi = __shfl_xor(mi, off, 64);
        const double orr = __shfl_xor(mr, off, 64);
        if (oh < hit) hit = oh;
        if (oi != 0x7FFFFFFFFFFFFFFFll && (mi == 0x7FFFFFFFFFFFFFFFll || orr < mr || (orr == mr && oi < mi))) { mr = orr; mi = oi; }
    }
    if (lane == 0) {
        verdict[b].first_hit = hit == 0x7FFFFFFFFFFFFFFFll ? -1 : hit;
        verdict[b].min_sample = mi == 0x7FFFFFFFFFFFFFFFll ? -1 : mi;
        verdict[b].min_radius = mi == 0x7FFFFFFFFFFFFFFFll ? __builtin_huge_val() : mr;
    }
}

// device form: the slots below the total from the cloud's workspaces into the caller's lists (a null list is not wanted); nothing when
// the total exceeds list_cap, and nothing behind the total ever
__global__ __launch_bounds__(256) void bb_export_kernel(long long B, const long long *__restrict__ offsets, long long list_cap,
                                                        const double *__restrict__ w_pos, const double *__restrict__ w_radius,
                                                        const double *__restrict__ w_d2, const uint32_t *__restrict__ w_idx,
                                                        double *__restrict__ pos, double *__restrict__ radius, double *__restrict__ d2,
                                                        uint32_t *__restrict__ idx)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = offsets[B];
    if (total > list_cap || s >= total) return;
    if (pos) { pos[3 * s] = w_pos[3 * s]; pos[3 * s + 1] = w_pos[3 * s + 1]; pos[3 * s + 2] = w_pos[3 * s + 2]; }
    if (radius) radius[s] = w_radius[s];
    if (d2) d2[s] = w_d2[s];
    if (idx) idx[s] = w_idx[s];
}

}  // namespace pct
