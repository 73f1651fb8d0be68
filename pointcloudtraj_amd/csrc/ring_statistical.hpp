// ring_statistical.hpp -- statistical outlier removal on the ROLLING obstacle map (pct_cloud_ring_remove_statistical, _remove_isolated,
// _knn_mean_distances, _knn_distance_stats): every judged row's mean distance to its k nearest OTHER rows of the window, the mean and
// deviation of those means in a pinned summation order, and the removal of the rows above a threshold, in place, for gfx950.  The rule
// is the paragraph "Statistical outliers" of include/pct_engine.h.
//
// Three kinds of launch, so that the judgement cannot see the removal and the threshold never leaves the device:
//   1. ring_knn_mean_kernel   read-only over the bucket table.  ONE WAVE PER JUDGED ROW, four rows per 256-thread block (a block per
//                             row with two block barriers per shell, as ring_knn_kernel spends, is right for a tick's few hundred
//                             queries and wrong for the 50 000 rows of a frame or the 5 M of a window).  The four waves walk different
//                             rows with different trip counts, so nothing in the walk is block-wide: each wave owns one sorted list in
//                             LDS (lane e owns entry e, knn_wave_insert) and tau = entry k - 1 stays in registers.  The walk is
//                             ring_knn_walk (ring_search.hpp), the one ring_knn_kernel calls, here with a group of 64, the judged
//                             slot as `self`, ks_lanes_per_bucket and an empty step.  Epilogue: lane 0 sums the k entries
//                             in list order (nearest first) with the sqrt and writes mean[slot]; a row with fewer than k candidates
//                             gets +inf.  The host has filled the buffer with NaN beforehand (rows out of scope, rows with a NaN).
//   2. ks_reduce_kernel       the sums in the contract's tree order: a block folds 256 consecutive values by halves (h = 128 and 64
//                             through LDS, h <= 32 as a butterfly inside wave 0: lane i < h receives exactly a[i] + a[i + h]) and
//                             writes {sum, sum of squares, measured rows} of its row of 256; the kernel is launched again on the block
//                             values until one is left, and thread 0 of that last launch computes mean, deviation and threshold into
//                             the device record (and its host-mapped copy).  No atomics on floating-point data: the result is a
//                             function of the means alone.
//   3. ring_remove_kernel<KsAbove>  the one removal kernel (ring_remove.hpp) with the predicate "this slot's mean is greater than the
//                             threshold in the device record" -- the NaN of an unjudged slot compares false.  For
//                             pct_cloud_ring_remove_isolated the record is filled from the argument (ks_set_threshold_kernel) instead
//                             of from the reduction.
#pragma once
#include "ring_search.hpp"
#include "ring_remove.hpp"
#include "ring_compact.hpp"

#pragma clang fp contract(off)

namespace pct {

// pct_knn_stats, field for field (include/pct_engine.h)
struct KsRecord {
    long long measured;
    double sum, sum_sq, mean, stddev, threshold;
};

// one row of 256 of the reduction tree
struct KsPart {
    double sum, sum_sq;
    unsigned long long n;
};

constexpr uint32_t kKsRows = 4;                        // judged rows per block: one per wave

// lanes of the wave that share one bucket of a step of `total` buckets (a power of two; 64 / lanes buckets are read at a time)
__device__ __forceinline__ int ks_lanes_per_bucket(int total) { return total <= 8 ? 8 : total <= 16 ? 4 : total <= 32 ? 2 : 1; }

// Judged rows: age positions [p0, W.n) of the window (rc_slot).  1 <= k <= KCAP.  WORK (the probe's build of the kernel,
// pct_set_work_counters): points = records read, cells = buckets visited, nodes = rows walked.
template <int KCAP, bool WORK>
__global__ __launch_bounds__(256) void ring_knn_mean_kernel(RingView V, RcWindow W, uint32_t p0, const float *__restrict__ x,
                                                            const float *__restrict__ y, const float *__restrict__ z, int k,
                                                            double *__restrict__ mean, WorkCounters *__restrict__ work)
{
    __shared__ double s_d[kKsRows][KCAP];
    __shared__ uint32_t s_i[kKsRows][KCAP];
    __shared__ unsigned long long s_w[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t p = (uint64_t)p0 + (uint64_t)blockIdx.x * kKsRows + (uint64_t)wave;
    uint32_t npts = 0, nbuckets = 0, walked = 0;
    if (p < W.n) {                                                      // everything below is uniform over the wave
        const uint32_t slot = rc_slot(W, (uint32_t)p);
        const float px = x[slot], py = y[slot], pz = z[slot];
        if (px == px && py == py && pz == pz) {                         // a row that holds a NaN is not judged
            double *ld = s_d[wave];
            uint32_t *li = s_i[wave];
            if (lane < k) { ld[lane] = __builtin_huge_val(); li[lane] = kNoIndex; }
            knn_lds_order();
            const float finf = __builtin_huge_valf();
            // a row with an infinite coordinate: every d2 that involves it is inf or NaN, it has no candidate
            if (fabsf(px) < finf && fabsf(py) < finf && fabsf(pz) < finf) {
                if (WORK) walked = 1;
                // the wave walks alone: tau stays in its registers, the step has nothing to do
                ring_knn_walk<64>(V, (double)px, (double)py, (double)pz, (uint32_t)lane, slot, ld, li, k, npts, nbuckets, ks_lanes_per_bucket,
                                  [](double &, uint32_t &) {});
            }
            knn_lds_order();
            if (lane == 0) {
                double m = __builtin_huge_val();                                // fewer than k candidates: not measured
                if (ld[k - 1] < __builtin_huge_val()) {
                    double s = 0.0;
                    for (int e = 0; e < k; e++) s = s + sqrt(ld[e]);
                    m = s / (double)k;
                }
                mean[slot] = m;
            }
        }
    }
    if (WORK) {
        ring_add_work(work, npts, nbuckets, s_w);
        ring_add_nodes(work, lane == 0 ? walked : 0u);
    }
}

// the fold of 256 values by halves; the block's value arrives in thread 0.  s: 256 entries of LDS per quantity
__device__ __forceinline__ void ks_fold(double &a, double &b, unsigned long long &c, double *s_a, double *s_b, unsigned long long *s_c)
{
    const uint32_t t = threadIdx.x;
    if (t >= 128) { s_a[t] = a; s_b[t] = b; s_c[t] = c; }
    __syncthreads();
    if (t < 128) { a = a + s_a[t + 128]; b = b + s_b[t + 128]; c += s_c[t + 128]; }
    if (t >= 64 && t < 128) { s_a[t] = a; s_b[t] = b; s_c[t] = c; }
    __syncthreads();
    if (t < 64) {
        a = a + s_a[t + 64]; b = b + s_b[t + 64]; c += s_c[t + 64];
#pragma unroll
        for (int h = 32; h > 0; h >>= 1) {                              // lane i < h: a[i] + a[i ^ h] = a[i] + a[i + h]
            a = a + __shfl_xor(a, h, kWave);
            b = b + __shfl_xor(b, h, kWave);
            c += (unsigned long long)__shfl_xor((long long)c, h, kWave);
        }
    }
}

// mean, deviation and threshold of the measured rows (the contract's formulas, one rounding per operation)
__device__ __forceinline__ KsRecord ks_finish(double sum, double sum_sq, unsigned long long n, double mult)
{
    KsRecord r;
    r.measured = (long long)n;
    r.sum = sum;
    r.sum_sq = sum_sq;
    if (n == 0) {
        r.mean = r.stddev = __builtin_nan("");
        r.threshold = __builtin_huge_val();
        return r;
    }
    const double N = (double)n;
    r.mean = sum / N;
    double var = 0.0;
    if (n >= 2) {
        var = (sum_sq - (sum * sum) / N) / (N - 1.0);
        if (!(var > 0.0)) var = 0.0;
    }
    r.stddev = sqrt(var);
    r.threshold = r.mean + mult * r.stddev;
    return r;
}

// One level of the tree.  FIRST: the values are the means of `count` slots (a measured judged row: its mean; every other slot:
// +0.0); otherwise they are `count` rows of the level below.  out[blockIdx.x] = this block's row; the launch with one block also
// writes the record (rec on the device, rec_host its host-mapped copy, read after the removal's wait or a stream synchronise).
template <bool FIRST>
__global__ __launch_bounds__(256) void ks_reduce_kernel(const double *__restrict__ mean, const KsPart *__restrict__ in, uint32_t count,
                                                        KsPart *__restrict__ out, double mult, KsRecord *__restrict__ rec,
                                                        KsRecord *__restrict__ rec_host)
{
    __shared__ double s_a[256], s_b[256];
    __shared__ unsigned long long s_c[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double a = 0.0, b = 0.0;
    unsigned long long c = 0;
    if (i < count) {
        if (FIRST) {
            const double m = mean[i];
            if (m < __builtin_huge_val()) { a = m; b = m * m; c = 1; }  // NaN (not judged) and +inf (not measured) compare false
        } else {
            a = in[i].sum; b = in[i].sum_sq; c = in[i].n;
        }
    }
    ks_fold(a, b, c, s_a, s_b, s_c);
    if (threadIdx.x != 0) return;
    out[blockIdx.x] = KsPart{ a, b, c };
    if (gridDim.x == 1) {
        const KsRecord r = ks_finish(a, b, c, mult);
        *rec = r;
        *rec_host = r;
        __threadfence_system();
    }
}

// pct_cloud_ring_remove_isolated: the record's threshold is the caller's
__global__ void ks_set_threshold_kernel(KsRecord *__restrict__ rec, double threshold)
{
    rec->threshold = threshold;
}

// the removal's predicate of ring_remove_kernel (ring_remove.hpp): mean[slot] as ring_knn_mean_kernel left it (NaN: not judged, +inf:
// not measured); a judged row above the record's threshold is removed -- the NaN of an unjudged slot compares false
struct KsAbove {
    const double *mean;
    const KsRecord *rec;
    __device__ __forceinline__ bool operator()(uint32_t slot, float, float, float) const { return mean[slot] > rec->threshold; }
};

}  // namespace pct
