// kernels.hpp -- gfx950 device code of the obstacle-cloud engine.
//
// Arithmetic contract (include/pct_engine.h): every distance is fp64 on float-widened
// operands, ((dx*dx + dy*dy) + dz*dz), one rounding per operation, NO fused multiply-add,
// so results are bit-identical to Utils/kdtree/src/kdtree.c:379-382 compiled for x86-64.
// The whole translation unit is built with -ffp-contract=off and this pragma repeats it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#pragma clang fp contract(off)

#include "bernstein.hpp"
#include "scan.hpp"
#include "query_bin.hpp"

namespace pct {

constexpr int kWave = 64;
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

// ((dx^2 + dy^2) + dz^2), point minus query as in kdtree.c (the sign is squared away).
__device__ __forceinline__ double dist2(double px, double py, double pz, double qx, double qy, double qz)
{
    double dx = px - qx, dy = py - qy, dz = pz - qz;
    double s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return s;
}

// total order used everywhere a winner is picked: smaller d2, then lower index
__device__ __forceinline__ bool better(double d2a, uint32_t ia, double d2b, uint32_t ib)
{
    return d2a < d2b || (d2a == d2b && ia < ib);
}

// What a query reports: a point only when its distance is < +inf.  Finite operands always have a finite d2 (at most ~1.4e78); a query
// with a NaN or infinite coordinate has no point at d2 < +inf and reports (PCT_NO_INDEX, +inf) on every path (pct_engine.h, non-finite
// input) -- the exact scans would otherwise hand such a query the lowest index they met, because better() orders +inf ties by index.
__device__ __forceinline__ uint32_t reported_index(double d2, uint32_t i, uint32_t index_base)
{
    return (i == kNoIndex || !(d2 < __builtin_huge_val())) ? kNoIndex : i + index_base;
}

__device__ __forceinline__ void wave_argmin(double &d, uint32_t &i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double od = __shfl_xor(d, off, kWave);
        uint32_t oi = (uint32_t)__shfl_xor((int)i, off, kWave);
        if (better(od, oi, d, i)) { d = od; i = oi; }
    }
}

// =====================================================================================
// 1. Streaming kernels: lanes own POINTS, queries are wave-uniform (scalar registers).
//    HBM-bound for small query tiles: the SoA cloud is read exactly once per pass with
//    16-byte-per-lane loads (three 1-KiB wave transactions per 256 points).
// =====================================================================================

// q64: [Q][3] doubles (float-widened queries).  One pass handles queries q0 .. q0+QT-1.
// Output: per-block partial winners part_d2/part_idx[(q0+j) * nparts + block].
template <int QT>
__global__ __launch_bounds__(256) void nn_stream_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ z, uint32_t n,
                                                        const double *__restrict__ q64, int q0, int qcount,
                                                        double *__restrict__ part_d2, uint32_t *__restrict__ part_idx,
                                                        int nparts)
{
    double qx[QT], qy[QT], qz[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        // tiles past the end re-use the last query (results discarded); keeps loads uniform
        int qi = q0 + (j < qcount ? j : qcount - 1);
        qx[j] = q64[3 * qi + 0];
        qy[j] = q64[3 * qi + 1];
        qz[j] = q64[3 * qi + 2];
    }
    double bd[QT];
    uint32_t bi[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) { bd[j] = __builtin_huge_val(); bi[j] = kNoIndex; }

    const uint32_t ngroups = n >> 2;
    const uint32_t stride = gridDim.x * blockDim.x;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    const float4 *y4 = reinterpret_cast<const float4 *>(y);
    const float4 *z4 = reinterpret_cast<const float4 *>(z);

    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) {
        const float4 X = x4[g], Y = y4[g], Z = z4[g];
        const float xs[4] = { X.x, X.y, X.z, X.w };
        const float ys[4] = { Y.x, Y.y, Y.z, Y.w };
        const float zs[4] = { Z.x, Z.y, Z.z, Z.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double px = (double)xs[k], py = (double)ys[k], pz = (double)zs[k];
            const uint32_t id = 4u * g + (uint32_t)k;
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const double d2 = dist2(px, py, pz, qx[j], qy[j], qz[j]);
                // indices grow within a thread, so strict < keeps the lowest index on ties
                if (d2 < bd[j]) { bd[j] = d2; bi[j] = id; }
            }
        }
    }
    // tail (n % 4 points): one lane each, in block 0
    if (blockIdx.x == 0) {
        const uint32_t id = 4u * ngroups + threadIdx.x;
        if (threadIdx.x < (n & 3u)) {
            const double px = (double)x[id], py = (double)y[id], pz = (double)z[id];
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const double d2 = dist2(px, py, pz, qx[j], qy[j], qz[j]);
                if (better(d2, id, bd[j], bi[j])) { bd[j] = d2; bi[j] = id; }
            }
        }
    }

    __shared__ double s_d[4][QT];
    __shared__ uint32_t s_i[4][QT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < QT; j++) {
        double d = bd[j];
        uint32_t i = bi[j];
        wave_argmin(d, i);
        if (lane == 0) { s_d[wave][j] = d; s_i[wave][j] = i; }
    }
    __syncthreads();
    if (threadIdx.x < QT && (int)threadIdx.x < qcount) {
        const int j = threadIdx.x;
        double d = s_d[0][j];
        uint32_t i = s_i[0][j];
#pragma unroll
        for (int w = 1; w < 4; w++)
            if (better(s_d[w][j], s_i[w][j], d, i)) { d = s_d[w][j]; i = s_i[w][j]; }
        part_d2[(size_t)(q0 + j) * nparts + blockIdx.x] = d;
        part_idx[(size_t)(q0 + j) * nparts + blockIdx.x] = i;
    }
}

// -------------------------------------------------------------------------------------
// fp32 filter + exact fp64 recheck, LDS-staged (the default brute-force path for Q > 4).
//
// Measured on MI355X: an fp64 vector op costs ~8 cycles per wave and a plain
// fp32 op ~4; only the packed v_pk_{add,mul,fma}_f32 forms reach the fp32 peak (2 lanes-worth per
// 4 cycles).  The all-fp64 kernel above needs 12 slow ops per (point, query) pair and tops out at
// 1.8e12 pairs/s.  Exactness only matters for the few points that can win, so:
//   1. nn_sample_bounds_kernel: packed-fp32 minimum over a 1/16 sample of the cloud per query.
//      ANY upper bound of the true minimum is a valid threshold; the sample only makes it tight.
//   2. nn_tile_candidates_kernel: each block stages its contiguous chunk of the SoA cloud in LDS
//      ONCE (HBM is read once per launch whatever Q is), then walks the query batch in tiles of
//      kTileQ wave-uniform queries.  Every pair is evaluated in packed fp32 on two points at a time
//      (per 4 points and query: 6 pk_add, 2 pk_mul, 4 pk_fma, min3+min, one compare).  When the
//      smallest of the four fp32 distances is <= thr = bound * (1 + 2^-19) + 2^-90 the group is
//      re-evaluated in the exact fp64 arithmetic and competes by (d2, index).  (brute2.hpp holds
//      the expanded form of the same filter, taken on large clouds.)
// Why nothing is lost: the fp32 value d32 of a pair differs from the exact d2 by < 4e-7 relative
// (correctly rounded differences, three non-negative products, two sums: no cancellation) plus
// underflow (< 2^-120 absolute).  The true winner w satisfies d2(w) <= d2(p) for the sample point
// p that set the bound, so d32(w) <= d2(w)(1+e) <= d2(p)(1+e) <= d32(p)(1+e)/(1-e) < thr.  Hence w
// and every exact tie of it always reach the fp64 path: results equal nn_stream_kernel's bit for bit.
// -------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int kSampleStride = 16;     // sample one 1024-point chunk out of every 16
constexpr int kTileQ = 8;             // wave-uniform queries per tile (7 scalar registers each)
constexpr int kSampleGroups = 4;      // sampled 256-group chunks per block of the bound kernel

struct PointGroup { v2f x01, x23, y01, y23, z01, z23; };

__device__ __forceinline__ PointGroup make_group(const float4 X, const float4 Y, const float4 Z)
{
    PointGroup g;
    g.x01 = v2f{ X.x, X.y }; g.x23 = v2f{ X.z, X.w };
    g.y01 = v2f{ Y.x, Y.y }; g.y23 = v2f{ Y.z, Y.w };
    g.z01 = v2f{ Z.x, Z.y }; g.z23 = v2f{ Z.z, Z.w };
    return g;
}

// smallest fp32 squared distance from the 4 points of g to (qx,qy,qz): 12 packed ops + min3 + min
__device__ __forceinline__ float group_min_d32(const PointGroup &g, float qx, float qy, float qz)
{
    const v2f qx2 = v2f{ qx, qx }, qy2 = v2f{ qy, qy }, qz2 = v2f{ qz, qz };
    const v2f dx01 = g.x01 - qx2, dx23 = g.x23 - qx2;
    const v2f dy01 = g.y01 - qy2, dy23 = g.y23 - qy2;
    const v2f dz01 = g.z01 - qz2, dz23 = g.z23 - qz2;
    v2f d01 = dx01 * dx01, d23 = dx23 * dx23;
    d01 = __builtin_elementwise_fma(dy01, dy01, d01);
    d23 = __builtin_elementwise_fma(dy23, dy23, d23);
    d01 = __builtin_elementwise_fma(dz01, dz01, d01);
    d23 = __builtin_elementwise_fma(dz23, dz23, d23);
    return fminf(fminf(d01.x, d01.y), fminf(d23.x, d23.y));
}

// Block-wide minimum of QT floats per thread through LDS (one transposed pass + a 32-lane
// butterfly instead of 6 cross-lane steps per value).  s_red: QT*256 floats.  Result for query j
// is returned by threads with (tid >> 5) == j, lane bit pattern (tid & 31) == 0.
template <int QT>
__device__ __forceinline__ float block_min_transposed(const float (&m)[QT], float *s_red)
{
    static_assert(QT <= 8, "one 32-lane group per query");
#pragma unroll
    for (int j = 0; j < QT; j++) s_red[j * 256 + threadIdx.x] = m[j];
    __syncthreads();
    const int j = threadIdx.x >> 5, l = threadIdx.x & 31;
    float v = __builtin_huge_valf();
    if (j < QT) {
#pragma unroll
        for (int i = 0; i < 8; i++) v = fminf(v, s_red[j * 256 + l + 32 * i]);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
    __syncthreads();
    return v;
}

// grid = sampled chunks / kSampleGroups; block b looks at kSampleGroups chunks of 256 groups, one
// every `sample_stride` chunks (the per-tile block reduction is amortised over them).  One launch
// covers the whole query batch: bound_part[q * nsblocks + b].
__global__ __launch_bounds__(256) void nn_sample_bounds_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                               const float *__restrict__ z, uint32_t n, uint32_t sample_stride,
                                                               const float *__restrict__ qf, int Q, int qslice,
                                                               float *__restrict__ bound_part, int nsblocks)
{
    __shared__ float s_red[kTileQ * 256];
    const uint32_t ngroups = n >> 2;
    const float big = __builtin_huge_valf();   // filler for slots past the end: its d32 is +inf and never lowers a bound
    PointGroup pg[kSampleGroups];
#pragma unroll
    for (int c = 0; c < kSampleGroups; c++) {
        const uint32_t g = (blockIdx.x * kSampleGroups + c) * sample_stride * 256u + threadIdx.x;
        pg[c] = make_group(make_float4(big, big, big, big), make_float4(big, big, big, big), make_float4(big, big, big, big));
        if (g < ngroups) pg[c] = make_group(reinterpret_cast<const float4 *>(x)[g], reinterpret_cast<const float4 *>(y)[g],
                                            reinterpret_cast<const float4 *>(z)[g]);
    }
    // blockIdx.y takes a slice of the batch (a multiple of kTileQ queries): small clouds have few point blocks, and the
    // tile loop below is sequential, so the batch is what fills the chip (4096 queries on 1 M points: 0.8 -> 0.1 ms)
    const int q_end = min(Q, ((int)blockIdx.y + 1) * qslice);
    for (int q0 = (int)blockIdx.y * qslice; q0 < q_end; q0 += kTileQ) {
        const int qcount = min(kTileQ, q_end - q0);
        float m[kTileQ];
#pragma unroll
        for (int j = 0; j < kTileQ; j++) {
            const int qi = q0 + (j < qcount ? j : qcount - 1);
            const float qx = qf[3 * qi], qy = qf[3 * qi + 1], qz = qf[3 * qi + 2];
            float v = group_min_d32(pg[0], qx, qy, qz);
#pragma unroll
            for (int c = 1; c < kSampleGroups; c++) v = fminf(v, group_min_d32(pg[c], qx, qy, qz));
            m[j] = v;
        }
        const float v = block_min_transposed<kTileQ>(m, s_red);
        const int j = threadIdx.x >> 5;
        if ((threadIdx.x & 31) == 0 && j < qcount) bound_part[(size_t)(q0 + j) * nsblocks + blockIdx.x] = v;
    }
}

// one block per query: fold the sample partials into the fp32 bound (bit pattern; FLT_MAX when
// the sample was empty, which makes the filter recheck everything)
__global__ __launch_bounds__(256) void bound_reduce_kernel(const float *__restrict__ bound_part, int nsblocks,
                                                           uint32_t *__restrict__ bound_bits)
{
    const float *p = bound_part + (size_t)blockIdx.x * nsblocks;
    float v = 3.402823466e+38f;
    for (int i = threadIdx.x; i < nsblocks; i += 256) v = fminf(v, p[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
    __shared__ float s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bound_bits[blockIdx.x] = __float_as_uint(fminf(fminf(s[0], s[1]), fminf(s[2], s[3])));
}

// Candidate-list form of the filter.  Keeping a running (d2, index) per lane and query and folding it per block and per tile
// of 8 queries costs two __syncthreads, a wave argmin and 8 partial writes for every tile, which at 4096 queries is 512 block
// reductions per block and, for clouds under a few million points, most of the run time; it also needs [query][block] partial
// arrays and a second kernel to fold them (retired variants).  But survivors of the fp32 bound are rare (about
// as many points as the sample stride lie closer than the closest SAMPLED point), so here a lane that holds one evaluates it
// exactly and appends (d2, index) to its query's candidate list in global memory; nothing else leaves the tile loop.
// nn_reduce_candidates_kernel then folds each list by (d2, index).  A list that overflows kCandCap entries (exact ties in
// bulk: duplicate points, lattice clouds seen from a lattice point) is queued for nn_overflow_scan_kernel, an exact scan by the
// whole grid -- rare, and still exact.
constexpr uint32_t kCandCap = 256;

__global__ __launch_bounds__(256) void nn_tile_candidates_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ z, uint32_t n, uint32_t chunk_groups,
                                                                 const float *__restrict__ qf, const double *__restrict__ q64,
                                                                 const uint32_t *__restrict__ bound_bits, int Q, int qslice,
                                                                 uint32_t *__restrict__ cand_count, double *__restrict__ cand_d2,
                                                                 uint32_t *__restrict__ cand_idx)
{
    extern __shared__ float4 s_pts[];                 // [3][chunk_groups]
    const uint32_t ngroups = n >> 2;
    const uint32_t g0 = blockIdx.x * chunk_groups;
    const uint32_t ng = min(chunk_groups, ngroups > g0 ? ngroups - g0 : 0u);
    float4 *sx = s_pts, *sy = s_pts + chunk_groups, *sz = s_pts + 2 * chunk_groups;
    for (uint32_t i = threadIdx.x; i < ng; i += 256) {
        sx[i] = reinterpret_cast<const float4 *>(x)[g0 + i];
        sy[i] = reinterpret_cast<const float4 *>(y)[g0 + i];
        sz[i] = reinterpret_cast<const float4 *>(z)[g0 + i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool tail_owner = (blockIdx.x == gridDim.x - 1) && threadIdx.x < (n & 3u);   // n % 4 leftover points

    const int q_end = min(Q, ((int)blockIdx.y + 1) * qslice);      // blockIdx.y = slice of the batch (see nn_sample_bounds_kernel)
    for (int q0 = (int)blockIdx.y * qslice; q0 < q_end; q0 += kTileQ) {
        const int qcount = min(kTileQ, q_end - q0);
        float qx[kTileQ], qy[kTileQ], qz[kTileQ], thr[kTileQ];
#pragma unroll
        for (int j = 0; j < kTileQ; j++) {
            const int qi = q0 + (j < qcount ? j : qcount - 1);
            qx[j] = qf[3 * qi]; qy[j] = qf[3 * qi + 1]; qz[j] = qf[3 * qi + 2];
            thr[j] = __uint_as_float(bound_bits[qi]) * (1.0f + 0x1p-19f) + 0x1p-90f;   // FLT_MAX bound -> +inf: everything is a candidate
        }
        for (uint32_t i = threadIdx.x; i < ng; i += 256) {
            const float4 X = sx[i], Y = sy[i], Z = sz[i];
            const PointGroup pg = make_group(X, Y, Z);
            unsigned long long hit = 0ull;
#pragma unroll
            for (int j = 0; j < kTileQ; j++) hit |= __builtin_amdgcn_ballot_w64(group_min_d32(pg, qx[j], qy[j], qz[j]) <= thr[j]);
            if (hit != 0ull) {                                 // wave-uniform: some lane holds a possible winner for some query
                if ((hit >> lane) & 1ull) {
                    const float xs[4] = { X.x, X.y, X.z, X.w }, ys[4] = { Y.x, Y.y, Y.z, Y.w }, zs[4] = { Z.x, Z.y, Z.z, Z.w };
#pragma unroll 1
                    for (int j = 0; j < qcount; j++) {
                        if (!(group_min_d32(pg, qx[j], qy[j], qz[j]) <= thr[j])) continue;
                        const int qi = q0 + j;
                        const double Qx = q64[3 * qi], Qy = q64[3 * qi + 1], Qz = q64[3 * qi + 2];
                        double bd = __builtin_huge_val();
                        uint32_t bi = kNoIndex;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const double d2 = dist2((double)xs[k], (double)ys[k], (double)zs[k], Qx, Qy, Qz);
                            if (d2 < bd) { bd = d2; bi = 4u * (g0 + i) + (uint32_t)k; }       // ids grow with k: lowest index on ties
                        }
                        const uint32_t slot = atomicAdd(&cand_count[qi], 1u);
                        if (slot < kCandCap) { cand_d2[(size_t)qi * kCandCap + slot] = bd; cand_idx[(size_t)qi * kCandCap + slot] = bi; }
                    }
                }
            }
        }
        if (tail_owner) {
            const uint32_t id = 4u * ngroups + threadIdx.x;
            const double px = (double)x[id], py = (double)y[id], pz = (double)z[id];
            for (int j = 0; j < qcount; j++) {
                const int qi = q0 + j;
                const double d2 = dist2(px, py, pz, q64[3 * qi], q64[3 * qi + 1], q64[3 * qi + 2]);
                // the true nearest neighbour is never farther than the nearest SAMPLED point, whose fp32 distance is the bound
                if (d2 <= (double)thr[j] * (1.0 + 0x1p-18) + 1e-300) {
                    const uint32_t slot = atomicAdd(&cand_count[qi], 1u);
                    if (slot < kCandCap) { cand_d2[(size_t)qi * kCandCap + slot] = d2; cand_idx[(size_t)qi * kCandCap + slot] = id; }
                }
            }
        }
    }
}

// one 256-thread block per query: fold its candidate list by (d2, index); re-zero the counter for the next slice.  A query
// whose list overflowed is queued (ovf[0] = count, ovf[1..] = queries) for the two kernels below.
__global__ __launch_bounds__(256) void nn_reduce_candidates_kernel(uint32_t *__restrict__ cand_count, const double *__restrict__ cand_d2,
                                                                   const uint32_t *__restrict__ cand_idx, uint32_t index_base,
                                                                   uint32_t *__restrict__ ovf, uint32_t *__restrict__ out_idx,
                                                                   double *__restrict__ out_d2)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    const int q = blockIdx.x;
    const uint32_t count = cand_count[q];
    if (count > kCandCap) {                                   // block-uniform
        if (threadIdx.x == 0) { ovf[1 + atomicAdd(&ovf[0], 1u)] = (uint32_t)q; cand_count[q] = 0; }
        return;
    }
    double d = __builtin_huge_val();
    uint32_t i = kNoIndex;
    if (threadIdx.x < count) { d = cand_d2[(size_t)q * kCandCap + threadIdx.x]; i = cand_idx[(size_t)q * kCandCap + threadIdx.x]; }
    wave_argmin(d, i);
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = d; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (better(s_d[w], s_i[w], d, i)) { d = s_d[w]; i = s_i[w]; }
        out_idx[q] = reported_index(d, i, index_base);
        out_d2[q] = d;
        cand_count[q] = 0;
    }
}

// Overflowed candidate lists (bulk exact ties: a sensor that accumulates the same points frame after frame, lattice clouds
// seen from a lattice point): the whole grid scans the cloud once more for just those queries, in exact fp64, each block its
// own contiguous range of points; a second kernel folds the per-block winners.  Both are launched after every slice and
// return at once when nothing overflowed (ovf[0] == 0), so the host never has to read the count back.
constexpr int kOvfBlocks = 1024;

__global__ __launch_bounds__(256) void nn_overflow_scan_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                               const float *__restrict__ z, uint32_t n, const double *__restrict__ q64,
                                                               const uint32_t *__restrict__ ovf, double *__restrict__ part_d2,
                                                               uint32_t *__restrict__ part_idx)
{
    const uint32_t count = ovf[0];
    if (count == 0) return;
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint32_t begin = min(n, blockIdx.x * per), end = min(n, begin + per);
    for (uint32_t m = 0; m < count; m++) {
        const uint32_t q = ovf[1 + m];
        const double qx = q64[3 * q], qy = q64[3 * q + 1], qz = q64[3 * q + 2];
        double d = __builtin_huge_val();
        uint32_t i = kNoIndex;
        for (uint32_t p = begin + threadIdx.x; p < end; p += 256) {
            const double d2 = dist2((double)x[p], (double)y[p], (double)z[p], qx, qy, qz);
            if (d2 < d) { d = d2; i = p; }                    // ids grow within a thread
        }
        wave_argmin(d, i);
        __syncthreads();                                      // previous round's s_d / s_i have been read
        if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = d; s_i[threadIdx.x >> 6] = i; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++)
                if (better(s_d[w], s_i[w], d, i)) { d = s_d[w]; i = s_i[w]; }
            part_d2[(size_t)m * gridDim.x + blockIdx.x] = d;
            part_idx[(size_t)m * gridDim.x + blockIdx.x] = i;
        }
    }
}

__global__ __launch_bounds__(256) void nn_overflow_fold_kernel(const uint32_t *__restrict__ ovf, const double *__restrict__ part_d2,
                                                               const uint32_t *__restrict__ part_idx, int nparts, uint32_t index_base,
                                                               uint32_t *__restrict__ out_idx, double *__restrict__ out_d2)
{
    if (blockIdx.x >= ovf[0]) return;
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    const uint32_t q = ovf[1 + blockIdx.x];
    double d = __builtin_huge_val();
    uint32_t i = kNoIndex;
    for (int p = threadIdx.x; p < nparts; p += 256) {
        const double pd = part_d2[(size_t)blockIdx.x * nparts + p];
        const uint32_t pi = part_idx[(size_t)blockIdx.x * nparts + p];
        if (better(pd, pi, d, i)) { d = pd; i = pi; }
    }
    wave_argmin(d, i);
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = d; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (better(s_d[w], s_i[w], d, i)) { d = s_d[w]; i = s_i[w]; }
        out_idx[q] = reported_index(d, i, index_base);
        out_d2[q] = d;
    }
}

// Exchange step of the sharded cloud, between its two all_reduce(min) calls: a rank stays in the race for a query only if its own
// squared distance IS the global minimum; everybody else offers INT32_MAX.  One pass instead of five elementwise kernels.
__global__ __launch_bounds__(256) void merge_mask_kernel(const double *__restrict__ d2_local, const double *__restrict__ d2_best,
                                                         const uint32_t *__restrict__ idx_local, int32_t *__restrict__ cand, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = d2_local[i];
    const uint32_t ix = idx_local[i];
    cand[i] = (d == d2_best[i] && d < __builtin_huge_val() && ix <= 0x7FFFFFFEu) ? (int32_t)ix : 0x7FFFFFFF;
}

// ---- spatially routed multi-GPU queries (include/pct_shard.h, "routed form"): every rank owns a slab of the cloud along one axis
// and answers only the queries that fall into it.  An answer travels as one 16-byte record.
struct RouteAnswer { uint32_t query, gid; double d2; };        // d2 < 0: the owner could not certify it (everybody answers it again)
constexpr int kRouteMaxWorld = 64;
struct RouteCuts { int world, axis; double cut[kRouteMaxWorld + 1]; };       // slab k = [cut[k], cut[k+1]) along `axis`; cut[0] = -inf, cut[world] = +inf

__device__ __forceinline__ int route_owner(const RouteCuts &C, double x)
{
    int k = 0;
    for (int j = 1; j < C.world; j++) k += x >= C.cut[j] ? 1 : 0;             // cuts ascend: the number of cuts at or below x
    return k;
}

// owner of every query; counts per owner (one LDS histogram per block); the queries of `rank` are compacted (any order: an answer
// carries its query's index)
__global__ __launch_bounds__(256) void route_owner_kernel(RouteCuts C, int rank, const float *__restrict__ q, uint32_t Q,
                                                          uint32_t *__restrict__ counts, uint32_t *__restrict__ mine_ids, float *__restrict__ mine_q)
{
    __shared__ uint32_t h[kRouteMaxWorld];
    __shared__ uint32_t s_base;
    if (threadIdx.x < (uint32_t)kRouteMaxWorld) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int own = -1;
    float qx = 0, qy = 0, qz = 0;
    uint32_t slot = 0;
    if (i < Q) {
        qx = q[3 * i]; qy = q[3 * i + 1]; qz = q[3 * i + 2];
        own = route_owner(C, (double)(C.axis == 0 ? qx : C.axis == 1 ? qy : qz));
        slot = atomicAdd(&h[own], 1u);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)C.world && h[threadIdx.x]) {
        const uint32_t b = atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
        if ((int)threadIdx.x == rank) s_base = b;
    }
    __syncthreads();
    if (own == rank) {
        const uint32_t p = s_base + slot;
        mine_ids[p] = i;
        mine_q[3 * p] = qx; mine_q[3 * p + 1] = qy; mine_q[3 * p + 2] = qz;
    }
}

// partitioned batches (every rank brings its OWN queries): owner of every query + counts per owner ...
__global__ __launch_bounds__(256) void route_owner_all_kernel(RouteCuts C, const float *__restrict__ q, uint32_t Q, uint32_t *__restrict__ counts,
                                                              unsigned char *__restrict__ owner)
{
    __shared__ uint32_t h[kRouteMaxWorld];
    if (threadIdx.x < (uint32_t)kRouteMaxWorld) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) {
        const int own = route_owner(C, (double)q[3 * i + C.axis]);
        owner[i] = (unsigned char)own;
        atomicAdd(&h[own], 1u);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)C.world && h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
}
// ... then the queries grouped by owner (segment k starts at off.v[k]; order inside a segment is arrival order of the atomics: every
// record carries the slot it came from)
struct RouteOffsets { uint32_t v[kRouteMaxWorld]; };
__global__ __launch_bounds__(256) void route_partition_kernel(RouteOffsets off, const unsigned char *__restrict__ owner, const float *__restrict__ q, uint32_t Q,
                                                              uint32_t *__restrict__ cursors, float *__restrict__ out_xyz, uint32_t *__restrict__ out_slot)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    const uint32_t o = owner[i];
    const uint32_t p = off.v[o] + atomicAdd(&cursors[o], 1u);
    out_xyz[3 * p] = q[3 * i]; out_xyz[3 * p + 1] = q[3 * i + 1]; out_xyz[3 * p + 2] = q[3 * i + 2];
    out_slot[p] = i;
}

// the owner's answers as records: certified when the point found is STRICTLY nearer than the edge of the slab's halo (a point just
// outside the halo at exactly that distance could tie with a lower index), otherwise flagged with d2 = -1
__global__ __launch_bounds__(256) void route_certify_kernel(int axis, double lo_edge, double hi_edge, const float *__restrict__ mine_q,
                                                            const uint32_t *__restrict__ mine_ids, uint32_t m, const uint32_t *__restrict__ lidx,
                                                            const double *__restrict__ ld2, const uint32_t *__restrict__ gid,
                                                            RouteAnswer *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double x = (double)mine_q[3 * i + axis];
    const double margin = fmin(x - lo_edge, hi_edge - x);             // +inf at the outer slabs' outer sides
    const double d2 = ld2[i];
    const bool found = lidx[i] != kNoIndex;
    const bool cert = found && margin > 0.0 && d2 < margin * margin;
    RouteAnswer a;
    a.query = mine_ids[i];
    a.gid = cert ? gid[lidx[i]] : kNoIndex;
    a.d2 = cert ? d2 : -1.0;
    out[i] = a;
}

// records -> the result arrays (each query appears exactly once); flagged queries are counted and listed
__global__ __launch_bounds__(256) void route_scatter_kernel(const RouteAnswer *__restrict__ rec, uint32_t n, uint32_t *__restrict__ out_idx,
                                                            double *__restrict__ out_d2, uint32_t *__restrict__ flag_count, uint32_t *__restrict__ flag_ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RouteAnswer a = rec[i];
    out_idx[a.query] = a.gid;
    out_d2[a.query] = a.d2;
    if (a.d2 < 0.0) flag_ids[atomicAdd(flag_count, 1u)] = a.query;
}

// second round: gather the flagged queries / map local answers to global ids / put the merged answers back
__global__ __launch_bounds__(256) void route_gather_queries_kernel(const float *__restrict__ q, const uint32_t *__restrict__ ids, uint32_t n, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = ids[i];
    out[3 * i] = q[3 * k]; out[3 * i + 1] = q[3 * k + 1]; out[3 * i + 2] = q[3 * k + 2];
}
__global__ __launch_bounds__(256) void route_to_global_kernel(uint32_t *__restrict__ lidx, uint32_t n, const uint32_t *__restrict__ gid)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && lidx[i] != kNoIndex) lidx[i] = gid[lidx[i]];
}
__global__ __launch_bounds__(256) void route_put_back_kernel(const uint32_t *__restrict__ ids, uint32_t n, const uint32_t *__restrict__ idx, const double *__restrict__ d2,
                                                             uint32_t *__restrict__ out_idx, double *__restrict__ out_d2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_idx[ids[i]] = idx[i];
    out_d2[ids[i]] = d2[i];
}

// behind the second reduction: the merged int32 candidates back to the engine's index convention (INT32_MAX = no shard holds a point)
__global__ __launch_bounds__(256) void merge_finish_kernel(const int32_t *__restrict__ cand, uint32_t *__restrict__ idx, uint32_t Q)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) idx[i] = cand[i] == 0x7FFFFFFF ? kNoIndex : (uint32_t)cand[i];
}

// one 256-thread block per query folds the per-block partials (loads issued back to back,
// compared afterwards); adds the shard's index base
__global__ __launch_bounds__(256) void nn_reduce_partials_kernel(const double *__restrict__ part_d2,
                                                                 const uint32_t *__restrict__ part_idx, int nparts,
                                                                 uint32_t index_base, uint32_t *__restrict__ out_idx,
                                                                 double *__restrict__ out_d2)
{
    const int q = blockIdx.x;
    const double *pd = part_d2 + (size_t)q * nparts;
    const uint32_t *pi = part_idx + (size_t)q * nparts;
    double d = __builtin_huge_val();
    uint32_t i = kNoIndex;
    for (int base = 0; base < nparts; base += 1024) {
        double ld[4];
        uint32_t li[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = base + k * 256 + (int)threadIdx.x;
            ld[k] = p < nparts ? pd[p] : __builtin_huge_val();
            li[k] = p < nparts ? pi[p] : kNoIndex;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (better(ld[k], li[k], d, i)) { d = ld[k]; i = li[k]; }
    }
    wave_argmin(d, i);
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = d; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; w++)
            if (better(s_d[w], s_i[w], d, i)) { d = s_d[w]; i = s_i[w]; }
        out_idx[q] = reported_index(d, i, index_base);
        out_d2[q] = d;
    }
}

// radius count, same streaming shape.  r2[j] = (double)r * (double)r (kdtree.c:273).
template <int QT>
__global__ __launch_bounds__(256) void count_stream_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, uint32_t n,
                                                           const double *__restrict__ q64, const double *__restrict__ r2,
                                                           int q0, int qcount, uint32_t *__restrict__ count)
{
    double qx[QT], qy[QT], qz[QT], rr[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        int qi = q0 + (j < qcount ? j : qcount - 1);
        qx[j] = q64[3 * qi + 0];
        qy[j] = q64[3 * qi + 1];
        qz[j] = q64[3 * qi + 2];
        rr[j] = r2[qi];
    }
    uint32_t c[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) c[j] = 0;

    const uint32_t ngroups = n >> 2;
    const uint32_t stride = gridDim.x * blockDim.x;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    const float4 *y4 = reinterpret_cast<const float4 *>(y);
    const float4 *z4 = reinterpret_cast<const float4 *>(z);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) {
        const float4 X = x4[g], Y = y4[g], Z = z4[g];
        const float xs[4] = { X.x, X.y, X.z, X.w };
        const float ys[4] = { Y.x, Y.y, Y.z, Y.w };
        const float zs[4] = { Z.x, Z.y, Z.z, Z.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double px = (double)xs[k], py = (double)ys[k], pz = (double)zs[k];
#pragma unroll
            for (int j = 0; j < QT; j++) c[j] += dist2(px, py, pz, qx[j], qy[j], qz[j]) <= rr[j] ? 1u : 0u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
        const uint32_t id = 4u * ngroups + threadIdx.x;
        const double px = (double)x[id], py = (double)y[id], pz = (double)z[id];
#pragma unroll
        for (int j = 0; j < QT; j++) c[j] += dist2(px, py, pz, qx[j], qy[j], qz[j]) <= rr[j] ? 1u : 0u;
    }
    __shared__ uint32_t s_c[4][QT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < QT; j++) {
        uint32_t v = c[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, kWave);
        if (lane == 0) s_c[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < QT && (int)threadIdx.x < qcount) {
        const int j = threadIdx.x;
        const uint32_t v = s_c[0][j] + s_c[1][j] + s_c[2][j] + s_c[3][j];
        if (v) atomicAdd(&count[q0 + j], v);
    }
}

// Order-preserving crop (lidar sensor: camera_sensor.cpp:133-145 radiusSearch + PointCloud(cloud, indices)).  A first
// version appended hits through one global cursor: it serialised on that address (~12 ns per hit, 20 K hits = 0.25 ms) and
// returned arrival order; this pair keeps insertion order and has no contended atomic:
//   crop_count_kernel    hits per 1024-point tile                                    (12 B/point read)
//   (scan_tile_sums_kernel of scan.hpp, one block: exclusive scan of the tile counts)
//   crop_scatter_kernel  recompute the test, rank inside the tile, write {index, d2, x, y, z}  (12 B/point + 32 B/hit)
constexpr int kCropTile = 1024;

__global__ __launch_bounds__(256) void crop_count_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                         const float *__restrict__ z, uint32_t n, double qx, double qy, double qz,
                                                         double r2, uint32_t *__restrict__ tile_sum)
{
    const uint32_t first = blockIdx.x * kCropTile + threadIdx.x * 4;
    uint32_t f[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = first + k;
        f[k] = (i < n && dist2((double)x[i], (double)y[i], (double)z[i], qx, qy, qz) <= r2) ? 1u : 0u;
    }
    uint32_t total;
    (void)tile_rank4(f, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void crop_scatter_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, uint32_t n, double qx, double qy, double qz,
                                                           double r2, uint32_t index_base, const uint32_t *__restrict__ tile_off,
                                                           uint32_t cap, uint32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                           float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ oz)
{
    const uint32_t first = blockIdx.x * kCropTile + threadIdx.x * 4;
    uint32_t f[4];
    double d[4];
    float px[4], py[4], pz[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = first + k;
        f[k] = 0;
        if (i < n) {
            px[k] = x[i]; py[k] = y[i]; pz[k] = z[i];
            d[k] = dist2((double)px[k], (double)py[k], (double)pz[k], qx, qy, qz);
            f[k] = d[k] <= r2 ? 1u : 0u;
        }
    }
    uint32_t total;
    uint32_t pos = tile_off[blockIdx.x] + tile_rank4(f, total);      // exclusive rank of this thread's first element
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (f[k]) {
            if (pos < cap) {
                if (out_idx) out_idx[pos] = first + k + index_base;
                if (out_d2) out_d2[pos] = d[k];
                if (ox) { ox[pos] = px[k]; oy[pos] = py[k]; oz[pos] = pz[k]; }
            }
            pos++;
        }
    }
}

// =====================================================================================
// 2. Host-layout plumbing
// =====================================================================================

// AoS(stride) staging buffer -> SoA slots [dst0, dst0+n) (ring wrap handled by the caller
// issuing two launches).  Each thread moves one point.
__global__ __launch_bounds__(256) void deinterleave_kernel(const unsigned char *__restrict__ aos, uint32_t stride_bytes,
                                                           uint32_t n, float *__restrict__ x, float *__restrict__ y,
                                                           float *__restrict__ z, uint32_t dst0)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = reinterpret_cast<const float *>(aos + (size_t)i * stride_bytes);
    x[dst0 + i] = p[0];
    y[dst0 + i] = p[1];
    z[dst0 + i] = p[2];
}

// packed xyz (12 B) fast path: 4 points = 3 float4 loads per lane -> three float4 stores
__global__ __launch_bounds__(256) void deinterleave12_kernel(const float4 *__restrict__ aos4, uint32_t ngroups,
                                                             float4 *__restrict__ x4, float4 *__restrict__ y4,
                                                             float4 *__restrict__ z4)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    const float4 a = aos4[3 * g], b = aos4[3 * g + 1], c = aos4[3 * g + 2];
    x4[g] = make_float4(a.x, a.w, b.z, c.y);
    y4[g] = make_float4(a.y, b.x, b.w, c.z);
    z4[g] = make_float4(a.z, b.y, c.x, c.w);
}

__global__ __launch_bounds__(256) void widen_queries_kernel(const float *__restrict__ q, uint32_t n3,
                                                            double *__restrict__ q64)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) q64[i] = (double)q[i];
}

__global__ __launch_bounds__(256) void square_radii_kernel(const float *__restrict__ r, uint32_t n, double *__restrict__ r2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const double w = (double)r[i]; r2[i] = w * w; }
}

__global__ __launch_bounds__(256) void fill_empty_kernel(uint32_t *__restrict__ idx, double *__restrict__ d2, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { idx[i] = kNoIndex; d2[i] = __builtin_huge_val(); }
}

// =====================================================================================
// 3. Uniform-cell index: counting sort of the cloud into cells (x fastest, then y, then z)
// =====================================================================================
struct GridDesc {
    float ox, oy, oz, inv_h;   // fp32 cell assignment (points and queries)
    double oxd, oyd, ozd, hd;  // fp64 face positions for the termination bound
    int gx, gy, gz;
    uint32_t ncells;
    // block table (optional, nullptr = none): for every corner (u, v, w) of the cell lattice, u in [0, gx] etc., the four x-runs of the
    // 2x2x2 block of cells around it -- entry 2*i = the runs' first records, 2*i + 1 = one past their last (block_corner_kernel)
    const uint4 *blocks;
};

// (cell_coord: query_bin.hpp, shared with the host)

__device__ __forceinline__ uint32_t cell_lin(const GridDesc &G, int cx, int cy, int cz)
{
    return ((uint32_t)cz * (uint32_t)G.gy + (uint32_t)cy) * (uint32_t)G.gx + (uint32_t)cx;
}

// The block table (opt-in: PCT_BLOCK_TABLE=1; measured slower than what it replaces, see engine.hip).  Stage 0 of the batch search reads
// the four x-runs of the 2x2x2 block of cells on the query's side of its cell: eight words of cell_start in four different rows of the
// table = four cache lines per query, 40 % of the line look-ups of the dense batch kernel.  The block only depends on the lattice corner
// the query is nearest to, so the build can lay the eight words of every corner side by side: one 32-byte entry, one line, no cross-lane
// broadcast -- but a table eight times the size of cell_start, which no longer lives in the L2s.  Corner (u, v, w), u in [0, gx]: cells [max(u-1, 0), min(u, gx-1)] along x, the same along y and z; a row that
// coincides with another one at the border of the grid is stored as an empty run (first == last), exactly as stage 0 computes it.
__global__ __launch_bounds__(256) void block_corner_kernel(GridDesc G, const uint32_t *__restrict__ cell_start, uint4 *__restrict__ blocks, uint32_t ncorners)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncorners) return;
    const uint32_t ux = (uint32_t)G.gx + 1u, uy = (uint32_t)G.gy + 1u;
    const int u = (int)(i % ux), v = (int)((i / ux) % uy), w = (int)(i / (ux * uy));
    const int xa = max(u - 1, 0), xb = min(u, G.gx - 1), ya = max(v - 1, 0), yb = min(v, G.gy - 1), za = max(w - 1, 0), zb = min(w, G.gz - 1);
    uint32_t s[4], e[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const bool ok = !((r >> 1) && zb == za) && !((r & 1) && yb == ya);
        const uint32_t row = cell_lin(G, 0, (r & 1) ? yb : ya, (r >> 1) ? zb : za);
        s[r] = cell_start[row + xa];
        e[r] = ok ? cell_start[row + xb + 1] : s[r];
    }
    blocks[2u * i] = make_uint4(s[0], s[1], s[2], s[3]);
    blocks[2u * i + 1u] = make_uint4(e[0], e[1], e[2], e[3]);
}

// per-block min/max -> partials[block][6]
// SKIP_REMOVED: rows whose three coordinates are all NaN (points removed from a rolling map, ring_remove.hpp) are left out
template <bool SKIP_REMOVED = false>
__global__ __launch_bounds__(256) void bbox_partial_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, uint32_t n,
                                                           float *__restrict__ partials)
{
    float lo[3] = { __builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf() };
    float hi[3] = { -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf() };
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v[3] = { x[i], y[i], z[i] };
        if (SKIP_REMOVED && v[0] != v[0] && v[1] != v[1] && v[2] != v[2]) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], v[k]); hi[k] = fmaxf(hi[k], v[k] == v[k] ? v[k] : __builtin_huge_valf()); }   // fmin / fmax drop a NaN: it shows as hi = +inf
    }
    __shared__ float s[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off, kWave));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off, kWave));
        }
        if (lane == 0) { s[wave][k] = lo[k]; s[wave][3 + k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float v = s[0][k];
        for (int w = 1; w < 4; w++) v = (k < 3) ? fminf(v, s[w][k]) : fmaxf(v, s[w][k]);
        partials[blockIdx.x * 6 + k] = v;
    }
}

__global__ __launch_bounds__(256) void cell_histogram_kernel(GridDesc G, const float *__restrict__ x,
                                                             const float *__restrict__ y, const float *__restrict__ z,
                                                             uint32_t n, uint32_t *__restrict__ cell_count,
                                                             uint32_t *__restrict__ point_cell)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t c = cell_lin(G, cell_coord(x[i], G.ox, G.inv_h, G.gx), cell_coord(y[i], G.oy, G.inv_h, G.gy),
                                    cell_coord(z[i], G.oz, G.inv_h, G.gz));
        point_cell[i] = c;
        atomicAdd(&cell_count[c], 1u);
    }
}

// exclusive scan, three launches: per-block scan of 1024-element tiles, scan of the tile sums
// (single block: scan_tile_sums_kernel of scan.hpp), then add.  cell_start has ncells+1 entries; entry ncells = n.
constexpr int kScanTile = 1024;

__global__ __launch_bounds__(256) void scan_tiles_kernel(const uint32_t *__restrict__ in, uint32_t n,
                                                         uint32_t *__restrict__ out, uint32_t *__restrict__ tile_sum)
{
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (base + k < n) ? in[base + k] : 0u;
    uint32_t total;
    uint32_t run = tile_rank4(v, total);    // exclusive prefix of this thread within the tile
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void scan_add_kernel(uint32_t *__restrict__ out, uint32_t n,
                                                       const uint32_t *__restrict__ tile_sum, uint32_t total)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += tile_sum[i / kScanTile];
    if (i == 0) out[n] = total;
}

// sorted[pos] = (x, y, z, bit-cast original index); order inside a cell is arbitrary, which
// is harmless because every consumer picks winners by (d2, index) or counts.
__global__ __launch_bounds__(256) void cell_scatter_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, uint32_t n,
                                                           const uint32_t *__restrict__ point_cell,
                                                           const uint32_t *__restrict__ cell_start,
                                                           uint32_t *__restrict__ cell_fill, float4 *__restrict__ sorted)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t c = point_cell[i];
        const uint32_t pos = cell_start[c] + atomicAdd(&cell_fill[c], 1u);
        sorted[pos] = make_float4(x[i], y[i], z[i], __uint_as_float(i));
    }
}

// Query binning for the cell-pruned kernels: a counting sort of the batch by coarse cell (BinDesc, query_bin<FAST>: query_bin.hpp,
// where the bin order and its two forms are described; FAST is the host's choice per cloud, B.fast).
//
// Counting sort of the batch on LDS histograms (a global-atomic version ran 2 M scattered
// device-scope atomics at ~20 G/s = 100 us per 1 M queries).  key = bin >> key_shift (< 2^20);
// bucket = key >> kSortLShift (<= 1024 buckets), queries left in arrival order inside a bucket.
// Global atomics are one per (block, non-empty bucket); everything else is LDS atomics and
// coalesced traffic.
constexpr int kSortBuckets = 1024;
constexpr int kSortLShift = 10;          // finer buckets (key >> 8, >> 9) measured the same
constexpr int kSortItems = 8;            // queries per thread in the sort kernels
constexpr int kSortPerBlock = 1024 * kSortItems;      // most queries per block in the sort kernels (engine.hip picks 1024..8192 by batch size)

// A thread's kSortItems queries of the sort kernels.  VEC (the query array is 16-byte aligned): the thread owns chunks of 4 CONSECUTIVE
// queries and fetches each chunk as three float4 (48 contiguous bytes) instead of twelve dwords at a stride of 12 bytes: a quarter of the
// load instructions.  Item k of thread `tid` is query sort_item<VEC>(base, k, tid); an item is live when sort_item_live says so.
// FULL: the block owns kSortPerBlock queries and all of them exist (one block-uniform test in the kernels, sort_block_full): every item
// of every thread is live, so nothing below is tested per item -- no exec-mask save / branch pair around each item, no sentinel key.
// At 1 M queries every block is such a block; the ragged last block and the smaller batches (fewer than kSortItems items) take FULL = false.
__device__ __forceinline__ bool sort_block_full(uint32_t base, uint32_t per_block, uint32_t Q)
{
    return per_block == (uint32_t)kSortPerBlock && Q - base >= per_block;      // base < Q: the launch has ceil(Q / per_block) blocks
}
template <bool VEC>
__device__ __forceinline__ uint32_t sort_item(uint32_t base, int k, uint32_t tid)
{
    return VEC ? base + 4u * (tid + 1024u * (uint32_t)(k >> 2)) + (uint32_t)(k & 3) : base + (uint32_t)k * 1024u + tid;
}
template <bool VEC, bool FULL = false>
__device__ __forceinline__ bool sort_item_live(uint32_t base, int k, uint32_t tid, int items, uint32_t Q)
{
    if (FULL) return true;
    if (VEC) return (tid + 1024u * (uint32_t)(k >> 2)) < 256u * (uint32_t)items && sort_item<true>(base, k, tid) < Q;
    return k < items && sort_item<false>(base, k, tid) < Q;
}
template <bool VEC, bool FULL>
__device__ __forceinline__ void sort_load_items(const float *__restrict__ q, uint32_t base, uint32_t tid, int items, uint32_t Q, float (&qv)[kSortItems][3])
{
    if (VEC) {
#pragma unroll
        for (int g = 0; g < kSortItems / 4; g++) {
            const uint32_t t0 = sort_item<true>(base, 4 * g, tid);
            if (FULL || ((tid + 1024u * (uint32_t)g) < 256u * (uint32_t)items && t0 + 3u < Q)) {       // base is a multiple of 1024: 3 * t0 floats = a multiple of 12
                const float4 *v = reinterpret_cast<const float4 *>(q + 3 * (size_t)t0);
                const float4 A = v[0], B = v[1], C = v[2];
                qv[4 * g][0] = A.x; qv[4 * g][1] = A.y; qv[4 * g][2] = A.z;
                qv[4 * g + 1][0] = A.w; qv[4 * g + 1][1] = B.x; qv[4 * g + 1][2] = B.y;
                qv[4 * g + 2][0] = B.z; qv[4 * g + 2][1] = B.w; qv[4 * g + 2][2] = C.x;
                qv[4 * g + 3][0] = C.y; qv[4 * g + 3][1] = C.z; qv[4 * g + 3][2] = C.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = 4 * g + j;
                    const uint32_t t = sort_item<true>(base, k, tid);
                    const bool ok = sort_item_live<true>(base, k, tid, items, Q);
                    qv[k][0] = ok ? q[3 * (size_t)t] : 0.0f; qv[k][1] = ok ? q[3 * (size_t)t + 1] : 0.0f; qv[k][2] = ok ? q[3 * (size_t)t + 2] : 0.0f;
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kSortItems; k++) {
            const uint32_t t = sort_item<false>(base, k, tid);
            const bool ok = sort_item_live<false, FULL>(base, k, tid, items, Q);
            qv[k][0] = ok ? q[3 * t] : 0.0f; qv[k][1] = ok ? q[3 * t + 1] : 0.0f; qv[k][2] = ok ? q[3 * t + 2] : 0.0f;
        }
    }
}

// the histogram pass over one block's items: bucket = bin >> bshift (key_shift + kSortLShift: the key itself is never needed)
template <bool VEC, bool FAST, bool FULL>
__device__ __forceinline__ void qsort_hist_items(const BinDesc &B, int bshift, const float *__restrict__ q, uint32_t Q, uint32_t base, int items,
                                                 uint32_t *h)
{
    // all of a thread's queries are requested before the first is used: the loop used to pay one memory round trip per item
    float qv[kSortItems][3];
    sort_load_items<VEC, FULL>(q, base, threadIdx.x, items, Q, qv);
#pragma unroll
    for (int k = 0; k < kSortItems; k++)
        if (sort_item_live<VEC, FULL>(base, k, threadIdx.x, items, Q))
            atomicAdd(&h[query_bin<FAST>(B, qv[k][0], qv[k][1], qv[k][2]) >> bshift], 1u);     // recomputed by the scatter pass
}

// Two dependent launches per batch (hist -> scatter1); at <= 256 K queries the sort is launch-latency-bound, so the bucket scan
// lives inside scatter1 and the counter arrays are re-zeroed without extra launches where possible: total1 is zero on entry
// (zeroed at allocation, then by the previous batch's hist pass through total1_next, or by a memset behind scatter1 when the
// batch is captured).
// A block's slice of each bucket comes from the histogram pass: the atomic that adds the block's count to total1[i] returns what the
// blocks before it (in arrival order, which is arbitrary) have added, and that is the block's offset inside bucket i.  It goes to
// slice[block * kSortBuckets + i] (0 where the block has nothing in the bucket), one coalesced row of 4 KB per block; scatter1 block b
// reads row b, after the launch boundary.  Invariants: total1 is zero when a hist pass starts (zeroed by whom: see above) and complete
// when scatter1 starts; every hist launch rewrites the rows of its own blocks in full, so slice is never zeroed, and rows beyond the
// launch's block count hold leftovers that no block of this launch reads; the table has a row for every block a reserved batch can
// have (engine.hip sort_slice_rows).  No global atomic and no counter of its own is left in the scatter pass.
template <bool VEC, bool FAST>
__global__ __launch_bounds__(1024) void qsort_hist_kernel(BinDesc B, int key_shift, const float *__restrict__ q,
                                                          uint32_t Q, uint32_t per_block,
                                                          uint32_t *__restrict__ total1, uint32_t *__restrict__ slice,
                                                          uint32_t *__restrict__ total1_next)
{
    __shared__ uint32_t h[kSortBuckets];
    if (blockIdx.x == 0 && total1_next)
        for (int i = threadIdx.x; i < kSortBuckets; i += 1024)
            total1_next[i] = 0;                       // the next batch's totals (its last reader finished a batch ago): no memset on the path
    for (int i = threadIdx.x; i < kSortBuckets; i += 1024) h[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * per_block;
    const int items = (int)(per_block >> 10);             // per_block is a multiple of 1024, at most kSortPerBlock
    const int bshift = key_shift + kSortLShift;
    if (sort_block_full(base, per_block, Q)) qsort_hist_items<VEC, FAST, true>(B, bshift, q, Q, base, items, h);
    else qsort_hist_items<VEC, FAST, false>(B, bshift, q, Q, base, items, h);
    __syncthreads();
    uint32_t *row = slice + (size_t)blockIdx.x * kSortBuckets;
    for (int i = threadIdx.x; i < kSortBuckets; i += 1024)
        row[i] = h[i] ? atomicAdd(&total1[i], h[i]) : 0u;      // what was there before: this block's offset inside bucket i
}

// the scatter pass over one block's items (every thread of the block goes the same way: the barrier is block-uniform).  On entry
// h[] is zero and visible to the block, and thread i has written basepos[i] = the first position of this block's slice of bucket i.
// An item's position is basepos[bucket] + its rank inside (block, bucket); h need not be complete before a thread writes.
template <bool VEC, bool FAST, bool FULL>
__device__ __forceinline__ void qsort_scatter_items(const BinDesc &B, int bshift, const float *__restrict__ q, uint32_t Q, uint32_t base, int items,
                                                    float4 *__restrict__ qsorted, uint32_t *h, const uint32_t *basepos)
{
    // all of a thread's queries are requested up front (one round trip instead of one per item)
    uint32_t bucket[kSortItems];                      // 0xFFFFFFFF: no such item (never with FULL)
    float qv[kSortItems][3];
    sort_load_items<VEC, FULL>(q, base, threadIdx.x, items, Q, qv);
#pragma unroll
    for (int k = 0; k < kSortItems; k++)
        bucket[k] = sort_item_live<VEC, FULL>(base, k, threadIdx.x, items, Q) ? query_bin<FAST>(B, qv[k][0], qv[k][1], qv[k][2]) >> bshift : 0xFFFFFFFFu;
    __syncthreads();                                  // publishes basepos[]; the only barrier of the pass, and in front of the ranks
    // the histogram atomic's return value IS the query's rank inside (block, bucket): one LDS atomic per query, not two
    uint32_t rank[kSortItems];
#pragma unroll
    for (int k = 0; k < kSortItems; k++)
        if (FULL || bucket[k] != 0xFFFFFFFFu) rank[k] = atomicAdd(&h[bucket[k]], 1u);
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        if (FULL || bucket[k] != 0xFFFFFFFFu) {
            const uint32_t t = sort_item<VEC>(base, k, threadIdx.x);
            const uint32_t pos = basepos[bucket[k]] + rank[k];
            qsorted[pos] = make_float4(qv[k][0], qv[k][1], qv[k][2], __uint_as_float(t));
        }
    }
}

// scatter: qsorted[pos] = {qx, qy, qz, bitcast(id)}, so the search kernels get a query and its output slot with ONE 16-byte load.
// Every block scans the 1024 bucket totals itself (thread i = bucket i) instead of waiting for a one-block scan kernel.
template <bool VEC, bool FAST>
__global__ __launch_bounds__(1024) void qsort_scatter1_kernel(BinDesc B, int key_shift, const float *__restrict__ q,
                                                              uint32_t Q, uint32_t per_block, const uint32_t *__restrict__ total1,
                                                              const uint32_t *__restrict__ slice, float4 *__restrict__ qsorted)
{
    static_assert(kSortBuckets == 1024, "one thread per bucket");
    __shared__ uint32_t h[kSortBuckets];
    __shared__ uint32_t basepos[kSortBuckets];
    h[threadIdx.x] = 0;                               // (published by the scan's barrier)
    const uint32_t mine = slice[(size_t)blockIdx.x * kSortBuckets + threadIdx.x];      // this block's offset inside bucket i (the hist pass)
    uint32_t all;
    const uint32_t start = block_exclusive<uint32_t, 1024>(total1[threadIdx.x], all);
    basepos[threadIdx.x] = start + mine;              // (published by the barrier in qsort_scatter_items)
    const uint32_t base = blockIdx.x * per_block;
    const int items = (int)(per_block >> 10);
    const int bshift = key_shift + kSortLShift;
    if (sort_block_full(base, per_block, Q)) qsort_scatter_items<VEC, FAST, true>(B, bshift, q, Q, base, items, qsorted, h, basepos);
    else qsort_scatter_items<VEC, FAST, false>(B, bshift, q, Q, base, items, qsorted, h, basepos);
}

// =====================================================================================
// 4. Cell-pruned kernels: the search walks an expanding cube of cells around the query.
//    Termination is exact: a point outside the scanned cube of cells is at least
//    `bound` away (distance to the cube's faces, minus a slack covering the fp32 cell
//    assignment rounding), so the search stops once best_d2 <= bound^2.
// =====================================================================================
struct WorkCounters { unsigned long long points, cells, nodes; };    // nodes: pyramid node visits (pyramid.hpp), 8 boxes of 32 bytes each
constexpr int kWorkSlots = 64;    // instrumented kernels spread their two counters over 64 slots (same-address atomics serialise)

// XCD-aware block order (cdna_hip_programming.md T1).  Workgroups are dealt round-robin over
// the 8 XCDs, each with a private 4 MiB L2.  With the batch binned in cell order, giving XCD k
// the k-th contiguous eighth of the blocks keeps the three cell planes a stretch of queries
// needs inside ONE L2 instead of spreading every plane over all eight.  Bijective for any grid
// size; placement is a speed matter only.
__device__ __forceinline__ uint32_t xcd_contiguous_block(uint32_t b, uint32_t nblocks)
{
    const uint32_t xcd = b & 7u, k = b >> 3;
    const uint32_t q = nblocks >> 3, r = nblocks & 7u;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// the cell of a query (or of any fp32 position): cell_coord per axis
__device__ __forceinline__ void query_cell(const GridDesc &G, float qxf, float qyf, float qzf, int &cx, int &cy, int &cz)
{
    cx = cell_coord(qxf, G.ox, G.inv_h, G.gx);
    cy = cell_coord(qyf, G.oy, G.inv_h, G.gy);
    cz = cell_coord(qzf, G.oz, G.inv_h, G.gz);
}

// distance from q to the nearest face of the box of cells [xa, xb] x [ya, yb] x [za, zb] that still has cells behind it
// (+inf when the box covers the whole grid), minus the slack that covers the fp32 cell assignment.  The ONE termination bound of the
// cell-pruned searches: a search that has seen every record of the box stops once its best (or k-th best) is within the bound.
__device__ __forceinline__ double box_bound(const GridDesc &G, int xa, int xb, int ya, int yb, int za, int zb, double qx, double qy, double qz)
{
    double bound = __builtin_huge_val();
    if (xa > 0) bound = fmin(bound, qx - (G.oxd + (double)xa * G.hd));
    if (xb < G.gx - 1) bound = fmin(bound, (G.oxd + (double)(xb + 1) * G.hd) - qx);
    if (ya > 0) bound = fmin(bound, qy - (G.oyd + (double)ya * G.hd));
    if (yb < G.gy - 1) bound = fmin(bound, (G.oyd + (double)(yb + 1) * G.hd) - qy);
    if (za > 0) bound = fmin(bound, qz - (G.ozd + (double)za * G.hd));
    if (zb < G.gz - 1) bound = fmin(bound, (G.ozd + (double)(zb + 1) * G.hd) - qz);
    return bound == __builtin_huge_val() ? bound : bound - G.hd * (1.0 / 256.0);
}
// ... of the cube of cells [c-r, c+r]^3
__device__ __forceinline__ double cube_bound(const GridDesc &G, int cx, int cy, int cz, int r, double qx, double qy, double qz)
{
    return box_bound(G, cx - r, cx + r, cy - r, cy + r, cz - r, cz + r, qx, qy, qz);
}

// -------------------------------------------------------------------------------------
// Cooperative form of the cell-pruned NN: EIGHT lanes per query (8 queries per wave).
//
// A lane-per-query search is bound by the vector L1's address path, not by arithmetic or DRAM
// (measured: ~150 L1 accesses per query, texture-address unit busy 65 % of the kernel): a lane
// reading the 6 points of a run one after the other issues 6 separate 16-byte accesses to the
// SAME 128-byte line.  Here the 8 lanes of a group read 8 consecutive points of a run with one
// coalesced 128-byte access, the 9 rows' cell_start entries are fetched by 9 different lanes at
// once, and the three rows of a z-plane are requested before any is consumed.
// -------------------------------------------------------------------------------------
constexpr int kCoop = 8;

// Cross-lane traffic inside a group of 8 lanes goes through DPP (data-parallel primitives: the operand of a VALU instruction is read
// from another lane of the same row) instead of ds_bpermute (an LDS instruction with its issue slot, ~50+ cycles of latency and an
// lgkmcnt wait): the folds below sit on every query's critical path.
constexpr int kDppXor1 = 0xB1;         // quad_perm [1, 0, 3, 2]
constexpr int kDppXor2 = 0x4E;         // quad_perm [2, 3, 0, 1]
constexpr int kDppHalfMirror = 0x141;  // lane i <-> 7 - i inside every 8 lanes: pairs the two quads of a group
constexpr int kDppQuadBcast0 = 0x00, kDppQuadBcast1 = 0x55, kDppQuadBcast2 = 0xAA, kDppQuadBcast3 = 0xFF;    // quad_perm [k, k, k, k]
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))); }
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double((long long)(((uint64_t)dpp_u32<CTRL>((uint32_t)(b >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)b)));
}

// (measured on the dense batch kernel: the DPP form of the folds below costs registers -- 64 VGPRs + 16 bytes of scratch at 8 waves per
// SIMD -- and the kernel ran 0.131 instead of 0.122 ms; at the present 7 waves / 72 VGPRs DPP folds + quad broadcasts of the run bounds
// measure the same as ds_bpermute, 0.1161-0.1163 against 0.1166-0.1167 ms, as does reading a +inf pad record instead of clamping and
// masking the slots beyond a run, 0.1156-0.1171 (profiles/r03_ab_dpp.txt).  They stay on the LDS pipe; the pyramid walk uses the DPP
// forms: 1.06 against 1.09 ms.)
//
// The exchanges of the 8-lane folds stay on the LDS pipe but as ds_swizzle in bit mode (source lane = ((lane & and) | or) ^ xor inside
// every 32 lanes, the pattern an immediate) instead of __shfl_xor(v, off, 64), which is a ds_bpermute whose byte index costs
// v_xor + v_cmp + v_cndmask + v_lshlrev per offset and three index registers kept live across the fold and the exact path.
// ds_swizzle, like ds_bpermute, returns 0 for a source lane that is switched off, so these helpers may only run where all 8 lanes of a
// group are active together.  That holds wherever they are used: `live` / `slot < Q` are uniform per group, the band test that selects
// the exact path is evaluated on folded (group-uniform) values, and the tail loops' T comes from run bounds every lane of the group holds.
constexpr int swz_xor(int off) { return (off << 10) | 0x1F; }          // lane ^ off                (and 0x1F, or 0, xor off)
constexpr int swz_group_lane(int k) { return (k << 5) | 0x18; }       // lane k of the 8-lane group (and 0x18, or k, xor 0)
template <int PATTERN>
__device__ __forceinline__ uint32_t swz_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, PATTERN); }
template <int PATTERN>
__device__ __forceinline__ float swz_f32(float v) { return __uint_as_float(swz_u32<PATTERN>(__float_as_uint(v))); }
template <int PATTERN>
__device__ __forceinline__ double swz_f64(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double((long long)(((uint64_t)swz_u32<PATTERN>((uint32_t)(b >> 32)) << 32) | swz_u32<PATTERN>((uint32_t)b)));
}

template <int OFF>
__device__ __forceinline__ void coop_argmin8_step(double &d, uint32_t &i)
{
    const double od = swz_f64<swz_xor(OFF)>(d);
    const uint32_t oi = swz_u32<swz_xor(OFF)>(i);
    if (better(od, oi, d, i)) { d = od; i = oi; }
}
__device__ __forceinline__ void coop_argmin8(double &d, uint32_t &i)
{
    coop_argmin8_step<1>(d, i);
    coop_argmin8_step<2>(d, i);
    coop_argmin8_step<4>(d, i);
}

// Element i of an array through a 32-bit byte offset from the (wave-uniform, scalar) base: global_load v, v_off, s[base] -- one shift.
// base[i] with a uint32_t i is a zero-extended 64-bit address per lane instead: a v_mov of 0 and a v_lshl_add_u64 per access, two
// registers per address.  The byte offset wraps at 2^32, so NARROW is only for arrays of at most 2^32 bytes: the host decides
// (narrow_offsets_fit), never a branch in the kernel.
template <bool NARROW, typename T>
__device__ __forceinline__ T ld_at(const T *__restrict__ base, uint32_t i)
{
    if constexpr (NARROW) return *(const T *)((const char *)base + (size_t)(uint32_t)(i * (uint32_t)sizeof(T)));
    else return base[i];
}
template <bool NARROW, typename T>
__device__ __forceinline__ void st_at(T *__restrict__ base, uint32_t i, T v)
{
    if constexpr (NARROW) *(T *)((char *)base + (size_t)(uint32_t)(i * (uint32_t)sizeof(T))) = v;
    else base[i] = v;
}

// ---- the parts every 8-lanes-per-query batch kernel of the cell index is made of (this file, knn.hpp, rsearch.hpp, pyramid.hpp) ----
// The batch slot of the calling lane's group, GROUPS queries per block: the blocks of a sorted batch in XCD-contiguous order.
template <int GROUPS>
__device__ __forceinline__ uint32_t coop_slot(const float4 *qsorted)
{
    const uint32_t bslot = qsorted ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    return bslot * GROUPS + (threadIdx.x / kCoop);
}

// The query of batch slot `slot`; returns the row its answer goes to.  Sorted batch: query and row in one 16-byte record.
// (No __restrict__ on the parameters of these helpers: the kernels' own pointers carry it, and a second scope on the inlined copy lets the
// compiler merge the two branches' loads -- the dense kernel then fetched its sorted record as four dwords.)
template <bool NARROW = false>
__device__ __forceinline__ uint32_t coop_fetch_query(const float4 *qsorted, const float *q, uint32_t slot, float &qxf, float &qyf, float &qzf)
{
    uint32_t t = slot;
    if (qsorted) {
        const float4 R = ld_at<NARROW>(qsorted, slot);
        qxf = R.x; qyf = R.y; qzf = R.z; t = __float_as_uint(R.w);
    } else {
        qxf = q[3 * t]; qyf = q[3 * t + 1]; qzf = q[3 * t + 2];
    }
    return t;
}

// One lane's run [s, e) of row (yy, zz) over the cells [x0, x1]; a row that is switched off (!ok: beyond the rows of its box, or one
// that coincides with another at the grid's border) reads row 0 and comes out empty.
__device__ __forceinline__ void row_run(const GridDesc &G, const uint32_t *cell_start, bool ok, int yy, int zz, int x0, int x1,
                                        uint32_t &s, uint32_t &e)
{
    const uint32_t row = ok ? cell_lin(G, 0, yy, zz) : 0u;
    const uint32_t a = cell_start[row + x0], b = cell_start[row + x1 + 1];
    s = a;
    e = ok ? b : a;
}

// The x-runs of row (yy, zz) that belong to the shell of Chebyshev radius r around cell (cx, cy, cz), f(s, e) for each: the whole row
// from cx - r to cx + r, clamped to the grid, where the row lies on a y or z face of the cube (or `full`: the cube itself is wanted), else the
// two end cells cx - r and cx + r, each where the grid has it.  The callers loop over the rows of the clamped cube in their own order.
template <typename F>
__device__ __forceinline__ void shell_row_runs(const GridDesc &G, const uint32_t *cell_start, int cx, int cy, int cz, int r, bool full,
                                               int yy, int zz, const F &f)
{
    const int xl = cx - r, xh = cx + r;
    const uint32_t row = cell_lin(G, 0, yy, zz);
    if (full || zz == cz - r || zz == cz + r || yy == cy - r || yy == cy + r) {
        f(cell_start[row + max(xl, 0)], cell_start[row + min(xh, G.gx - 1) + 1]);
    } else {
        if (xl >= 0) f(cell_start[row + xl], cell_start[row + xl + 1]);
        if (xh <= G.gx - 1) f(cell_start[row + xh], cell_start[row + xh + 1]);
    }
}

// The two work counters of an instrumented launch: summed over the wave, one pair of atomics per wave into the block's slot.
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, kWave);
    return v;
}
__device__ __forceinline__ void commit_work(WorkCounters *work, uint32_t npts, uint32_t nruns)
{
    const unsigned long long a = wave_sum(npts), b = wave_sum(nruns);
    if ((threadIdx.x & 63) == 0) { WorkCounters *w = work + (blockIdx.x & (kWorkSlots - 1)); atomicAdd(&w->points, a); atomicAdd(&w->cells, b); }
}

// exact scan of [s, e) shared by the 8 lanes of a group (lane `sub` takes s+sub, s+sub+8, ...)
__device__ __forceinline__ void coop_scan_exact(const float4 *__restrict__ pts, uint32_t s, uint32_t e, uint32_t sub, double qx,
                                                double qy, double qz, double &bd, uint32_t &bi)
{
    for (uint32_t p = s + sub; p < e; p += kCoop) {
        const float4 P = pts[p];
        const double d2 = dist2((double)P.x, (double)P.y, (double)P.z, qx, qy, qz);
        const uint32_t id = __float_as_uint(P.w);
        if (better(d2, id, bd, bi)) { bd = d2; bi = id; }
    }
}

// rows of the shell of Chebyshev radius r around cell (cx,cy,cz), shared by 8 lanes
template <bool COUNT>
__device__ __forceinline__ void coop_scan_shell(const GridDesc &G, const float4 *__restrict__ pts,
                                                const uint32_t *__restrict__ cell_start, int cx, int cy, int cz, int r,
                                                uint32_t sub, double qx, double qy, double qz, double &bd,
                                                uint32_t &bi, uint32_t &npts, uint32_t &nruns)
{
    const int y0 = max(cy - r, 0), y1 = min(cy + r, G.gy - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, G.gz - 1);
    for (int zz = z0; zz <= z1; zz++)
        for (int yy = y0; yy <= y1; yy++)
            shell_row_runs(G, cell_start, cx, cy, cz, r, false, yy, zz, [&](uint32_t s, uint32_t e) {
                if (COUNT && sub == 0) { npts += e - s; nruns += 1; }
                coop_scan_exact(pts, s, e, sub, qx, qy, qz, bd, bi);
            });
}

// fp32 screening of NR x-runs by the 8 lanes of a group (min, runner-up, position), then the exact fp64 winner: if the
// runner-up lies outside the fp32 error band the minimum IS the exact winner and is evaluated once in fp64, otherwise the
// runs are rescanned in exact arithmetic.  All NR rows are requested before any is consumed (the kernel is bound by
// dependent memory round trips: one for the bounds, one for the points).  Leaves (bd, bi) = (+inf, none) for empty runs.
// The clamp keeps the lanes beyond a run on the run's last cache line (reading the slots behind the run unclamped measured slower:
// DESIGN.md, retired variants).
//
// TAIL (stage 0 of the dense batch kernel): one more slot per lane, shared by the NR runs and requested together with the main ones.
// A run longer than its 8 * DEPTH main slots has a tail of t_k = len_k - 8 * DEPTH records; a rolled loop per run takes a tail in
// dependent round trips with nothing else of the wave in flight (2.2 such trips per wave at 6 points per cell).  With T = sum of the
// t_k -- computed from the run bounds, which every lane of the group holds: no shuffles -- a group with T <= 8 gives lane `sub` the
// tail record number `sub` in run order (the run whose prefix range [sum of t before k, + t_k) holds it) and masks the lanes
// sub >= T to +inf; those read their last main slot again (a line the group touches anyway).  A group with T > 8 (0.7 % of the
// queries) masks the slot off altogether and keeps the loops for ALL its tails, so no record is screened twice.
// Results cannot change: the same set of records -- every record of the NR runs, once -- goes through the same fp32 expression into
// the same (m1, m2, p1) update, only in another order, and min / runner-up are order-independent up to WHICH of several equal minima
// p1 names; equal minima have m2 == m1, fail the band test below and go to the exact rescan, which orders by (d2, index) in fp64.
// So whenever fp32 cannot decide, exact arithmetic does, as before.
//
// The clamp is min(position, b - 1) with b - 1 WRAPPING for b == 0 (no compare per run, no select per slot for the empty run).  An empty
// run [a, a) with a > 0 sends its lanes to record a - 1, a live record; an empty run at the start of the array (a == b == 0) leaves the
// positions unclamped: sub + 8 j <= 8 DEPTH - 1 <= 15 < kGridPad, and the record array is allocated with kGridPad records behind the
// n written ones (gridbuild.hpp; the cloud's cell-sorted array is the only one that reaches this function), so the read stays inside
// the allocation even for a cloud of one point.  Either way p < b fails and the slot is masked to +inf: what was read never reaches a
// result.
//
// NARROW: the record reads of the screening (main slots, tail slot, long rows, the winner's reload) take 32-bit byte offsets (ld_at).
template <int NR, int DEPTH, bool TAIL = false, bool NARROW = false>
__device__ __forceinline__ void coop_screen_rows(const float4 *__restrict__ pts, const uint32_t (&rs)[NR], const uint32_t (&re)[NR],
                                                 uint32_t sub, float qxf, float qyf, float qzf, double qx, double qy, double qz,
                                                 double &bd, uint32_t &bi)
{
    // TAIL only (the dense batch kernel; the pyramid's stage 0 keeps the compiler's choice): the three differences of a slot are made
    // opaque where they are formed, which keeps the SLP vectoriser from pairing the slots' subtractions.  Left alone it packs two slots
    // into v_pk_add / v_pk_mul / v_pk_fma_f32 and pays for it with moves: the loaded records shuffled into aligned register pairs and a
    // second copy of the query kept in pairs.  Straight path of the narrow form (entry to the tail_loops branch): packed 270 vector
    // instructions with 27 v_pk_*, 36 v_mov_b32 and 16 s_nop, 65 VGPRs; pinned 261 with 12 v_pk_* (the squares still pair up), 14
    // v_mov_b32 and 14 s_nop, 64 VGPRs, all nine record loads still before the first s_waitcnt vmcnt (profiles/r08_stage0_asm.txt).
    // The pin is an empty asm, not volatile: no instruction of its own.  The same expression in the same order, v_fma_f32 rounds as
    // v_pk_fma_f32 does and nothing contracts (-ffp-contract=off): (m1, m2, p1) are the same bits.
    constexpr bool kUnpacked = TAIL;
    float m1 = __builtin_huge_valf(), m2 = __builtin_huge_valf();
    uint32_t p1 = 0;
    // DEPTH points per lane and row (8 * DEPTH per row for the group) are requested up front
    float4 P[NR][DEPTH];
#pragma unroll
    for (int k = 0; k < NR; k++) {
        const uint32_t a = rs[k], b = re[k];
        const uint32_t last = b - 1u;                           // wraps for b == 0; an empty row reads a record that is masked below (see above)
#pragma unroll
        for (int j = 0; j < DEPTH; j++) P[k][j] = ld_at<NARROW>(pts, min(a + sub + kCoop * j, last));
    }
    uint32_t tp = 0;                                              // the shared tail slot: position, in use, the group takes the loops instead
    bool tail_on = false, tail_loops = false;
    float4 PT = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (TAIL) {
        constexpr uint32_t kMain = kCoop * DEPTH;
        uint32_t T = 0;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            const uint32_t t = max(re[k] - rs[k], kMain) - kMain;
            tp = sub >= T ? rs[k] + kMain + (sub - T) : tp;          // T = exclusive prefix here: the last run with prefix <= sub holds the lane's record
            T += t;
        }
        tail_on = sub < T && T <= (uint32_t)kCoop;
        tail_loops = T > (uint32_t)kCoop;
        const uint32_t a = rs[NR - 1], b = re[NR - 1];
        tp = tail_on ? tp : min(a + sub + kCoop * (DEPTH - 1), b - 1u);   // idle: the lane's last main slot again (same wrapping clamp)
        PT = ld_at<NARROW>(pts, tp);
    }
#pragma unroll
    for (int k = 0; k < NR; k++) {
        const uint32_t a = rs[k], b = re[k];
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            const uint32_t p = a + sub + kCoop * j;
            float dx = P[k][j].x - qxf, dy = P[k][j].y - qyf, dz = P[k][j].z - qzf;
            if constexpr (kUnpacked) asm("" : "+v"(dx), "+v"(dy), "+v"(dz));
            float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            d = (p < b) ? d : __builtin_huge_valf();
            const bool lt = d < m1;
            m2 = __builtin_amdgcn_fmed3f(m1, m2, d);            // second smallest of {m1 <= m2, d}
            p1 = lt ? p : p1;
            m1 = fminf(m1, d);
        }
    }
    // rows longer than 8 * DEPTH points.  Unrolled over the rows when there are few of them: a rolled loop indexes rs[] / re[] with
    // its counter, i.e. a chain of selects per iteration (~10 vector instructions x 4 rows in every wave of the batch kernel:
    // 121.5 -> 117 us)
    auto long_row = [&](uint32_t a, uint32_t b) {
        for (uint32_t p = a + kCoop * DEPTH + sub; p < b; p += kCoop) {
            const float4 Pp = ld_at<NARROW>(pts, p);
            float dx = Pp.x - qxf, dy = Pp.y - qyf, dz = Pp.z - qzf;
            if constexpr (kUnpacked) asm("" : "+v"(dx), "+v"(dy), "+v"(dz));
            const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const bool lt = d < m1;
            m2 = __builtin_amdgcn_fmed3f(m1, m2, d);
            p1 = lt ? p : p1;
            m1 = fminf(m1, d);
        }
    };
    if constexpr (TAIL) {
        float dx = PT.x - qxf, dy = PT.y - qyf, dz = PT.z - qzf;
        if constexpr (kUnpacked) asm("" : "+v"(dx), "+v"(dy), "+v"(dz));
        float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        d = tail_on ? d : __builtin_huge_valf();
        const bool lt = d < m1;
        m2 = __builtin_amdgcn_fmed3f(m1, m2, d);
        p1 = lt ? tp : p1;
        m1 = fminf(m1, d);
        if (tail_loops) {                                         // rare: runs under the EXEC mask of the groups with T > 8 only
#pragma unroll
            for (int k = 0; k < NR; k++) long_row(rs[k], re[k]);
        }
    } else if constexpr (NR <= 4) {
#pragma unroll
        for (int k = 0; k < NR; k++) long_row(rs[k], re[k]);
    } else {
#pragma unroll 1
        for (int k = 0; k < NR; k++) long_row(rs[k], re[k]);
    }
    // fold (smallest, runner-up, position) over the 8 lanes: all 8 are active here (see swz_xor)
    auto fold = [&](auto off) {
        constexpr int kPat = swz_xor(decltype(off)::value);
        const float o1 = swz_f32<kPat>(m1), o2 = swz_f32<kPat>(m2);
        const uint32_t op = swz_u32<kPat>(p1);
        const bool lt = o1 < m1;
        m2 = fminf(fminf(m2, o2), fmaxf(m1, o1));                // second smallest of the two sorted pairs
        p1 = lt ? op : p1;
        m1 = fminf(m1, o1);
    };
    fold(std::integral_constant<int, 1>{});
    fold(std::integral_constant<int, 2>{});
    fold(std::integral_constant<int, 4>{});
    bd = __builtin_huge_val();
    bi = kNoIndex;
    // m1 == +inf: the runs are empty, OR every fp32 distance overflowed (points farther than sqrt(FLT_MAX) = 1.8447e19 from the query:
    // far queries, clouds of huge extent).  Their fp64 distances are finite and must compete, so that case takes the exact scan too
    // (over empty runs it does nothing).
    if (m1 < __builtin_huge_valf() && m2 > m1 * (1.0f + 0x1p-19f) + 0x1p-90f) {   // unique within the fp32 error band: it is the exact winner
        const float4 W = ld_at<NARROW>(pts, p1);
        bd = dist2((double)W.x, (double)W.y, (double)W.z, qx, qy, qz);
        bi = __float_as_uint(W.w);
    } else {                                                      // near-ties / duplicates / overflow: exact (d2, index) order decides
#pragma unroll 1
        for (int k = 0; k < NR; k++) coop_scan_exact(pts, rs[k], re[k], sub, qx, qy, qz, bd, bi);
        coop_argmin8(bd, bi);
    }
}

// ---- the dense batch search: stage 0, then a WAVE-cooperative fallback -------------------------------------------------------
// Stage 0 decides ~99 % of the queries at 6 points per cell, but a wave holds 8 queries and used to run the 3x3x3 cube for all of
// them -- 8 lanes per query, the 9 rows of ~18 points taken 8 at a time -- as soon as ONE was undecided: 0.99^8 = 8 % of the waves,
// 15 % of the kernel's time (18 of 124 us on the 10 M-point cloud).  Here the whole wave turns to each undecided query in turn:
// 9 lanes fetch the bounds of what the block leaves of the cube's rows within reach of stage 0's best distance, every lane takes one
// point of each such row (all loads in flight), one ballot of the records that can beat or tie that best, and only those are compared
// exactly (wave_remainder_search).  The queries that even the cube does not decide (~1e-4) finish with the 8-lane shell walk as before.

// The 2x2x2 block of cells stage 0 scans for a query: its own cell (cx, cy, cz), its fractional position f in that cell (outside [0, 1) only
// where the cell coordinate was clamped: a query outside the grid) and, per axis, the neighbour on the side of f < 0.5, clamped to the grid.
// ONE function for the place where the runs are located and for the exact termination test, which must use the bounds of the block that
// was scanned: both calls are the same fp32 expressions of (G, q) in the same order (no contraction: -ffp-contract=off), so they agree to
// the bit -- on the half-cell planes too (tests/test_gpu_stage0_accept.py, case a).
struct Stage0Block { int cx, cy, cz; float fx, fy, fz; int xa, xb, ya, yb, za, zb; };
__device__ __forceinline__ void stage0_block(const GridDesc &G, float qxf, float qyf, float qzf, Stage0Block &B)
{
    query_cell(G, qxf, qyf, qzf, B.cx, B.cy, B.cz);
    B.fx = (qxf - G.ox) * G.inv_h - (float)B.cx; B.fy = (qyf - G.oy) * G.inv_h - (float)B.cy; B.fz = (qzf - G.oz) * G.inv_h - (float)B.cz;
    B.xa = max(B.fx < 0.5f ? B.cx - 1 : B.cx, 0); B.xb = min(B.fx < 0.5f ? B.cx : B.cx + 1, G.gx - 1);
    B.ya = max(B.fy < 0.5f ? B.cy - 1 : B.cy, 0); B.yb = min(B.fy < 0.5f ? B.cy : B.cy + 1, G.gy - 1);
    B.za = max(B.fz < 0.5f ? B.cz - 1 : B.cz, 0); B.zb = min(B.fz < 0.5f ? B.cz : B.cz + 1, G.gz - 1);
}

// Stage 0's termination test has two parts.
//
// The quick accept (stage0_accept_threshold, every query): the distance bc, in cell units, from the query to the nearest face of its block,
// shortened by 1/64 cell and taken 1e-6 short, as an fp32 length b; the query is decided when its best distance is within b.  The margin
// is far more than the fp32 rounding of f (< 2e-4 cells for coordinates of at most ~1024 cells, hence the |f| < 2 guard: only queries
// inside the grid or next to it) plus the exact test's own 1/256 slack, so whatever passes here passes the exact test too.
//
// bc comes from f alone: min over the axes of max(f, 1 - f).  The block is the two cells on the query's side, chosen by f < 0.5, so along
// an axis its faces are f + 1 and 1 - f away (low side) or f and 2 - f (high side): the nearer one is max(f, 1 - f) in either case, and
// for f in [0, 1) the fp32 values are the ones the face-by-face form computed (f + 1.0f >= 1.0f - f, 2.0f - f >= f).  Where the cell
// coordinate was clamped the same expression holds: f < 0 (cell 0, low side, the block starts at the grid's edge) leaves the face 1 - f
// away as the only one with cells behind it, f >= 1 (last cell, high side) the face f away.  A face WITHOUT cells behind it -- the block
// touches the grid's border on that side, or the grid has one or two cells along the axis -- does not bound the search at all, and the
// exact test leaves it out; counting it here only makes bc smaller.  So
//     bc <= the minimum over the faces that have cells behind them  (the form this replaced: six face distances from the block's bounds),
// the accept bd <= ((bc - 1/64) h 0.999999)^2 is monotone in bc, and: accepted here  =>  accepted by the face-by-face form  =>  accepted
// by the exact test.  (Where no face has cells behind it the face-by-face form declined and the exact test accepted everything: "the
// block covers the whole grid".)  A NaN f drops out of the minimum as it dropped out of the face-by-face one; all three NaN give b = NaN
// and no accept.  What is not accepted here takes the exact test, as the ~2 % of queries in the 1/64-cell band always did: results cannot
// change (tests/test_stage0_accept_model.py checks the chain of inclusions in the kernel's arithmetic).
// It needs no cell index and no block bound and is computed BEFORE the record loads: one register (b) crosses the screening where the
// six bounds (packed into two), the three f and the three cell coordinates did.
__device__ __forceinline__ float stage0_accept_threshold(const GridDesc &G, float fx, float fy, float fz)
{
    const float bc = fminf(fminf(fmaxf(fx, 1.0f - fx), fmaxf(fy, 1.0f - fy)), fmaxf(fz, 1.0f - fz));
    return fmaxf(fmaxf(fabsf(fx), fabsf(fy)), fabsf(fz)) < 2.0f ? (bc - 0.015625f) * (float)G.hd * 0.999999f : 0.0f;
}

// The exact test on the bound of the block that was scanned (box_bound): decided when the block covers the whole grid (+inf) or the best
// distance is within the bound.
__device__ __forceinline__ bool block_undecided(double bound, double bd)
{
    return bound != __builtin_huge_val() && !(bound > 0.0 && bd <= bound * bound);
}

// The exact test (rare: the 1/64-cell band, the undecided queries, queries outside the grid): is the query still undecided after its
// block gave best distance bd?  The block's bounds are recomputed from the query (stage0_block) instead of being carried across the
// screening.
__device__ __forceinline__ bool block_leaves_undecided(const GridDesc &G, float qxf, float qyf, float qzf, double qx, double qy, double qz, double bd)
{
    // (the query is made opaque first: the compiler would otherwise reuse the values of coop_stage0's own call, i.e. carry them across the
    // screening after all; the copies cost nothing where they stand, inside the rare branch)
    Stage0Block B;
    asm volatile("" : "+v"(qxf), "+v"(qyf), "+v"(qzf));
    stage0_block(G, qxf, qyf, qzf, B);
    return block_undecided(box_bound(G, B.xa, B.xb, B.ya, B.yb, B.za, B.zb, qx, qy, qz), bd);
}

// stage 0: the 2x2x2 block of cells on the query's side of its own cell = 4 x-runs; returns true when the query is still undecided
template <bool COUNT, bool NARROW>
__device__ __forceinline__ bool coop_stage0(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                            float qxf, float qyf, float qzf, uint32_t sub, double &bd, uint32_t &bi, uint32_t &npts,
                                            uint32_t &nruns)
{
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    Stage0Block B;
    stage0_block(G, qxf, qyf, qzf, B);
    // The threshold is pinned here, opaque to the compiler, which otherwise sinks its arithmetic behind the screening and keeps f and the
    // cell coordinates in registers across the record loads for it (six registers at the kernel's peak instead of one).
    float b = stage0_accept_threshold(G, B.fx, B.fy, B.fz);
    asm volatile("" : "+v"(b));
    uint32_t rs[4], re[4];
    if (G.blocks) {                                               // the corner's entry of the block table: one line, every lane reads it itself
        const uint32_t u = (uint32_t)(B.fx < 0.5f ? B.cx : B.cx + 1), v = (uint32_t)(B.fy < 0.5f ? B.cy : B.cy + 1), w = (uint32_t)(B.fz < 0.5f ? B.cz : B.cz + 1);
        const uint4 *ent = G.blocks + 2u * ((w * ((uint32_t)G.gy + 1u) + v) * ((uint32_t)G.gx + 1u) + u);
        const uint4 S = ent[0], E = ent[1];
        rs[0] = S.x; rs[1] = S.y; rs[2] = S.z; rs[3] = S.w;
        re[0] = E.x; re[1] = E.y; re[2] = E.z; re[3] = E.w;
        if (COUNT && sub < 4) {
            const int ri = (int)sub;
            const bool ok = !((ri >> 1) && B.zb == B.za) && !((ri & 1) && B.yb == B.ya);
            npts += re[ri] - rs[ri]; nruns += ok ? 1u : 0u;
        }
    } else {
        // One load instruction for the eight run bounds: lane k < 4 of the group fetches run k's start, lane 4 + k its end -- the start's
        // own address where the row is disabled (it coincides with another at the grid's border), which makes the run empty.
        const int ri = (int)sub & 3;
        const bool ok = !((ri >> 1) && B.zb == B.za) && !((ri & 1) && B.yb == B.ya);
        const uint32_t row = cell_lin(G, 0, (ri & 1) ? B.yb : B.ya, (ri >> 1) ? B.zb : B.za);
        const uint32_t mine = ld_at<NARROW>(cell_start, row + ((sub & 4u) && ok ? (uint32_t)B.xb + 1u : (uint32_t)B.xa));
        // broadcasts with an immediate pattern, all 8 lanes active (see swz_xor)
        rs[0] = swz_u32<swz_group_lane(0)>(mine); re[0] = swz_u32<swz_group_lane(4)>(mine);
        rs[1] = swz_u32<swz_group_lane(1)>(mine); re[1] = swz_u32<swz_group_lane(5)>(mine);
        rs[2] = swz_u32<swz_group_lane(2)>(mine); re[2] = swz_u32<swz_group_lane(6)>(mine);
        rs[3] = swz_u32<swz_group_lane(3)>(mine); re[3] = swz_u32<swz_group_lane(7)>(mine);
        if (COUNT) {
            const uint32_t my_e = swz_u32<swz_xor(4)>(mine);      // lane k < 4: its run's end, from lane 4 + k
            if (sub < 4) { npts += my_e - mine; nruns += ok ? 1u : 0u; }
        }
    }
    coop_screen_rows<4, 2, true, NARROW>(pts, rs, re, sub, qxf, qyf, qzf, qx, qy, qz, bd, bi);
    if (b > 0.0f && bd <= (double)b * (double)b) return false;    // the quick accept
    return block_leaves_undecided(G, qxf, qyf, qzf, qx, qy, qz, bd);
}

// What the 2x2x2 block B of a WAVE-UNIFORM query leaves of the 3x3x3 cube around the query's cell, searched by all 64 lanes from stage 0's
// result: on entry (bd, bi) is the exact winner by (d2, index) among the block's records ((+inf, none) for an empty block), on return the
// exact winner among the records of the whole cube.  (It replaces a search that took the undecided query as if nothing were known about
// it: all nine rows of the cube, the block's eight cells among them, (min, runner-up, position) per lane, a 6-step fold of three
// ds_bpermute each, the winner's reload -- three dependent trips where stage 0's point most often still was the answer.)
//
// Lanes 0..8 own the nine (y, z) rows of the cube.  Each finds the x-cells of its row that are inside the grid, not in B, and within reach
// of the ball of radius sqrt(bd) around the query: the cell's box -- widened per axis by the h/256 slack of cube_bound, which covers the
// fp32 cell assignment, and open towards the outside at the grid's border, where the assignment clamps -- is at most sqrt(bd) away.  The
// gaps come from the query's real coordinates (fp64, the face positions as cube_bound computes them), so queries outside the grid work;
// the sum of their squares is taken 2^-40 short, which covers its own rounding: for a query within 2^36 cells of the grid a gap is off by
// < 2^-13 h, far inside the slack (the assignment needs 4e-4 h of the h/256), for a query farther away by < 2^-49 of itself.  A comparison
// that is not decided (NaN, bd = +inf) counts as within reach.  The cells within reach are contiguous: a row of B has at most one cube
// cell left, at one end; a row outside B meets the ball in an interval around the query's own x-cell, whose gap is 0.  (Were they not, the
// range taken from the first to the last would only scan more.)  A lane with an empty range fetches nothing.
//
// Screening is one-sided against the known best: a record is a candidate iff d32 <= thr, thr = (float)bd rounded up, times (1 + 2^-19),
// plus 2^-90 -- the band proved at the head of the brute-force filter above (nn_tile_candidates_kernel's form): a record with exact
// d2 <= bd has d32 <= d2 (1 + 4e-7) + 2^-120 <= thr.  Inclusive, because an equal distance with a lower index must win.  bd beyond
// FLT_MAX gives thr = +inf and every record is a candidate: far queries, whose fp32 distances overflow while the fp64 ones are finite and
// must compete.  No candidate anywhere (the common case): (bd, bi) stands after two trips, bounds and records.  Otherwise the lanes that
// hold candidates evaluate them in exact fp64 from the record registers they still hold, under better() against (bd, bi), and one
// wave_argmin gives every lane the result.
//
// The rows with records are taken kRemRows = 4 at a time (a ball that passes one face of the block has 2 or 4 rows in reach: one pass):
// the kernel's VGPR count is the maximum over all its paths, and the exact comparison with the records of all nine rows still held costs
// 72 VGPRs and scratch where the kernel has 69 and none (profiles/r06_fallback_asm.txt).
//
// Why this is exact.  Let S be the cells scanned.  Every record of S with exact d2 <= bd lies inside the band and is compared exactly, so
// on return (bd, bi) is the (d2, index)-minimum over B and S.  Every record of the cube outside B and S lies in a cell whose widened box
// is strictly farther than sqrt(bd_in) >= sqrt(bd_out): it is neither better nor a tie.  So the cube is fully accounted for, and the
// termination test and the shell walk (coop_finish_shells) stand on the same ground as after a scan of all its 27 cells.
constexpr int kRemRows = 4;
template <bool COUNT>
__device__ __forceinline__ void wave_remainder_search(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                      float qxf, float qyf, float qzf, double &bd, uint32_t &bi, uint32_t &npts, uint32_t &nruns)
{
    const uint32_t lane = threadIdx.x & 63;
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    Stage0Block B;                                                    // the block, as coop_stage0 chose it
    stage0_block(G, qxf, qyf, qzf, B);
    const int cx = B.cx, cy = B.cy, cz = B.cz;
    // distance along one axis from q to cell c of g (0 inside), a face counting only where the grid has cells behind it, minus the slack
    auto gap = [&](int c, int g, double o, double q) {
        const double ninf = -__builtin_huge_val();
        const double below = c > 0 ? (o + (double)c * G.hd) - q : ninf;
        const double above = c < g - 1 ? q - (o + (double)(c + 1) * G.hd) : ninf;
        return fmax(fmax(below, above) - G.hd * (1.0 / 256.0), 0.0);
    };
    uint32_t my_s = 0, my_e = 0;                                      // lanes 9.. and lanes with nothing in reach: the empty run
    {
        const int l = lane < 9 ? (int)lane : 0;
        const int zz = cz + l / 3 - 1, yy = cy + l % 3 - 1;
        const bool ok = lane < 9 && zz >= 0 && zz < G.gz && yy >= 0 && yy < G.gy;
        const bool block_row = yy >= B.ya && yy <= B.yb && zz >= B.za && zz <= B.zb;
        const double gy = gap(yy, G.gy, G.oyd, qy), gz = gap(zz, G.gz, G.ozd, qz);
        auto reach = [&](int c) {
            const bool valid = ok && c >= 0 && c <= G.gx - 1 && !(block_row && c >= B.xa && c <= B.xb);
            const double gxx = gap(c, G.gx, G.oxd, qx);
            return valid & !(((gxx * gxx + gy * gy) + gz * gz) * (1.0 - 0x1p-40) > bd);
        };
        const bool rm = reach(cx - 1), r0 = reach(cx), rp = reach(cx + 1);
        if (rm || r0 || rp) {
            const int lo = rm ? cx - 1 : (r0 ? cx : cx + 1), hi = rp ? cx + 1 : (r0 ? cx : cx - 1);
            const uint32_t row = cell_lin(G, 0, yy, zz);
            my_s = cell_start[row + (uint32_t)lo];
            my_e = cell_start[row + (uint32_t)hi + 1u];
            if (COUNT) { npts += my_e - my_s; nruns += 1u; }
        }
    }
    float thr = (float)bd;
    if ((double)thr < bd) thr = __uint_as_float(__float_as_uint(thr) + 1u);   // rounded up (bd >= 0; FLT_MAX steps to +inf)
    thr = thr * (1.0f + 0x1p-19f) + 0x1p-90f;
    double ld = bd;
    uint32_t li = bi;
    // The exact comparison widens the query where it is used, from scalar registers the compiler cannot see through: kept as three fp64
    // values across the screening they are six more vector registers next to the records in flight, and the kernel's count is the
    // maximum over all its paths (see nn_grid_coop_kernel).
    auto exact = [&](const float4 &R) {
        float sx = qxf, sy = qyf, sz = qzf;
        asm volatile("" : "+s"(sx), "+s"(sy), "+s"(sz));
        const double d2 = dist2((double)R.x, (double)R.y, (double)R.z, (double)sx, (double)sy, (double)sz);
        const uint32_t id = __float_as_uint(R.w);
        if (better(d2, id, ld, li)) { ld = d2; li = id; }
    };
    bool any = false;                                                 // (wave-uniform) some lane met a candidate
    unsigned long long rows = __builtin_amdgcn_ballot_w64(my_e > my_s);   // the rows with records: bits 0..8
    while (rows) {                                                    // wave-uniform: kRemRows rows at a time, their loads all issued before the first is consumed
        uint32_t rs[kRemRows], len[kRemRows];                         // run bounds in scalar registers; rows without records cost nothing
#pragma unroll
        for (int j = 0; j < kRemRows; j++) {
            rs[j] = 0; len[j] = 0;
            if (rows) {
                const int k = __builtin_ctzll(rows);
                rows &= rows - 1;
                rs[j] = (uint32_t)__builtin_amdgcn_readlane((int)my_s, k);
                len[j] = (uint32_t)__builtin_amdgcn_readlane((int)my_e, k) - rs[j];
            }
        }
        float4 P[kRemRows];
#pragma unroll
        for (int j = 0; j < kRemRows; j++)
            if (len[j]) P[j] = pts[rs[j] + min(lane, len[j] - 1u)];   // lane beyond the row: the row's last record, masked below
        uint32_t cm = 0;                                              // bit j: the lane's record of row j is a candidate; bit kRemRows: a long row had one
#pragma unroll
        for (int j = 0; j < kRemRows; j++)
            if (len[j]) {
                const float dx = P[j].x - qxf, dy = P[j].y - qyf, dz = P[j].z - qzf;
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                cm |= (uint32_t)((lane < len[j]) & (d <= thr)) << j;
            }
#pragma unroll
        for (int j = 0; j < kRemRows; j++)
            if (len[j] > 64u)                                         // rows of more than 64 records
                for (uint32_t o = 64u + lane; o < len[j]; o += 64u) {
                    const float4 R = pts[rs[j] + o];
                    const float dx = R.x - qxf, dy = R.y - qyf, dz = R.z - qzf;
                    const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    if (d <= thr) { exact(R); cm |= 1u << kRemRows; }
                }
        if (__builtin_amdgcn_ballot_w64(cm != 0u)) {                  // (wave-uniform) rare: stage 0's point most often stands
            any = true;
#pragma unroll
            for (int j = 0; j < kRemRows; j++)
                if ((cm >> j) & 1u) exact(P[j]);                      // (set for rows with records only)
        }
    }
    if (any) {
        wave_argmin(ld, li);
        bd = ld;
        bi = li;
    }
}

// after the cube: shells of growing radius until the termination bound holds (8 lanes per query, rare on dense clouds)
template <bool COUNT>
__device__ __forceinline__ void coop_finish_shells(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                   float qxf, float qyf, float qzf, uint32_t sub, double &bd, uint32_t &bi, uint32_t &npts,
                                                   uint32_t &nruns)
{
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    int cx, cy, cz;
    query_cell(G, qxf, qyf, qzf, cx, cy, cz);
    for (int r = 1;; r++) {
        if (r > 1) {
            coop_scan_shell<COUNT>(G, pts, cell_start, cx, cy, cz, r, sub, qx, qy, qz, bd, bi, npts, nruns);
            coop_argmin8(bd, bi);
        }
        const double bound = cube_bound(G, cx, cy, cz, r, qx, qy, qz);
        if (bound == __builtin_huge_val() || (bound > 0.0 && bd <= bound * bound)) break;
    }
}

// One query per group of 8 lanes, every lane of the wave in step (live = the group has a query): stage 0, then the whole wave on what each
// undecided query's block leaves of its cube, in turn, then the 8-lane shell walk for what even the cube leaves open.  Every lane of a group returns its
// query's exact (bd, bi).
template <bool COUNT, bool NARROW>
__device__ __forceinline__ void coop_wave_search(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start, bool live,
                                                 float qxf, float qyf, float qzf, uint32_t sub, double &bd, uint32_t &bi, uint32_t &npts, uint32_t &nruns)
{
    bd = __builtin_huge_val();
    bi = kNoIndex;
    bool undecided = false;
    if (live) undecided = coop_stage0<COUNT, NARROW>(G, pts, cell_start, qxf, qyf, qzf, sub, bd, bi, npts, nruns);
    unsigned long long todo = __builtin_amdgcn_ballot_w64(undecided && sub == 0);
    while (todo) {                                    // wave-uniform: one undecided query at a time, all 64 lanes on it
        const int g = __builtin_ctzll(todo);
        todo &= todo - 1;
        const float bx = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(qxf), g)),
                    by = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(qyf), g)),
                    bz = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(qzf), g));
        double cbd = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bd), g), __builtin_amdgcn_readlane(__double2loint(bd), g));   // stage 0's exact best
        uint32_t cbi = (uint32_t)__builtin_amdgcn_readlane((int)bi, g);
        wave_remainder_search<COUNT>(G, pts, cell_start, bx, by, bz, cbd, cbi, npts, nruns);
        if (((threadIdx.x & 63) >> 3) == (uint32_t)(g >> 3)) { bd = cbd; bi = cbi; }
    }
    if (live && undecided) coop_finish_shells<COUNT>(G, pts, cell_start, qxf, qyf, qzf, sub, bd, bi, npts, nruns);
}

// Occupancy target 7 waves per SIMD, as minimum AND maximum: with 8 allowed the scheduler keeps the kernel at 64 VGPRs by issuing the
// eight record loads of stage 0 two at a time (four dependent round trips); capped at 7 it takes 72 VGPRs and issues all eight before the
// first use.  Headline step 0.1198-0.1210 -> 0.1163-0.1179 ms (6 waves: 0.122, 5: 0.134; profiles/r03_ab_occupancy_cap.txt).  Raising
// only the minimum (round 2's "7 waves" experiment) never changed the code: the scheduler still aimed for 8.
// With the shared tail slot (coop_screen_rows<4, 2, true>) nine loads are in flight; whatever is added to stage 0 has to be checked against
// that ceiling in the compiler's resource remarks AND in the order of the loads in the ISA (profiles/r07_stage0_asm.txt): NARROW 68 VGPRs,
// all nine record loads before the first s_waitcnt vmcnt (vmcnt(8)), 270 vector instructions from the entry to the tail_loops branch, 20
// in the fold and 28 from there to the ballot of the undecided for a query the quick accept decides; wide 70 VGPRs, all nine loads before
// vmcnt(8) as well, 280 + 20 + 29.  (Before the quick accept moved in front of the loads and the run bounds into one load instruction:
// 69 VGPRs, 256 + 20 + 81, r05_stage0_asm.txt; before the swizzle folds, the wrapping clamp and the 32-bit offsets: 70 VGPRs, eight loads
// and the ninth behind vmcnt(7), 283 + 36.)
// With the screening unpacked (coop_screen_rows, kUnpacked) the narrow form is 261 vector instructions on that path and needs 64 VGPRs, so
// for the first time it builds for 8 waves without scratch and with the nine loads in one flight (the wide form splits them 8 + 1 there
// and keeps 7 unmeasured).  Run, the eighth wave does not pay: headline step 0.1165 ms at 8 waves against 0.1160 at 7 (parent, packed,
// 0.1183; five alternated rounds, profiles/r08_ab_unpacked_waves.txt) -- the kernel is bound by vector issue, and a wave more per SIMD
// only waits longer for it.  The target is a property of the instantiation (nn_coop_waves), 7 for every one of them.
// NARROW (chosen per launch on the host: narrow_offsets_fit, gridbuild.hpp) addresses the records, the run bounds, the sorted query and
// the two results with 32-bit byte offsets from their scalar bases (ld_at / st_at); only the TAIL instantiation of coop_screen_rows takes
// it -- the pyramid's stage 0 and the rare paths (exact rescans, the wave's remainder search, shells) keep 64-bit addresses.
// BLOCK (threads per block, chosen per cloud on the host: pct_cloud::nn_block): nothing in the kernel is shared between the waves of a
// block -- no LDS, no barrier -- so the block is only the unit in which the dispatcher hands out wave slots, and a block of four waves
// waits until a CU has four of its 28 slots free at once.  Blocks of kNNBlock = 128 threads (two waves, 16 queries) where the cloud's
// records fit the Infinity Cache: headline step (profiles/nn_persist_ab.txt) 256 threads 0.1210 ms, kernel 0.1017; 128 threads 0.1188 /
// 0.0994; 64 threads 0.1189 / 0.0992 -- below the 256-thread form in every one of five alternated rounds, 0.77 of the wave slots occupied
// instead of 0.68.  256 threads where they do not: on the 100 M-point cloud, whose batch waits on HBM, the smaller block ran 1 M queries at
// 0.2670 against 0.2652 ms and 8 M at 1.598 against 1.49-1.58.  The same kernel as resident blocks that walk the sorted batch in a loop
// (one launch block per set of wave slots) ran the headline step at 0.1659 ms: DESIGN.md, retired variants.
constexpr int kNNBlock = 128;
// waves per SIMD the instantiation is built for, as minimum and maximum (see above; 8 needs <= 64 VGPRs, no scratch and the nine loads in
// one flight, which only <false, true, .> has, and which measured slower there)
template <bool COUNT, bool NARROW, int BLOCK>
constexpr int nn_coop_waves() { return 7; }
template <bool COUNT, bool NARROW, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(nn_coop_waves<COUNT, NARROW, BLOCK>(), nn_coop_waves<COUNT, NARROW, BLOCK>()))) void nn_grid_coop_kernel(GridDesc G, const float4 *__restrict__ pts,
                                                           const uint32_t *__restrict__ cell_start,
                                                           const float *__restrict__ q, uint32_t Q, uint32_t index_base,
                                                           const float4 *__restrict__ qsorted,
                                                           uint32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                           WorkCounters *__restrict__ work)
{
    const uint32_t sub = threadIdx.x & (kCoop - 1);
    const uint32_t slot = coop_slot<BLOCK / kCoop>(qsorted);
    uint32_t npts = 0, nruns = 0;
    const bool live = slot < Q;                       // every lane of the wave stays in step: the fallback is wave-cooperative (see above)
    uint32_t t = slot;
    float qxf = 0.0f, qyf = 0.0f, qzf = 0.0f;
    if (live) t = coop_fetch_query<NARROW>(qsorted, q, slot, qxf, qyf, qzf);
    double bd;
    uint32_t bi;
    coop_wave_search<COUNT, NARROW>(G, pts, cell_start, live, qxf, qyf, qzf, sub, bd, bi, npts, nruns);
    if (live && sub == 0) {
        st_at<NARROW>(out_idx, t, reported_index(bd, bi, index_base));
        st_at<NARROW>(out_d2, t, bd);
    }
    if (COUNT) commit_work(work, npts, nruns);
}

// The cells [x0, x1] x [y0, y1] x [z0, z1] that can hold a point within r of the query: the box every kernel that walks a ball's rows
// uses (the radius count, and the radius search's fill, which must meet exactly the rows the count reserved space for).
// r enters only squared (kdtree.c:273).  The box edges q -/+ pad are fp32 sums: each is off by up to 2^-24 (|q| + pad), and the
// fp64 test itself admits points up to r (1 + 2^-50) away, so the pad carries 2^-22 (|q| + |r|) per axis on top of h/100 --
// nothing at ordinary magnitudes, everything for a query 1e18 away whose ball reaches back to the cloud.  An edge that comes
// out NaN (inf - inf: infinite query or radius) opens the box to that side (cell_coord sends NaN to cell 0: right for the
// lower edge only).  The box is filled through a reference: returned by value, the compiler computes the lower edges behind the
// upper edges' branches, which reschedules count_grid_coop_kernel's prologue.
struct BallBox { int x0, x1, y0, y1, z0, z1; };

__device__ __forceinline__ void grid_ball_box(const GridDesc &G, float qxf, float qyf, float qzf, float rf, BallBox &B)
{
    const float pad0 = fabsf(rf) + 0.01f * (1.0f / G.inv_h);
    const float padx = pad0 + 0x1p-22f * (fabsf(qxf) + fabsf(rf)), pady = pad0 + 0x1p-22f * (fabsf(qyf) + fabsf(rf)),
                padz = pad0 + 0x1p-22f * (fabsf(qzf) + fabsf(rf));
    const float hx = qxf + padx, hy = qyf + pady, hz = qzf + padz;
    B.x0 = cell_coord(qxf - padx, G.ox, G.inv_h, G.gx); B.x1 = hx == hx ? cell_coord(hx, G.ox, G.inv_h, G.gx) : G.gx - 1;
    B.y0 = cell_coord(qyf - pady, G.oy, G.inv_h, G.gy); B.y1 = hy == hy ? cell_coord(hy, G.oy, G.inv_h, G.gy) : G.gy - 1;
    B.z0 = cell_coord(qzf - padz, G.oz, G.inv_h, G.gz); B.z1 = hz == hz ? cell_coord(hz, G.oz, G.inv_h, G.gz) : G.gz - 1;
}

// Cooperative radius count: 8 lanes per query, the rows of the ball's bounding box: the run bounds of up to 16 rows fetched at once
// (two per lane), then the rows two at a time, every lane with four 16-byte loads per row in flight (32 points per row for the group)
// before the first compare; longer rows finish in a tail loop.  Every distance is the exact fp64 one (kdtree.c:273,
// d2 <= r*r inclusive).  The box is [q - r - pad, q + r + pad] with pad = h/100: a point within r of q can only sit in a
// cell of that range, because the fp32 cell assignment errs by < 4e-4 cells (same argument as cube_bound's h/256 slack).
template <bool COUNT>
__global__ __launch_bounds__(256) void count_grid_coop_kernel(GridDesc G, const float4 *__restrict__ pts,
                                                              const uint32_t *__restrict__ cell_start,
                                                              const float *__restrict__ q, const float *__restrict__ rad, uint32_t Q,
                                                              const float4 *__restrict__ qsorted, uint32_t *__restrict__ count,
                                                              WorkCounters *__restrict__ work)
{
    const uint32_t sub = threadIdx.x & (kCoop - 1);
    const uint32_t slot = coop_slot<256 / kCoop>(qsorted);
    uint32_t npts = 0, nruns = 0;
    if (slot < Q) {                                   // uniform within a group of 8 lanes
        float qxf, qyf, qzf;
        const uint32_t t = coop_fetch_query(qsorted, q, slot, qxf, qyf, qzf);
        const float rf = rad[t];
        const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
        const double r2 = (double)rf * (double)rf;
        BallBox B;
        grid_ball_box(G, qxf, qyf, qzf, rf, B);
        const int x0 = B.x0, x1 = B.x1, y0 = B.y0, z0 = B.z0;
        const int ny = B.y1 - y0 + 1, nrows = ny * (B.z1 - z0 + 1);
        uint32_t c = 0;
        // Rows of the box: the run bounds of up to 16 rows in ONE trip (two per lane), then the rows two at a time with 32 points of each
        // in flight (a row of 3-4 cells holds ~20): a query's 9-16 rows cost 1 + rows/2 dependent round trips.  (The first form took the
        // rows four at a time with 16 points each and finished every row in a tail loop, one trip per row: ~18 trips; 1 M counts of r = 1 on
        // the 10 M-point cloud 0.51 -> 0.43 ms, profiles/r03_ab_count_rows.txt.)
        for (int base = 0; base < nrows; base += 16) {
            uint32_t bs[2], be[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int k = base + 8 * h + (int)sub;
                const bool ok = k < nrows;
                row_run(G, cell_start, ok, y0 + k % ny, z0 + k / ny, x0, x1, bs[h], be[h]);
                if (COUNT) { npts += be[h] - bs[h]; nruns += ok ? 1u : 0u; }
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {                         // rows base + 2 i, base + 2 i + 1
                if (base + 2 * i >= nrows) break;                 // uniform within the group of 8 lanes
                uint32_t rs[2], re[2];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int r = 2 * i + j;                      // compile-time: which register, which lane
                    rs[j] = (uint32_t)__shfl((int)bs[r >> 3], r & 7, kCoop);
                    re[j] = (uint32_t)__shfl((int)be[r >> 3], r & 7, kCoop);
                }
                float4 P[2][4];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint32_t last = re[j] > rs[j] ? re[j] - 1 : 0u;
#pragma unroll
                    for (int d = 0; d < 4; d++) P[j][d] = pts[min(rs[j] + sub + kCoop * d, last)];
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const bool in = rs[j] + sub + kCoop * d < re[j];
                        c += (in && dist2((double)P[j][d].x, (double)P[j][d].y, (double)P[j][d].z, qx, qy, qz) <= r2) ? 1u : 0u;
                    }
                }
#pragma unroll 1
                for (int j = 0; j < 2; j++)
                    for (uint32_t p = rs[j] + 4 * kCoop + sub; p < re[j]; p += kCoop) {
                        const float4 Pp = pts[p];
                        c += dist2((double)Pp.x, (double)Pp.y, (double)Pp.z, qx, qy, qz) <= r2 ? 1u : 0u;
                    }
            }
        }
#pragma unroll
        for (int off = 1; off < kCoop; off <<= 1) c += (uint32_t)__shfl_xor((int)c, off, kWave);
        if (sub == 0) count[t] = c;
    }
    if (COUNT) commit_work(work, npts, nruns);
}

// =====================================================================================
// 4b. Low-latency ("express") kernels: ONE launch per call, query passed by value or read from
//     host-mapped memory, results written straight to host-mapped memory.  The planner's RRT*
//     loop issues single queries in sequence (corridor_finder.cpp:719-756); there the cost is
//     launch + copy latency, not throughput.
// =====================================================================================
struct ExpressOut { double d2; double radius; uint32_t idx; uint32_t count; };

// Completion word of an express launch.  hipStreamSynchronize costs ~20 us of host time however short the kernel
// (profiles/r01_corridor_rocprof_summary.txt); here the kernel itself tells the host it is done: the thread that wrote a block's
// results fences them to system scope and takes a ticket, the block holding the last ticket stores `value` (release, system
// scope) into a word of host-mapped memory the host spins on.  seq == nullptr: no signalling (the caller synchronises).
struct ExpressSignal { uint32_t *counter; uint32_t *seq; uint32_t value; };

// called by the ONE thread that stored the block's host-visible results, after the stores
__device__ __forceinline__ void express_done(const ExpressSignal &S)
{
    if (!S.seq) return;
    __threadfence_system();
    bool last = gridDim.x == 1;
    if (!last) {
        last = atomicAdd(S.counter, 1u) == gridDim.x - 1;
        if (last) { atomicExch(S.counter, 0u); __threadfence_system(); }
    }
    if (last) __hip_atomic_store(S.seq, S.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the same for kernels in which every thread stores host-visible data: all fence, the block meets, thread 0 signals
__device__ __forceinline__ void express_done_block(const ExpressSignal &S)
{
    if (!S.seq) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) express_done(S);
}

// Results of a host-buffer batch leave the card by this kernel instead of two DMA copies + a stream synchronise: it stores
// (index, d2) -- or counts -- into host-mapped memory, every storing thread fences at system scope, and the last block releases the
// sequence word the host spins on (express_done_block).  A 4096-query batch saves ~80 us of copy setup + synchronise this way.
// ... and the queries enter the same way: one pass over the host-mapped staging buffer into device memory (the batch's kernels
// read their queries many times; only this copy crosses the bus)
__global__ __launch_bounds__(256) void import_floats_kernel(const float *__restrict__ h_src, uint32_t n, float *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = h_src[i];
}

__global__ __launch_bounds__(256) void export_results_kernel(const uint32_t *__restrict__ idx, const double *__restrict__ d2, uint32_t Q,
                                                             uint32_t *__restrict__ h_idx, double *__restrict__ h_d2, ExpressSignal sig)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) {
        h_idx[i] = idx[i];
        if (d2) h_d2[i] = d2[i];
    }
    express_done_block(sig);
}

// one block, exact fp64 brute force over a small cloud (the RRT* node set of the kd_* drop-in).  Besides the winner (lowest index
// among the minima) it reports HOW MANY points attain the minimum (out->count): the kd_* drop-in resolves an exact tie the way
// the reference's tree walk does (kdtree_gpu.cpp reference_tie_winner) and only then needs the tied set.
__device__ __forceinline__ void tie_merge(double &d, uint32_t &i, uint32_t &c, double od, uint32_t oi, uint32_t oc)
{
    if (od < d) { d = od; i = oi; c = oc; }
    else if (od == d) { c += oc; i = min(i, oi); }
}

__global__ __launch_bounds__(1024) void nn_small_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ z, uint32_t n, double qx, double qy, double qz,
                                                        uint32_t index_base, ExpressOut *__restrict__ out, ExpressSignal sig)
{
    double bd = __builtin_huge_val();
    uint32_t bi = kNoIndex, bc = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const double d2 = dist2((double)x[i], (double)y[i], (double)z[i], qx, qy, qz);
        if (d2 < bd) { bd = d2; bi = i; bc = 1; }
        else if (d2 == bd) bc++;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd, off, kWave);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off, kWave), oc = (uint32_t)__shfl_xor((int)bc, off, kWave);
        tie_merge(bd, bi, bc, od, oi, oc);
    }
    __shared__ double s_d[16];
    __shared__ uint32_t s_i[16], s_c[16];
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = bd; s_i[threadIdx.x >> 6] = bi; s_c[threadIdx.x >> 6] = bc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) tie_merge(bd, bi, bc, s_d[w], s_i[w], s_c[w]);
        out->d2 = bd;
        out->idx = reported_index(bd, bi, index_base);
        out->count = bc;
        express_done(sig);
    }
}

// one block: ids of all points with d2 <= r2 (arrival order; the host sorts), count in out->count
__global__ __launch_bounds__(1024) void radius_small_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, uint32_t n, double qx, double qy, double qz,
                                                            double r2, uint32_t index_base, uint32_t *__restrict__ ids, uint32_t cap,
                                                            ExpressOut *__restrict__ out, ExpressSignal sig)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024)
        if (dist2((double)x[i], (double)y[i], (double)z[i], qx, qy, qz) <= r2) {
            const uint32_t pos = atomicAdd(&s_n, 1u);
            if (pos < cap) ids[pos] = i + index_base;
        }
    __syncthreads();
    if (threadIdx.x == 0) out->count = s_n;
    express_done_block(sig);
}

// =====================================================================================
// 5. Planner arithmetic around the NN: sphere inflation and the sampled Bezier check
// =====================================================================================
// batched forms for speculative RRT* expansion: one 256-thread block per query over a small cloud
__global__ __launch_bounds__(256) void nn_small_batch_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                             const float *__restrict__ z, uint32_t n,
                                                             const double *__restrict__ q, uint32_t index_base,
                                                             ExpressOut *__restrict__ out, ExpressSignal sig)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    const double qx = q[3 * blockIdx.x], qy = q[3 * blockIdx.x + 1], qz = q[3 * blockIdx.x + 2];
    double bd = __builtin_huge_val();
    uint32_t bi = kNoIndex;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const double d2 = dist2((double)x[i], (double)y[i], (double)z[i], qx, qy, qz);
        if (d2 < bd) { bd = d2; bi = i; }
    }
    wave_argmin(bd, bi);
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = bd; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (better(s_d[w], s_i[w], bd, bi)) { bd = s_d[w]; bi = s_i[w]; }
        out[blockIdx.x].d2 = bd;
        out[blockIdx.x].idx = reported_index(bd, bi, index_base);
        express_done(sig);
    }
}

// ids[block * cap_per_query + k] = k-th hit (arrival order), out[block].count = number of hits (may exceed the cap)
__global__ __launch_bounds__(256) void radius_small_batch_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ z, uint32_t n,
                                                                 const double *__restrict__ q, const double *__restrict__ r,
                                                                 uint32_t index_base, uint32_t *__restrict__ ids,
                                                                 uint32_t cap_per_query, ExpressOut *__restrict__ out, ExpressSignal sig)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const double qx = q[3 * blockIdx.x], qy = q[3 * blockIdx.x + 1], qz = q[3 * blockIdx.x + 2];
    const double r2 = r[blockIdx.x] * r[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += 256)
        if (dist2((double)x[i], (double)y[i], (double)z[i], qx, qy, qz) <= r2) {
            const uint32_t pos = atomicAdd(&s_n, 1u);
            if (pos < cap_per_query) ids[(size_t)blockIdx.x * cap_per_query + pos] = i + index_base;
        }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x].count = s_n;
    express_done_block(sig);
}

// corridor_finder.cpp:113-126: early-out test in fp64 on the planner's Vector3d, then the
// query is narrowed to fp32 (searchPoint.x = search_Pt(0)).  skip[i] = 1 when the early-out fires.
__global__ __launch_bounds__(256) void inflate_prologue_kernel(InflateParams P, const double *__restrict__ pts,
                                                               uint32_t n, float *__restrict__ q,
                                                               unsigned char *__restrict__ skip)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    skip[i] = inflate_skips(P, px, py, pz) ? 1 : 0;
    q[3 * i] = (float)px;
    q[3 * i + 1] = (float)py;
    q[3 * i + 2] = (float)pz;
}

// corridor_finder.cpp:130-132: r = sqrt(d2) - search_margin, min(r, max_radius);
// early-out rows get max_radius - search_margin, idx = none, d2 = +inf.
__global__ __launch_bounds__(256) void inflate_epilogue_kernel(InflateParams P, uint32_t n,
                                                               const unsigned char *__restrict__ skip, int cloud_empty,
                                                               uint32_t *__restrict__ idx, double *__restrict__ d2,
                                                               double *__restrict__ radius)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (skip[i] || cloud_empty) {
        radius[i] = inflate_skipped_radius(P);
        idx[i] = kNoIndex;
        d2[i] = __builtin_huge_val();
        return;
    }
    radius[i] = inflate_radius(P, d2[i]);
}

// the same epilogue writing one {d2, radius, idx} record per point into host-mapped memory (small batches: the host reads the
// results after one stream sync instead of issuing three device-to-host copies)
__global__ __launch_bounds__(256) void inflate_epilogue_out_kernel(InflateParams P, uint32_t n, const unsigned char *__restrict__ skip,
                                                                   int cloud_empty, const uint32_t *__restrict__ idx,
                                                                   const double *__restrict__ d2, ExpressOut *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (skip[i] || cloud_empty) {
        out[i].radius = inflate_skipped_radius(P);
        out[i].idx = kNoIndex;
        out[i].d2 = __builtin_huge_val();
        return;
    }
    out[i].radius = inflate_radius(P, d2[i]);
    out[i].idx = idx[i];
    out[i].d2 = d2[i];
}

// Block-wide winner: every thread passes its (d2, index) and gets back the block's best.
__device__ __forceinline__ void block_argmin256(double &d, uint32_t &i, double *s_d, uint32_t *s_i)
{
    wave_argmin(d, i);
    __syncthreads();                                   // previous use of s_d / s_i is over
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = d; s_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    d = s_d[0]; i = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; w++)
        if (better(s_d[w], s_i[w], d, i)) { d = s_d[w]; i = s_i[w]; }
}

// Low-latency fused inflation: ONE 256-thread block per planner point (early-out test, narrowing, cell
// search, radius), arguments and results in host-mapped memory.  A single query has no batch to hide
// latency behind, so the parallelism goes across the ROWS of the cube / shell being searched: the 32
// groups of 8 lanes each take every 32nd row, and the block folds its candidates after each shell.
// stop_d2: when only the radius is wanted the search may stop once everything unseen is farther than
// max_radius + search_margin (the radius is then max_radius whatever lies beyond); +inf = exact NN.
// Same arithmetic and the same termination bound (cube_bound) as the batch kernel's shell walk.
// INFLATE = false: plain nearest neighbour of the (fp32-valued) points in qpts -- no early-out, no radius.
// The block-wide search itself: nearest obstacle point of the fp32-narrowed (px, py, pz); every thread returns the winner.
__device__ __forceinline__ void block_nn_search(const GridDesc &G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                double px, double py, double pz, double stop_d2, double *s_d, uint32_t *s_i, double &bd,
                                                uint32_t &bi)
{
    const uint32_t sub = threadIdx.x & (kCoop - 1), grp = threadIdx.x / kCoop;   // 32 groups
    const float qxf = (float)px, qyf = (float)py, qzf = (float)pz;                    // searchPoint.x = search_Pt(0), :125-128
    const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
    int cx, cy, cz;
    query_cell(G, qxf, qyf, qzf, cx, cy, cz);
    bd = __builtin_huge_val();
    bi = kNoIndex;
    // the cube r = 1, then the shells r = 2, 3, ..
    for (int r = 1;; r++) {
        const int y0 = max(cy - r, 0), y1 = min(cy + r, G.gy - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, G.gz - 1);
        const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
        for (int k = (int)grp; k < nrows; k += 256 / kCoop) {
            shell_row_runs(G, cell_start, cx, cy, cz, r, r == 1, y0 + k % ny, z0 + k / ny,
                           [&](uint32_t s, uint32_t e) { coop_scan_exact(pts, s, e, sub, qx, qy, qz, bd, bi); });
        }
        block_argmin256(bd, bi, s_d, s_i);
        const double bound = cube_bound(G, cx, cy, cz, r, qx, qy, qz);
        if (bound == __builtin_huge_val()) break;             // the cube covers the whole box: every point has been seen
        if (bound > 0.0 && (bd <= bound * bound || bound * bound >= stop_d2)) break;
    }
}

template <bool INFLATE>
__global__ __launch_bounds__(256) void inflate_block_kernel(GridDesc G, const float4 *__restrict__ pts,
                                                            const uint32_t *__restrict__ cell_start, InflateParams P,
                                                            const double *__restrict__ qpts, double stop_d2, uint32_t index_base,
                                                            ExpressOut *__restrict__ out, ExpressSignal sig)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    const uint32_t slot = blockIdx.x;
    const double px = qpts[3 * slot], py = qpts[3 * slot + 1], pz = qpts[3 * slot + 2];
    if (INFLATE && inflate_skips(P, px, py, pz)) {
        if (threadIdx.x == 0) { out[slot].radius = inflate_skipped_radius(P); out[slot].idx = kNoIndex; out[slot].d2 = __builtin_huge_val(); express_done(sig); }
        return;
    }
    double bd;
    uint32_t bi;
    block_nn_search(G, pts, cell_start, px, py, pz, stop_d2, s_d, s_i, bd, bi);
    if (threadIdx.x == 0) {
        if (INFLATE) out[slot].radius = inflate_radius(P, bd);
        out[slot].idx = reported_index(bd, bi, index_base);
        out[slot].d2 = bd;
        express_done(sig);
    }
}

// One RRT* iteration's three dependent queries in ONE launch (corridor_finder.cpp:385-410 genNewNode, :428-437
// findNearstVertex, :464 the treeRewire neighbourhood): a 256-thread block per sample
//   A. nearest tree node of the fp32-narrowed sample (kd_nearestf semantics, lowest index on ties) over the node set,
//   B. steer: centre = nearest + (sample - nearest) * (r_nearest / dist) when the sample lies outside the node's sphere,
//      then the sphere inflation of that centre against the obstacle cloud (radiusSearch :113-133, early-out included),
//   C. the nodes within 2 * float(radius) of the fp32-narrowed centre (candidates for kd_nearest_rangef).
// Sequentially these are three launches + three host round trips (~45-70 us per sample); fused they are one (~20 us),
// for one sample or for a speculative batch.  node_aux[4*i..] = {x, y, z, radius} of node i as the planner holds them
// (fp64 coordinates, float radius widened), in host-mapped memory like the node coordinates themselves.
struct ExpandOut { double cx, cy, cz, radius; uint32_t near_idx, count; };

// (the kernel itself, rrt_expand_kernel<RING>, is in ring.hpp: it searches either index kind)

struct BezierDesc {
    const double *coef;      // device copy of PolyCoeff, nseg x row_stride
    const double *seg_time;  // device
    const int *orders;       // device
    int row_stride, nseg;
    double t_start, stop_time, dt;
    int cap;
};

// sim_planning_demo.cpp:729-771.  Thread 0 enumerates the sample times (bezier_enumerate); then one thread per sample
// evaluates getPosFromBezier (bezier_point).  Outputs: pos (fp64) and nsamples, the unclipped count.
__global__ __launch_bounds__(256) void bezier_samples_kernel(BezierDesc B, double *__restrict__ pos,
                                                             int *__restrict__ nsamples)
{
    extern __shared__ unsigned char smem[];
    double *s_t = reinterpret_cast<double *>(smem);
    int *s_seg = reinterpret_cast<int *>(s_t + B.cap);
    __shared__ int s_n;
    if (threadIdx.x == 0) {
        const int n = (int)bezier_enumerate<false>(B.seg_time, 0, B.nseg, B.t_start, B.stop_time, B.dt, B.cap, kBezierNoBound,
                                                   [&](long long k, double t, int seg) { s_t[k] = t; s_seg[k] = seg; });
        s_n = n;
        *nsamples = n;
    }
    __syncthreads();
    const int n = min(s_n, B.cap);
    for (int s = threadIdx.x; s < n; s += blockDim.x) {
        const int seg = s_seg[s];
        const double T = B.seg_time[seg];
        bezier_point(B.coef + (size_t)seg * B.row_stride, B.orders[seg], T, s_t[s] / T, pos + 3 * s);
    }
}

// Low-latency form of the whole check on an indexed cloud: ONE launch, a 256-thread block per sample.  The host enumerates
// the sample times (bezier_enumerate: IEEE adds are the same on both sides) and hands (segment, t) per sample; the block
// evaluates getPosFromBezier (bezier_point_block), applies the inflation early-out and runs the block-wide cell search.
// Arguments and results live in host-mapped memory; the host picks the first sample with a negative radius.
__global__ __launch_bounds__(256) void bezier_block_kernel(GridDesc G, const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start,
                                                           InflateParams P, const double *__restrict__ coef, int row_stride,
                                                           const double *__restrict__ seg_time, const uint32_t *__restrict__ orders,
                                                           const uint32_t *__restrict__ sample_seg, const double *__restrict__ sample_t,
                                                           double stop_d2, uint32_t index_base, ExpressOut *__restrict__ out,
                                                           double *__restrict__ pos_out, ExpressSignal sig)
{
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    __shared__ double s_term[3 * (kMaxBezierOrder + 1)];
    __shared__ double s_pos[3];
    const uint32_t slot = blockIdx.x;
    const int seg = (int)sample_seg[slot];
    const double T = seg_time[seg];
    bezier_point_block(coef + (size_t)seg * row_stride, (int)orders[seg], T, sample_t[slot] / T, s_term, s_pos);
    const double px = s_pos[0], py = s_pos[1], pz = s_pos[2];
    // every host-visible store of the block comes from thread 0, so one thread fences and signals
    if (threadIdx.x == 0) { pos_out[3 * slot] = px; pos_out[3 * slot + 1] = py; pos_out[3 * slot + 2] = pz; }
    if (inflate_skips(P, px, py, pz)) {
        if (threadIdx.x == 0) { out[slot].radius = inflate_skipped_radius(P); out[slot].idx = kNoIndex; out[slot].d2 = __builtin_huge_val(); express_done(sig); }
        return;
    }
    double bd;
    uint32_t bi;
    block_nn_search(G, pts, cell_start, px, py, pz, stop_d2, s_d, s_i, bd, bi);
    if (threadIdx.x == 0) {
        out[slot].radius = inflate_radius(P, bd);
        out[slot].idx = reported_index(bd, bi, index_base);
        out[slot].d2 = bd;
        express_done(sig);
    }
}

// getPosFromBezier (bezier_point) for host-enumerated samples (segment, t), one thread per sample;
// positions go to device memory for the inflation kernels and to host-mapped memory for the caller
__global__ __launch_bounds__(128) void bezier_eval_kernel(const double *__restrict__ coef, int row_stride, const double *__restrict__ seg_time,
                                                          const uint32_t *__restrict__ orders, const uint32_t *__restrict__ sample_seg,
                                                          const double *__restrict__ sample_t, int n, double *__restrict__ pos_dev,
                                                          double *__restrict__ pos_mapped)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int seg = (int)sample_seg[s];
    const double T = seg_time[seg];
    double p[3];
    bezier_point(coef + (size_t)seg * row_stride, (int)orders[seg], T, sample_t[s] / T, p);
    for (int d = 0; d < 3; d++) { pos_dev[3 * s + d] = p[d]; pos_mapped[3 * s + d] = p[d]; }
}

// first sample with negative radius (checkTrajPtCol, corridor_finder.cpp:412-416); -1 if none
__global__ __launch_bounds__(256) void first_hit_kernel(const double *__restrict__ radius, const int *__restrict__ nsamples,
                                                        int cap, long long *__restrict__ first_hit)
{
    __shared__ int s_min;
    if (threadIdx.x == 0) s_min = 0x7FFFFFFF;
    __syncthreads();
    const int n = min(*nsamples, cap);
    int best = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (radius[i] < 0.0 && i < best) best = i;
    atomicMin(&s_min, best);
    __syncthreads();
    if (threadIdx.x == 0) *first_hit = (s_min == 0x7FFFFFFF) ? -1ll : (long long)s_min;
}

}  // namespace pct
