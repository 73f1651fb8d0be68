// segment_polyhedron.hpp -- FREE-SPACE POLYHEDRA: the supports of a capsule row and their planes (pct_segment_polyhedron_batch,
// pct_segment_supports_dev), for gfx950.
//
// The contract is the paragraph "Free-space polyhedra" of include/pct_engine.h: walk row i of the capsule search in
// PCT_ORDER_DISTANCE; an entry is a SUPPORT iff no earlier support of the row cuts it; support p (n = its c of "Segment queries")
// cuts a later entry x iff h = (n0*u0 + n1*u1) + n2*u2 >= 0 with u = x - p.  Everything is fp64 on float-widened operands, one
// rounding per operation, no contraction.  The decomposition is a pure filter over a row the capsule search has made: no walk, no
// index -- which is why it inherits all three index forms and their exactness.
//
// poly_filter_kernel: one 256-thread block per row.  The row is taken in WINDOWS of kPolyLds entries, gathered once into LDS as
// fp32 x / y / z in three arrays (12 B per entry; lane l of a wave reads word l of a 64-entry chunk: 32 distinct banks per group of
// 32 lanes, conflict-free) beside an alive mask of one bit per entry (kPolyLds / 64 words of 64 bits: one wave reads the whole mask,
// a word per lane).  A window is first swept by the supports found in earlier windows -- staged kPolyStage at a time into LDS with
// their normals, every thread judging its own 16 entries -- and then continued greedily:
//     find   every wave reads the mask, blanks what lies before the cursor, and takes the first set bit by a ballot over the words;
//            all four waves do this for themselves and arrive at the same entry, so nothing is broadcast;
//     mark   thread 0 appends the entry's position in the row to sup[] (the row's own slice of a per-entry buffer: supports are
//            found in row order, so their list needs no scan); every thread reads p from LDS and computes n;
//     sweep  wave w takes the 64-entry chunks c == w (mod 4) behind the support: a lane tests one alive entry, a ballot collects the
//            cut ones and lane 0 clears them in the chunk's word -- only this wave ever writes that word, no atomics;
//     one barrier, and the next trip.
// A wave that is ahead clears only bits BEHIND the support its slower neighbours are still looking for, so they find the same
// entry and take the same exit.  The trip count is the number of supports: tens on surface clouds, the whole row in the worst case
// (points on a sphere around a degenerate segment).  Rows longer than a window are served with the same bytes: the greedy order is
// the row's order whichever window an entry sits in, and an entry is alive in its window iff no earlier support cuts it.
//
// kPolyLds = 4096: 48 KiB of coordinates + 512 B of mask + 9 KiB of staged supports = 57.5 KiB static -- under 64 KiB, two blocks
// a CU with room to spare (160 KiB per CU), and the mask is exactly one word per lane of a wave.
//
// poly_emit_kernel writes idx / d2 / s / plane of the supports in row order behind the scan of the counts (list_scan): everything is
// recomputed from the segment and the row the index names, of which it is a function (as ss_param_kernel argues for s).
#pragma once
#include "segment_search.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr int kPolyLds = 4096;                    // entries of a row a block keeps in LDS at a time
constexpr int kPolyPer = kPolyLds / 256;          // ... per thread
constexpr int kPolyWords = kPolyLds / 64;         // words of the alive mask
constexpr int kPolyStage = 256;                   // earlier supports staged per trip of a later window's first sweep
static_assert(kPolyWords == kWave, "one wave reads the whole alive mask, a word per lane");
static_assert(kPolyLds * 12 + kPolyWords * 8 + kPolyStage * 36 <= 65536, "static LDS within 64 KiB");

// d2 and s of the widened row p on segment S ("Segment queries") and the normal n_k = w_k - s * e_k, that paragraph's c_k: the
// same operations on the same operands as inside seg_point_terms, hence the same bits
__device__ __forceinline__ void poly_normal(const SegGeom &S, double px, double py, double pz, double &n0, double &n1, double &n2, double &d2,
                                            double &s)
{
    seg_point_d2(S, px, py, pz, d2, s);
    const double w0 = px - S.ax, w1 = py - S.ay, w2 = pz - S.az;
    n0 = w0 - s * S.ex; n1 = w1 - s * S.ey; n2 = w2 - s * S.ez;
}

// THE cut test: does the support (p, n) cut the widened row x
__device__ __forceinline__ bool poly_cuts(double px, double py, double pz, double n0, double n1, double n2, double xx, double xy, double xz)
{
    const double u0 = xx - px, u1 = xy - py, u2 = xz - pz;
    const double h = (n0 * u0 + n1 * u1) + n2 * u2;
    return h >= 0.0;
}

// The rows (row_offsets[Q + 1], row_idx: the capsule search's CSR in PCT_ORDER_DISTANCE) -> count[row] = supports of the row,
// sup[row_offsets[row] + j] = the position inside the row of its j-th support.  Nothing but count[] (zeros) is written when
// row_offsets[Q] > row_cap -- the rows were never made -- and a row whose bounds do not lie in order inside [0, row_offsets[Q]] is
// taken as empty.  An entry whose index lies outside the cloud, or names a row that is not finite, is never alive.
__global__ __launch_bounds__(256) void poly_filter_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                          uint32_t n, const double *__restrict__ seg, uint32_t Q, uint32_t index_base,
                                                          const long long *__restrict__ row_offsets, long long row_cap,
                                                          const uint32_t *__restrict__ row_idx, uint32_t *__restrict__ sup,
                                                          uint32_t *__restrict__ count)
{
    __shared__ float s_x[kPolyLds], s_y[kPolyLds], s_z[kPolyLds];
    __shared__ unsigned long long s_alive[kPolyWords];
    __shared__ double s_sn[kPolyStage][3];
    __shared__ float s_sp[kPolyStage][3];
    const uint32_t row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long off0 = row_offsets[row], off1 = row_offsets[row + 1], tot = row_offsets[Q];
    SegGeom S;
    double bx, by, bz;
    const bool finite = seg_load(seg, row, S, bx, by, bz);
    const bool ok = finite && tot <= row_cap && off0 >= 0 && off0 <= off1 && off1 <= tot;      // block-uniform
    const long long len = ok ? off1 - off0 : 0;
    const float finf = __builtin_huge_valf();
    uint32_t nsup = 0;
    for (long long w0 = 0; w0 < len; w0 += kPolyLds) {      // block-uniform trip count
        const int wn = (int)min((long long)kPolyLds, len - w0);
        __syncthreads();                                    // the previous window's last find has read the mask
        // gather: entry e = k * 256 + thread; bit k of `mine`: it can be a support
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < kPolyPer; k++) {
            const int e = k * 256 + (int)threadIdx.x;
            if (e < wn) {
                const uint32_t i = row_idx[off0 + w0 + e] - index_base;
                if (i < n) {                                // an index outside the cloud is never dereferenced
                    const float fx = x[i], fy = y[i], fz = z[i];
                    s_x[e] = fx; s_y[e] = fy; s_z[e] = fz;
                    if (fabsf(fx) < finf && fabsf(fy) < finf && fabsf(fz) < finf) mine |= 1u << k;
                }
            }
        }
        // the supports of earlier windows, kPolyStage at a time (nsup == 0 in the first window)
        for (uint32_t j0 = 0; j0 < nsup; j0 += kPolyStage) {
            __syncthreads();                                // the stage is free; sup[] of earlier trips is visible
            const uint32_t j = j0 + threadIdx.x;
            if (j < nsup) {
                const uint32_t i = row_idx[off0 + sup[off0 + j]] - index_base;      // a support: inside the cloud
                const float fx = x[i], fy = y[i], fz = z[i];
                double n0, n1, n2, d2, s;
                poly_normal(S, (double)fx, (double)fy, (double)fz, n0, n1, n2, d2, s);
                s_sp[threadIdx.x][0] = fx; s_sp[threadIdx.x][1] = fy; s_sp[threadIdx.x][2] = fz;
                s_sn[threadIdx.x][0] = n0; s_sn[threadIdx.x][1] = n1; s_sn[threadIdx.x][2] = n2;
            }
            __syncthreads();
            const int m = (int)min((uint32_t)kPolyStage, nsup - j0);
#pragma unroll 1
            for (int k = 0; k < kPolyPer; k++) {
                if (!((mine >> k) & 1u)) continue;
                const int e = k * 256 + (int)threadIdx.x;
                const double xx = (double)s_x[e], xy = (double)s_y[e], xz = (double)s_z[e];
                for (int t = 0; t < m; t++)
                    if (poly_cuts((double)s_sp[t][0], (double)s_sp[t][1], (double)s_sp[t][2], s_sn[t][0], s_sn[t][1], s_sn[t][2], xx, xy, xz)) {
                        mine &= ~(1u << k);
                        break;
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < kPolyPer; k++) {                // chunk k * 4 + wave holds this wave's entries k
            const unsigned long long b = __builtin_amdgcn_ballot_w64((mine >> k) & 1u);
            if (lane == 0) s_alive[k * 4 + wave] = b;
        }
        __syncthreads();
        // the greedy loop of this window
        const int nchunks = (wn + 63) >> 6;
        int cursor = 0;
        for (;;) {
            unsigned long long wd = s_alive[lane];
            const int cw = cursor >> 6;
            if (lane < cw) wd = 0;
            else if (lane == cw) wd &= ~0ull << (cursor & 63);
            const unsigned long long any = __builtin_amdgcn_ballot_w64(wd != 0);
            if (!any) break;                                // the same in every wave (see above)
            const int fw = __builtin_ctzll(any);
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)wd, fw, kWave), hi = (uint32_t)__shfl((int)(uint32_t)(wd >> 32), fw, kWave);
            const int pos = fw * 64 + (lo ? __builtin_ctz(lo) : 32 + __builtin_ctz(hi));
            if (threadIdx.x == 0) sup[off0 + nsup] = (uint32_t)(w0 + pos);       // nsup < len: a support is an entry of the row
            nsup++;
            const double px = (double)s_x[pos], py = (double)s_y[pos], pz = (double)s_z[pos];
            double n0, n1, n2, d2, s;
            poly_normal(S, px, py, pz, n0, n1, n2, d2, s);
            const int c0 = pos >> 6;
            for (int c = c0 + ((wave - c0) & 3); c < nchunks; c += 4) {
                const unsigned long long old = s_alive[c];
                const int e = c * 64 + lane;
                const bool live = ((old >> lane) & 1ull) && e > pos;
                if (!__builtin_amdgcn_ballot_w64(live)) continue;                // wave-uniform
                const bool cut = live && poly_cuts(px, py, pz, n0, n1, n2, (double)s_x[e], (double)s_y[e], (double)s_z[e]);
                const unsigned long long cm = __builtin_amdgcn_ballot_w64(cut);
                if (lane == 0 && cm) s_alive[c] = old & ~cm;
            }
            cursor = pos + 1;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) count[row] = nsup;
}

// The supports of every row in row order behind the scan: entry offsets[row] + j is the row's j-th support -- idx as the row names
// it, d2 and s of "Segment queries", and the plane nh0 nh1 nh2 off with d = sqrt(d2), nh_k = n_k / d, off = (nh0*p0 + nh1*p1) +
// nh2*p2; (0, 0, 0, -1) when d2 == 0.  Written only when offsets[Q] <= cap.  When the rows were never made (row_offsets[Q] >
// row_cap) every entry of offsets becomes -1 instead and nothing else is touched.  Blocks take the rows in turn.
__global__ __launch_bounds__(256) void poly_emit_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                        uint32_t n, const double *__restrict__ seg, uint32_t Q, uint32_t index_base,
                                                        const long long *__restrict__ row_offsets, long long row_cap,
                                                        const uint32_t *__restrict__ row_idx, const uint32_t *__restrict__ sup,
                                                        long long *__restrict__ offsets, long long cap, uint32_t *__restrict__ out_idx,
                                                        double *__restrict__ out_d2, double *__restrict__ out_s, double *__restrict__ out_plane)
{
    if (row_offsets[Q] > row_cap) {                         // grid-uniform: no block reads offsets[] on this side
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= Q; i += gridDim.x * 256u) offsets[i] = -1;
        return;
    }
    if (offsets[Q] > cap) return;
    for (uint32_t row = blockIdx.x; row < Q; row += gridDim.x) {
        const long long o0 = offsets[row], cnt = offsets[row + 1] - o0;
        if (cnt == 0) continue;
        const long long off0 = row_offsets[row];
        SegGeom S;
        double bx, by, bz;
        (void)seg_load(seg, row, S, bx, by, bz);
        for (long long j = threadIdx.x; j < cnt; j += 256) {
            const uint32_t id = row_idx[off0 + sup[off0 + j]];
            const uint32_t i = id - index_base;
            if (i >= n) continue;                           // cannot be: a support lies inside the cloud
            const double px = (double)x[i], py = (double)y[i], pz = (double)z[i];
            double n0, n1, n2, d2, s;
            poly_normal(S, px, py, pz, n0, n1, n2, d2, s);
            out_idx[o0 + j] = id;
            if (out_d2) out_d2[o0 + j] = d2;
            if (out_s) out_s[o0 + j] = s;
            if (out_plane) {
                double *P = out_plane + 4 * (o0 + j);
                if (d2 == 0.0) { P[0] = 0.0; P[1] = 0.0; P[2] = 0.0; P[3] = -1.0; }
                else {
                    const double d = sqrt(d2);
                    const double h0 = n0 / d, h1 = n1 / d, h2 = n2 / d;
                    P[0] = h0; P[1] = h1; P[2] = h2;
                    P[3] = (h0 * px + h1 * py) + h2 * pz;
                }
            }
        }
    }
}

}  // namespace pct
