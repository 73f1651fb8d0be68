// query_bin.hpp -- the bin of a query in the batch sort (kernels.hpp qsort_*), one definition for the device and the host.
//
// Query binning for the cell-pruned kernels: a counting sort of the batch by coarse cell ((cx,cy,cz) >> shift, x fastest) so that
// neighbouring lanes walk neighbouring cells and share cache lines.  Random 1M-query batches ran 2.5x faster pre-sorted.
// Bin order = (y-strip, z, y inside the strip, x): walking the batch in this order sweeps a strip of `strip` bin rows through all z
// before moving to the next strip, so the planes a stretch of queries re-uses (z-1, z, z+1) are a strip wide, not a whole plane wide,
// and stay inside one XCD's 4 MiB L2 (a full-plane sweep re-fetched every plane ~3x, measured).
//
// Two forms of the same function, chosen per cloud on the host (bin_desc_make), never per item:
//   generic  the definition: cell_coord per axis, >> shift, cy / strip and cy % strip, the linear index in 32-bit multiplies.  On the
//            card that is a division by a run-time value (its reciprocal set up again for every item) and eight slow integer multiplies.
//   FAST     the same bin from full-rate instructions: the coarse coordinate straight from the product scaled by 2^-shift
//            (floor(t) >> s == floor(t * 2^-s) for t >= 0, scaling by a power of two is exact, so the clamp moves to (g - 1) >> s),
//            the strip quotient by a reciprocal the host has checked over every cy in [0, by), and the index from the identity,
//            with s = cy / strip,  ((s * bz + cz) * strip + cy % strip) * bx + cx = (s * (strip * (bz - 1)) + (cz * strip + cy)) * bx + cx:
//            the row number in the brackets as two fp32 multiply-adds on the still unconverted coordinates (integers below 2^24: exact,
//            fused or not), the last step as one 24-bit integer multiply-add.  Valid when every multiplicand fits in 24 bits and
//            every product in 32 (bin_desc_make decides).
//            (The row in 24-bit integer multiply-adds does not survive the compiler: a product whose consumer reads only 24 bits of
//            it loses its operands' masks in the optimiser and comes out of the backend as a full 32-bit multiply again.)
#pragma once

#include <cmath>
#include <cstdint>

namespace pct {

__host__ __device__ __forceinline__ int cell_coord(float v, float o, float inv_h, int g)
{
    float t = floorf((v - o) * inv_h);
    t = fminf(fmaxf(t, 0.0f), (float)(g - 1));
    return (int)t;
}

struct BinDesc {
    int shift, bx, by, bz, strip;
    uint32_t nbins;
    float ox, oy, oz, inv_h;       // the grid's fp32 cell assignment (GridDesc)
    int gx, gy, gz;
    // FAST form, prepared once by bin_desc_make
    int fast;                      // 1: the fields below are valid and the sort kernels use them
    float cscale;                  // inv_h * 2^-shift
    float hx, hy, hz;              // (g - 1) >> shift = b - 1 per axis, as the clamp
    float rstrip;                  // cy / strip == floorf((float)cy * rstrip) for every cy in [0, by)
    float stripf, zmulf;           // strip and strip * (bz - 1)
};

// low 32 bits of the product of the low 24 bits of a and b (on the card v_mul_u32_u24; with an add behind it, v_mad_u32_u24)
__host__ __device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }

template <bool FAST>
__host__ __device__ __forceinline__ uint32_t query_bin(const BinDesc &B, float qx, float qy, float qz)
{
    if (FAST) {
        // fmaxf drops a NaN (-> 0), as in cell_coord; a product that overflows to +inf clamps to b - 1 in both forms
        const float cx = fminf(fmaxf(floorf((qx - B.ox) * B.cscale), 0.0f), B.hx);
        const float cy = fminf(fmaxf(floorf((qy - B.oy) * B.cscale), 0.0f), B.hy);
        const float cz = fminf(fmaxf(floorf((qz - B.oz) * B.cscale), 0.0f), B.hz);
        const float s = floorf(cy * B.rstrip);
        const float row = fmaf(s, B.zmulf, fmaf(cz, B.stripf, cy));
        return mul_u24((uint32_t)(int)row, (uint32_t)B.bx) + (uint32_t)(int)cx;
    }
    const int cx = cell_coord(qx, B.ox, B.inv_h, B.gx) >> B.shift;
    const int cy = cell_coord(qy, B.oy, B.inv_h, B.gy) >> B.shift;
    const int cz = cell_coord(qz, B.oz, B.inv_h, B.gz) >> B.shift;
    const uint32_t s = (uint32_t)cy / (uint32_t)B.strip, yin = (uint32_t)cy % (uint32_t)B.strip;
    return ((s * (uint32_t)B.bz + (uint32_t)cz) * (uint32_t)B.strip + yin) * (uint32_t)B.bx + (uint32_t)cx;
}

// The bin layout of a grid (host, once per index build).  shift is clamped to [0, 4], strip to [1, by].  The FAST form is taken when
//   * inv_h * 2^-shift is a normal fp32 number that scales back to inv_h exactly (so the scaled product is the product, scaled),
//   * the row number (s * bz + cz) * strip + yin stays below 2^24 (exact in fp32, as every partial sum of it) and bx below 2^24
//     (the multiplicands), and the padded bin count below 2^32 (the product: at most the last bin),
//   * a reciprocal of strip exists with floorf(cy * rstrip) == cy / strip, CHECKED for every cy in [0, by) (by <= 2^24 by the above).
// Anything else keeps the generic form.
inline BinDesc bin_desc_make(int gx, int gy, int gz, float ox, float oy, float oz, float inv_h, int shift, int strip)
{
    BinDesc B{};
    B.shift = shift < 0 ? 0 : shift > 4 ? 4 : shift;
    B.gx = gx; B.gy = gy; B.gz = gz;
    B.ox = ox; B.oy = oy; B.oz = oz; B.inv_h = inv_h;
    B.bx = ((gx - 1) >> B.shift) + 1;
    B.by = ((gy - 1) >> B.shift) + 1;
    B.bz = ((gz - 1) >> B.shift) + 1;
    B.strip = strip < 1 ? 1 : strip;
    if (B.strip > B.by) B.strip = B.by;
    const uint64_t rows = (uint64_t)((B.by + B.strip - 1) / B.strip) * (uint64_t)B.strip * (uint64_t)B.bz;
    const uint64_t nbins = (uint64_t)B.bx * rows;
    B.nbins = (uint32_t)nbins;
    B.cscale = std::ldexp(inv_h, -B.shift);
    B.hx = (float)(B.bx - 1); B.hy = (float)(B.by - 1); B.hz = (float)(B.bz - 1);
    B.stripf = (float)B.strip;
    bool ok = std::isnormal(B.cscale) && std::ldexp(B.cscale, B.shift) == inv_h;
    ok = ok && rows <= (1ull << 24) && (uint64_t)B.bx < (1ull << 24) && nbins < (1ull << 32);
    if (ok) {
        B.zmulf = (float)((uint32_t)B.strip * (uint32_t)(B.bz - 1));       // below rows
        ok = false;
        float r = 1.0f / (float)B.strip;         // rounded down, a multiple of strip falls short of its quotient: try the next few up
        for (int t = 0; t < 4 && !ok; t++, r = std::nextafter(r, 2.0f)) {
            bool all = true;
            for (uint32_t cy = 0; cy < (uint32_t)B.by && all; cy++) all = floorf((float)cy * r) == (float)(cy / (uint32_t)B.strip);
            if (all) { B.rstrip = r; ok = true; }
        }
    }
    B.fast = ok ? 1 : 0;
    return B;
}

}  // namespace pct
