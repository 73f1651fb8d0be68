// vox_key.hpp -- voxel keys and the open-addressing key table, shared by voxel.hip (pct_voxel_map) and ring_dedup.hpp (the
// de-duplicating appends of the rolling map): one definition of "which voxel is this point in" for both.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pct_vox {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int kVoxBias = 1 << 20;                 // voxel coordinates in [-2^20, 2^20)

__device__ __forceinline__ uint32_t vox_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;   // murmur3 finaliser
    return (uint32_t)k;
}

// voxel_map.cpp:5-16: (int) round(coordinate / res), fp64 division on the (widened) coordinate
template <typename T>
__device__ __forceinline__ bool vox_coords(const unsigned char *rec, double res, int &ix, int &iy, int &iz)
{
    const T *p = reinterpret_cast<const T *>(rec);
    const double rx = round((double)p[0] / res), ry = round((double)p[1] / res), rz = round((double)p[2] / res);
    const double lim = (double)kVoxBias;
    if (!(rx >= -lim && rx < lim && ry >= -lim && ry < lim && rz >= -lim && rz < lim)) return false;   // also NaN
    ix = (int)rx; iy = (int)ry; iz = (int)rz;
    return true;
}

__device__ __forceinline__ unsigned long long vox_pack(int ix, int iy, int iz)
{
    return (unsigned long long)(uint32_t)(ix + kVoxBias) | ((unsigned long long)(uint32_t)(iy + kVoxBias) << 21) |
           ((unsigned long long)(uint32_t)(iz + kVoxBias) << 42);
}

__device__ __forceinline__ void vox_unpack(unsigned long long key, int &ix, int &iy, int &iz)
{
    ix = (int)(uint32_t)(key & 0x1FFFFFull) - kVoxBias;
    iy = (int)(uint32_t)((key >> 21) & 0x1FFFFFull) - kVoxBias;
    iz = (int)(uint32_t)((key >> 42) & 0x1FFFFFull) - kVoxBias;
}

// (internal linkage: the header is compiled into more than one translation unit of the library)
static __global__ __launch_bounds__(256) void vox_table_init_kernel(unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t T)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < T; i += stride) { keys[i] = kEmptyKey; vals[i] = 0xFFFFFFFFu; }
}

__device__ __forceinline__ uint32_t vox_find_or_claim(unsigned long long *__restrict__ keys, uint32_t mask, unsigned long long key)
{
    uint32_t slot = vox_hash(key) & mask;
    for (uint32_t probes = 0; probes <= mask; probes++) {
        const unsigned long long seen = keys[slot];                       // most points hit an existing voxel: plain read first
        if (seen == key) return slot;
        if (seen == kEmptyKey) {
            const unsigned long long old = atomicCAS(&keys[slot], kEmptyKey, key);
            if (old == kEmptyKey || old == key) return slot;
        }
        slot = (slot + 1) & mask;
    }
    return kNoSlot;
}

}  // namespace pct_vox
