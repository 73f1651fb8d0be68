// ring_remove.hpp -- removing points from the ROLLING obstacle map (ring.hpp) by region or by index (pct_cloud_ring_remove_*).
//
// A point used to leave the window only when the ring cursor overwrote its slot.  A removed slot is a NaN row whose record has been
// retired: its three coordinates read back as NaN (on every path a NaN row is never a neighbour, never counted, never listed and
// keyless for de-dup, include/pct_engine.h), its record is marked dead exactly as an eviction marks it (ring_retire_record), and
// where[slot] = kRingUnfiled, so that the eviction that later overwrites the slot touches nothing.  No query kernel has a new case.
//
// Records now die out of arrival order: a bucket's [head, tail) may hold dead records behind a live head.  Every reader skips
// them; they occupy bucket room until the head passes, and a bucket that looks full spills newcomers to the overflow queue
// (correct, slower; the queue's bound does not depend on the order of deaths, see RingDesc).  Nothing is compacted here.
//
// Counting: every block reduces {rows it removed, rows still live = without a NaN coordinate} and adds them to two device words
// (one atomic each per block, none for a zero); the block holding the last ticket hands the totals and then the sequence word to
// host-mapped memory, where the host polls for them -- one wait per call, as a de-duplicating append waits for its survivor count.
// (The blocks do not add into the host-mapped words themselves: 20 000 blocks of a 5 M-slot window would each cross the bus.)
#pragma once
#include "ring.hpp"

#pragma clang fp contract(off)

namespace pct {

constexpr uint32_t kRemovedBits = 0x7FC00000u;         // the NaN a removed slot's coordinates hold

// device words the blocks of a removal meet on (zero between launches: the last block resets them)
struct RingRemoveMeet { uint32_t removed, live, ticket, pad; };

// the region of a removal: kind 0 = ball (centre a, squared radius r2), kind 1 = box [a, b]; outside != 0 removes the complement.
// A predicate of ring_remove_kernel (below).
struct RingRegion {
    double a[3], b[3], r2;
    int kind, outside;

    // inside <=> ((dx*dx + dy*dy) + dz*dz) <= r*r with dx = (double)x - centre[0] (the rows pct_radius_indices_q64 lists), or
    // lo[k] <= (double)p[k] <= hi[k] on all three axes.  The row holds no NaN; a NaN r*r puts nothing inside.
    __device__ __forceinline__ bool inside(float px, float py, float pz) const
    {
        if (kind == 0) return dist2((double)px, (double)py, (double)pz, a[0], a[1], a[2]) <= r2;
        return a[0] <= (double)px && (double)px <= b[0] && a[1] <= (double)py && (double)py <= b[1] && a[2] <= (double)pz && (double)pz <= b[2];
    }
    __device__ __forceinline__ bool operator()(uint32_t, float px, float py, float pz) const { return inside(px, py, pz) != (outside != 0); }
};

// block-wide: add this block's counts to the meeting words; the last block publishes {seq, removed, live} to the host.
// final == 0: the totals stay on the device for a later launch of the same call to publish (the index-list form)
__device__ __forceinline__ void ring_remove_count(bool removed, bool live, RingRemoveMeet *__restrict__ meet, uint32_t *__restrict__ host_word,
                                                  uint32_t seq, int final)
{
    const uint32_t n_removed = (uint32_t)__syncthreads_count(removed ? 1 : 0);
    const uint32_t n_live = (uint32_t)__syncthreads_count(live ? 1 : 0);
    if (threadIdx.x != 0) return;
    if (n_removed) atomicAdd(&meet->removed, n_removed);
    if (n_live) atomicAdd(&meet->live, n_live);
    if (!final) return;
    __threadfence();
    if (atomicAdd(&meet->ticket, 1u) != gridDim.x - 1u) return;
    __threadfence();
    const uint32_t tr = atomicExch(&meet->removed, 0u), tl = atomicExch(&meet->live, 0u);
    atomicExch(&meet->ticket, 0u);
    __hip_atomic_store(&host_word[1], tr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_word[2], tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(&host_word[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Everything a removal kernel needs to edit one window: the mutable counterpart of RingView (ring.hpp), built by the host's
// ring_edit().  `count` = the window's size; meet / host_word / seq: the meeting words above, the host-mapped {seq, removed, live}
// triple the last block publishes, and the sequence number the host waits for.
struct RingEdit {
    RingDesc R;
    float *x, *y, *z;
    uint32_t count;
    uint2 *ht;
    float4 *slots, *ovf;
    uint32_t *where;
    RingState *st;
    RingRemoveMeet *meet;
    uint32_t *host_word;
    uint32_t seq;
};

// One thread per slot below the window's size: a row without a NaN that `condemned(slot, px, py, pz)` names is retired, becomes a
// NaN row and is marked unfiled.  The predicate is asked about no other slot: what it reads at `slot` lies below the size, and a NaN
// row costs it nothing.  No record is filed while this runs (appends are ordered before and after it on the stream).
template <typename Pred>
__device__ __forceinline__ void ring_remove_where(const RingEdit &E, const Pred &condemned)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q_tail = E.st->ovf_tail;
    const bool queue_in_use = q_tail != E.st->ovf_head;
    bool removed = false, live = false;
    if (slot < E.count) {
        const float px = E.x[slot], py = E.y[slot], pz = E.z[slot];
        if (px == px && py == py && pz == pz) {
            removed = condemned(slot, px, py, pz);
            live = !removed;
            if (removed) {
                ring_retire_record(E.R, E.where[slot], px, py, pz, E.ht, E.slots, E.ovf);
                const float gone = __uint_as_float(kRemovedBits);
                E.x[slot] = gone; E.y[slot] = gone; E.z[slot] = gone;
                E.where[slot] = kRingUnfiled;
            }
        }
    }
    if (queue_in_use) ring_queue_head_advance(E.R, E.ovf, E.st, q_tail);
    ring_remove_count(removed, live, E.meet, E.host_word, E.seq, 1);
}

// THE one-pass removal kernel: ball and box (RingRegion), the depth-image and range-image carves (DepthSeenThrough, ring_depth.hpp; RangeSeenThrough, ring_range.hpp), radius
// outliers (RoBelow, ring_outlier.hpp) and statistical / isolated outliers (KsAbove, ring_statistical.hpp) differ in `Pred` alone,
// a small trivially-copyable functor passed by value.  The host's ring_remove_run launches it.
template <typename Pred>
__global__ __launch_bounds__(256) void ring_remove_kernel(RingEdit E, Pred condemned)
{
    ring_remove_where(E, condemned);
}

// One thread per list entry (ring slots, already validated against the window by the host).  A slot named twice is claimed once:
// the compare-and-swap of the NaN pattern into x[slot] succeeds for one thread only, and a row that already holds a NaN is left
// alone.  The live count comes from ring_live_count_kernel, launched behind this one: nothing is published here (E.host_word and
// E.seq are not looked at).
__global__ __launch_bounds__(256) void ring_remove_list_kernel(RingEdit E, const uint32_t *__restrict__ list, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q_tail = E.st->ovf_tail;
    const bool queue_in_use = q_tail != E.st->ovf_head;
    bool removed = false;
    if (i < n) {
        const uint32_t slot = list[i];
        uint32_t *xw = reinterpret_cast<uint32_t *>(E.x) + slot;
        const uint32_t xb = __hip_atomic_load(xw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float px = __uint_as_float(xb);
        // y and z become NaN only after x has been claimed: a NaN seen here means "already a NaN row" or "claimed by another entry"
        uint32_t *yw = reinterpret_cast<uint32_t *>(E.y) + slot, *zw = reinterpret_cast<uint32_t *>(E.z) + slot;
        const float py = __uint_as_float(__hip_atomic_load(yw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const float pz = __uint_as_float(__hip_atomic_load(zw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (px == px && py == py && pz == pz && atomicCAS(xw, xb, kRemovedBits) == xb) {
            removed = true;
            ring_retire_record(E.R, E.where[slot], px, py, pz, E.ht, E.slots, E.ovf);
            __hip_atomic_store(yw, kRemovedBits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(zw, kRemovedBits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            E.where[slot] = kRingUnfiled;
        }
    }
    if (queue_in_use) ring_queue_head_advance(E.R, E.ovf, E.st, q_tail);
    ring_remove_count(removed, false, E.meet, nullptr, 0u, 0);
}

// rows below the size without a NaN coordinate; publishes {seq, removed so far in this call, live}.  Of E it reads x, y, z, count,
// meet, host_word and seq alone
__global__ __launch_bounds__(256) void ring_live_count_kernel(RingEdit E)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool live = false;
    if (slot < E.count) {
        const float px = E.x[slot], py = E.y[slot], pz = E.z[slot];
        live = px == px && py == py && pz == pz;
    }
    ring_remove_count(false, live, E.meet, E.host_word, E.seq, 1);
}

}  // namespace pct
