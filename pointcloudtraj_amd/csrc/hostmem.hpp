// hostmem.hpp -- who owns the host side's buffers and how they grow.  No HIP include: the memory kind is a
// policy (engine_internal.hpp provides device / pinned / host-mapped over the HIP runtime; tests/host/hostmem_check.cpp one over
// malloc), and the wait takes its stream synchronise as a callable.
//
//   Buf<T, Mem>   one owning, grow-only block of T.  Mem::alloc(bytes, &host, &dev) returns 0 or an error code and leaves both
//                 pointers null on failure; Mem::release(host, dev, bytes) frees what alloc handed out.
//   regrow        buffers of different element types and kinds that share one capacity variable, grown as one group
//   pow2_at_least the doubling rule of the grow-only workspaces
//   wait_word     spin on a host-mapped completion word, fall back to the stream
//
// The type decides no policy: how much to allocate, whether to synchronise first and whether growth is allowed at all (graph
// capture) stay with the call site.  A group that fails to grow is left with no member at all (before regrow most sites kept the
// members allocated ahead of the failing one): its capacity variable is 0, and the next call builds the whole group again.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pct_host {

template <typename T, typename Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : h_(o.h_), d_(o.d_), cap_(o.cap_) { o.h_ = o.d_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            release();
            h_ = o.h_; d_ = o.d_; cap_ = o.cap_;
            o.h_ = o.d_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { release(); }

    operator T *() const { return d_; }          // what a kernel or a hipMemcpy takes (the pinned kind: the host pointer itself)
    T *get() const { return d_; }
    T *host() const { return h_; }               // pinned and host-mapped kinds
    size_t capacity() const { return cap_; }     // elements

    void release()
    {
        if (d_ || h_) Mem::release(h_, d_, bytes(cap_));
        h_ = d_ = nullptr;
        cap_ = 0;
    }

    // release, then allocate exactly `count` elements (one element's room when count is 0); empty on failure
    int reset(size_t count)
    {
        release();
        void *h = nullptr, *d = nullptr;
        if (const int st = Mem::alloc(bytes(count), &h, &d)) return st;
        h_ = static_cast<T *>(h);
        d_ = static_cast<T *>(d);
        cap_ = count;
        return 0;
    }

    // grow-only: nothing happens while need <= capacity().  Otherwise the old block goes first (peak memory does not rise) and
    // alloc_count elements are asked for (0: exactly `need`).  The caller makes sure no launch still reads the old block.
    int reserve(size_t need, size_t alloc_count = 0)
    {
        if (need <= cap_) return 0;
        return reset(alloc_count > need ? alloc_count : need);
    }

private:
    static size_t bytes(size_t count) { return (count ? count : 1) * sizeof(T); }
    T *h_ = nullptr, *d_ = nullptr;
    size_t cap_ = 0;
};

// One member of a group and the elements it gets; dropped(): released with the group and left empty (a member the caller does
// not want now, or allocates itself later -- reset(0) would allocate one element's room).
template <typename B>
struct Part {
    B &buf;
    size_t count;
    bool wanted;
};
template <typename B> Part<B> part(B &buf, size_t count) { return { buf, count, true }; }
template <typename B> Part<B> dropped(B &buf) { return { buf, 0, false }; }

// Grow the group guarded by `cap`: cap goes to 0 first, every member is released before any is allocated (peak memory does not
// rise), then the members are allocated in the order listed.  The first failure releases them all, leaves cap 0 and is returned;
// on success cap becomes new_cap.  The caller has decided that the group must grow and has waited for whatever reads it.
template <typename Cap, typename N, typename... B>
int regrow(Cap &cap, N new_cap, Part<B>... parts)
{
    cap = 0;
    (parts.buf.release(), ...);
    int st = 0;
    (void)((parts.wanted ? (st = parts.buf.reset(parts.count)) == 0 : true) && ...);
    if (st) {
        (parts.buf.release(), ...);
        return st;
    }
    cap = static_cast<Cap>(new_cap);
    return 0;
}

// the smallest floor * 2^k that is >= need (floor a power of two: the result is one, and *log2 its exponent)
template <typename I>
I pow2_at_least(I floor, I need, int *log2 = nullptr)
{
    I v = floor;
    while (v < need) v <<= 1;
    if (log2) *log2 = __builtin_ctzll((unsigned long long)v);
    return v;
}

// Wait until the host-mapped word *w holds `want`: spin on it (a stream synchronise costs ~20 us of host time more) and, when
// max_spins run out (0: polling is off), fall back to sync().  Returns whether the word matched after that.
template <typename Sync>
bool wait_word(const volatile uint32_t *w, uint32_t want, long max_spins, Sync sync)
{
    for (long spins = 0; spins < max_spins; spins++) {
        if (*w == want) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; }
        __builtin_ia32_pause();
    }
    sync();
    return *w == want;
}

}  // namespace pct_host
