// Stand-alone check of csrc/hostmem.hpp (tests/test_hostmem.py builds it with -fsanitize=address,undefined and runs it).
// The memory kind is a fake over malloc that counts live blocks and can be told to fail the k-th allocation from now.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <utility>

#include "../../pointcloudtraj_amd/csrc/hostmem.hpp"

namespace {

int g_live = 0, g_allocs = 0, g_releases = 0, g_fail_in = 0, g_live_at_last_request = -1;
size_t g_live_bytes = 0;
constexpr int kErr = -7;

struct FakeMem {
    static int alloc(size_t bytes, void **host, void **dev)
    {
        *host = *dev = nullptr;
        g_live_at_last_request = g_live;
        if (g_fail_in > 0 && --g_fail_in == 0) return kErr;
        *dev = std::malloc(bytes);
        g_live++; g_allocs++; g_live_bytes += bytes;
        return 0;
    }
    static void release(void *host, void *dev, size_t bytes)
    {
        if (host) std::abort();          // this kind hands out no host pointer
        std::free(dev);
        g_live--; g_releases++; g_live_bytes -= bytes;
    }
};

// a pair of pointers to one block, as the host-mapped kind hands out (the "device alias" is the block shifted by one byte, so a
// mix-up of the two shows)
int g_pair_live = 0, g_pair_releases = 0;
struct FakePair {
    static int alloc(size_t bytes, void **host, void **dev)
    {
        *host = std::malloc(bytes + 1);
        *dev = static_cast<char *>(*host) + 1;
        g_pair_live++;
        return 0;
    }
    static void release(void *host, void *dev, size_t)
    {
        if (dev != static_cast<char *>(host) + 1) std::abort();
        std::free(host);
        g_pair_live--; g_pair_releases++;
    }
};

using B = pct_host::Buf<int, FakeMem>;
static_assert(!std::is_copy_constructible<B>::value, "Buf must not be copy-constructible");
static_assert(!std::is_copy_assignable<B>::value, "Buf must not be copy-assignable");
static_assert(std::is_move_constructible<B>::value && std::is_move_assignable<B>::value, "Buf must be movable");

int g_failed = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

void check_buf()
{
    {
        B b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b);
        CHECK(b.reserve(0) == 0 && g_allocs == 0);                  // nothing needed, nothing asked for
        CHECK(b.reserve(100) == 0 && b.capacity() == 100 && g_live == 1);
        int *p = b;
        p[99] = 1;
        const int allocs = g_allocs;
        CHECK(b.reserve(100) == 0 && b.reserve(7) == 0);            // within capacity: no allocation, the block stays
        CHECK(g_allocs == allocs && b.get() == p);
        CHECK(b.reserve(101, 256) == 0 && b.capacity() == 256);     // growth: the old block goes first
        CHECK(g_live_at_last_request == 0 && g_live == 1);
        b.get()[255] = 1;
        g_fail_in = 1;                                               // a failed growth: empty, the error, nothing live
        CHECK(b.reserve(1000) == kErr);
        CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 0);
        CHECK(b.reserve(1000) == 0 && b.capacity() == 1000 && g_live == 1);   // ... and a later one succeeds
        CHECK(b.reset(3) == 0 && b.capacity() == 3 && g_live == 1);  // reset: exactly that many
        CHECK(g_live_at_last_request == 0);
        const int rel = g_releases;
        b.release();
        CHECK(g_releases == rel + 1 && g_live == 0 && b.get() == nullptr && b.capacity() == 0);
        b.release();                                                 // once
        CHECK(g_releases == rel + 1);
        CHECK(b.reset(0) == 0 && b.get() != nullptr && b.capacity() == 0 && g_live == 1);   // room for one element, as the engine's allocations
    }
    CHECK(g_live == 0 && g_live_bytes == 0 && g_allocs == g_releases);        // the destructor freed the last block, once
    {
        B a;
        CHECK(a.reset(10) == 0);
        int *p = a;
        B b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 10 && g_live == 1);
        B c;
        CHECK(c.reset(5) == 0 && g_live == 2);
        c = std::move(b);                                            // the target's block goes, the source is left empty
        CHECK(g_live == 1 && b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 10);
    }
    CHECK(g_live == 0 && g_live_bytes == 0 && g_allocs == g_releases);
    {
        pct_host::Buf<double, FakePair> m;
        CHECK(m.reset(8) == 0 && g_pair_live == 1);
        CHECK(m.host() != nullptr && (char *)m.get() == (char *)m.host() + 1 && (double *)m == m.get());
        m.host()[7] = 1.0;
        CHECK(m.reserve(9) == 0 && g_pair_live == 1 && g_pair_releases == 1);
    }
    CHECK(g_pair_live == 0 && g_pair_releases == 2);
}

// pct_host::regrow over three element types and a fourth part that is only released, under one capacity variable
void check_group()
{
    using pct_host::dropped;
    using pct_host::part;
    {
        B a, d;
        pct_host::Buf<double, FakeMem> b;
        pct_host::Buf<char, FakeMem> c;
        size_t cap = 0;
        const auto ensure = [&](size_t n) {
            if (n <= cap) return 0;                                  // the call site's own test
            return pct_host::regrow(cap, n, part(a, n), part(b, 2 * n), part(c, n / 2 + 1), dropped(d));
        };
        const auto none_live = [&] { return !a && !b && !c && !d && g_live == 0; };
        CHECK(d.reset(4) == 0 && g_live == 1);                       // the fourth holds a block of its own before the first growth
        for (size_t n : { (size_t)64, (size_t)128 }) {               // 0 -> n -> 2n
            CHECK(ensure(n) == 0 && cap == n && g_live == 3);
            CHECK(a.capacity() == n && b.capacity() == 2 * n && c.capacity() == n / 2 + 1);
            CHECK(!d && d.capacity() == 0);                          // released with the group, not allocated
            a.get()[n - 1] = 1; b.get()[2 * n - 1] = 1.0; c.get()[n / 2] = 1;
        }
        int allocs = g_allocs;
        g_live_at_last_request = -1;
        CHECK(ensure(256) == 0 && cap == 256 && g_live == 3);
        CHECK(g_allocs == allocs + 3);
        allocs = g_allocs;
        const int rel = g_releases;
        CHECK(ensure(256) == 0 && ensure(1) == 0);                   // the test passes: nothing is allocated or released
        CHECK(g_allocs == allocs && g_releases == rel && cap == 256);
        for (int k = 1; k <= 3; k++) {                               // the k-th allocation of a regrowth fails
            const size_t n = 2 * cap;
            g_fail_in = k;
            CHECK(ensure(n) == kErr);
            CHECK(cap == 0 && none_live());
            CHECK(ensure(n) == 0 && cap == n && g_live == 3);        // ... and the next growth builds the whole group
            CHECK(a.capacity() == n && b.capacity() == 2 * n && c.capacity() == n / 2 + 1 && !d);
        }
    }
    CHECK(g_live == 0 && g_live_bytes == 0 && g_allocs == g_releases);
    {
        // every old block is gone before the first allocation of a regrowth asks for memory
        B a;
        pct_host::Buf<double, FakeMem> b;
        pct_host::Buf<char, FakeMem> c;
        size_t cap = 0;
        CHECK(pct_host::regrow(cap, 8, part(a, 8), part(b, 8), part(c, 8)) == 0 && g_live == 3);
        g_fail_in = 1;                                               // the first request of the regrowth is the last one made
        CHECK(pct_host::regrow(cap, 16, part(a, 16), part(b, 16), part(c, 16)) == kErr);
        CHECK(g_live_at_last_request == 0 && cap == 0 && g_live == 0);
    }
    CHECK(g_live == 0 && g_live_bytes == 0 && g_allocs == g_releases);
}

void check_pow2()
{
    using pct_host::pow2_at_least;
    int lg = -1;
    CHECK(pow2_at_least<int64_t>(4096, 0) == 4096);
    CHECK(pow2_at_least<int64_t>(4096, 4096) == 4096);
    CHECK(pow2_at_least<int64_t>(4096, 4097) == 8192);
    CHECK(pow2_at_least<size_t>((size_t)1 << 16, ((size_t)1 << 20)) == (size_t)1 << 20);
    CHECK(pow2_at_least<size_t>((size_t)1 << 16, ((size_t)1 << 20) + 1) == (size_t)1 << 21);
    CHECK(pow2_at_least<int64_t>(1, 0, &lg) == 1 && lg == 0);
    CHECK(pow2_at_least<int64_t>(1, 5, &lg) == 8 && lg == 3);
    CHECK(pow2_at_least<uint64_t>(1024, 2ull * 5000) == 16384);
}

void check_wait_word()
{
    using pct_host::wait_word;
    {
        std::atomic<uint32_t> word{ 0 };                             // stands for the host-mapped word a kernel's last block stores
        const volatile uint32_t *w = reinterpret_cast<const volatile uint32_t *>(&word);
        int syncs = 0;
        std::thread t([&] { std::this_thread::sleep_for(std::chrono::milliseconds(20)); word.store(5, std::memory_order_release); });
        const bool seen = wait_word(w, 5u, 2000000000l, [&] { syncs++; });
        t.join();
        CHECK(seen && syncs == 0);
    }
    {
        uint32_t word = 3;
        int syncs = 0;
        CHECK(!wait_word(&word, 4u, 1000, [&] { syncs++; }) && syncs == 1);      // nobody stores it: one sync, no match
        syncs = 0;
        CHECK(wait_word(&word, 4u, 1000, [&] { syncs++; word = 4; }) && syncs == 1);   // the sync lets the store land
        syncs = 0;
        CHECK(wait_word(&word, 4u, 0, [&] { syncs++; }) && syncs == 1);          // polling off: straight to the sync
    }
}

}  // namespace

int main()
{
    check_buf();
    check_group();
    check_pow2();
    check_wait_word();
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("hostmem ok\n");
    return 0;
}
