// engine_internal.hpp -- what the other translation units of libpct_engine.so (voxel.hip, traj.hip) share with
// engine.hip: the library's stream, lazy initialisation, the error string and the three kinds of memory its buffers
// (hostmem.hpp) live in.  Not part of the ABI (hidden symbols).
#pragma once
#include <hip/hip_runtime.h>

#include "hostmem.hpp"

namespace pct_internal {
__attribute__((visibility("hidden"))) hipStream_t stream();     // the library-owned stream (valid after require_init)
__attribute__((visibility("hidden"))) int require_init();       // pct_init(0) on first use
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Memory kinds of pct_host::Buf (defined in engine.hip; live blocks and bytes are counted for pct_debug_live_buffers)
struct __attribute__((visibility("hidden"))) DeviceMem {         // hipMalloc
    static int alloc(size_t bytes, void **host, void **dev);
    static void release(void *host, void *dev, size_t bytes);
};
struct __attribute__((visibility("hidden"))) PinnedMem {         // hipHostMalloc, default flags: host() and the conversion give the same pointer
    static int alloc(size_t bytes, void **host, void **dev);
    static void release(void *host, void *dev, size_t bytes);
};
struct __attribute__((visibility("hidden"))) MappedMem {         // hipHostMalloc mapped + its device alias
    static int alloc(size_t bytes, void **host, void **dev);
    static void release(void *host, void *dev, size_t bytes);
};
template <typename T> using DevBuf = pct_host::Buf<T, DeviceMem>;
template <typename T> using PinnedBuf = pct_host::Buf<T, PinnedMem>;
template <typename T> using MappedBuf = pct_host::Buf<T, MappedMem>;
}  // namespace pct_internal
