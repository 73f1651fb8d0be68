// The handful of HIP built-ins a kernel written in plain C++ needs, on the CPU: one std::thread per lane of ONE workgroup at a time,
// __syncthreads as a std::barrier.  For tests/host/trajgen_check.cpp only (-std=c++20; no HIP runtime, no device).
#pragma once
#include <atomic>
#include <barrier>
#include <cmath>

#define __global__
#define __device__
#define __host__
#define __shared__
#define __launch_bounds__(...)

struct hip_stub_dim3 { unsigned x, y, z; };
inline thread_local hip_stub_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0};

namespace hip_stub {
inline std::barrier<> *g_barrier = nullptr;       // set by the program before it starts the lanes
inline std::atomic<int> g_or{0};
}  // namespace hip_stub

inline void __syncthreads() { hip_stub::g_barrier->arrive_and_wait(); }
inline int __syncthreads_or(int p)
{
    if (p) hip_stub::g_or.store(1);
    __syncthreads();
    const int r = hip_stub::g_or.load();
    __syncthreads();
    if (threadIdx.x == 0) hip_stub::g_or.store(0);
    __syncthreads();
    return r;
}

using std::isfinite;
