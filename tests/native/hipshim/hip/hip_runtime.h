// tests/native/hipshim/hip/hip_runtime.h -- TEST ONLY: just enough of HIP for tests/native/sim_errs.cpp to compile
// text_alignment_amd/csrc/ta_errs.hip for the HOST.  A workgroup of one wave runs as 64 coroutines (ucontext) on the
// calling thread, lane after lane: every wave-wide operation the kernel uses (ballot, any, readfirstlane, the DPP
// wave_shr:1 move, the barrier) is a rendezvous -- a lane that reaches one hands over to the next lane, and lane 63 back
// to lane 0, so nobody passes it before everybody has arrived.  The kernel calls them under wave-uniform control flow
// only; a divergent call would pair up different rendezvous and show as a wrong answer or a lane left behind (checked at
// the end of a workgroup).  LDS arrays are function-local statics (one workgroup runs at a time).
#pragma once
#include <stdint.h>
#include <ucontext.h>

#include <algorithm>
#include <functional>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(...)

typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct sim_idx { unsigned x; };
extern sim_idx threadIdx, blockIdx;
struct ulonglong2 { unsigned long long x, y; };
inline ulonglong2 make_ulonglong2(unsigned long long x, unsigned long long y) { return ulonglong2{x, y}; }
using std::max;
using std::min;

constexpr unsigned kSimLanes = 64;
struct sim_wave {
    ucontext_t host, lane[kSimLanes];
    unsigned finished;
    std::function<void()> body;
    unsigned long long slot[kSimLanes];
};
extern sim_wave sim_w;
inline void sim_meet() {
    const unsigned me = threadIdx.x, next = (me + 1) % kSimLanes;
    threadIdx.x = next;
    swapcontext(&sim_w.lane[me], &sim_w.lane[next]);
    threadIdx.x = me;
}

// every lane publishes v; returns what lane `from(lane)` published
template <typename F>
inline unsigned long long sim_exchange(unsigned long long v, F pick) {
    sim_w.slot[threadIdx.x] = v;
    sim_meet();
    const unsigned long long r = pick(sim_w.slot);
    sim_meet();
    return r;
}
inline unsigned long long __ballot(int pred) {
    return sim_exchange(pred != 0, [](const unsigned long long* s) {
        unsigned long long m = 0;
        for (int l = 0; l < 64; ++l) m |= s[l] << l;
        return m;
    });
}
inline int __any(int pred) { return __ballot(pred) != 0ull; }
inline void __syncthreads() { sim_meet(); }
inline void __threadfence() {}
inline int __builtin_amdgcn_readfirstlane(int v) {
    return (int)sim_exchange((unsigned)v, [](const unsigned long long* s) { return s[0]; });
}
// only DPP control 0x138 (wave_shr:1, all rows and banks, no bound control): lane l takes lane l - 1's src, lane 0 keeps old
inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    if (ctrl != 0x138 || row_mask != 0xf || bank_mask != 0xf || bound_ctrl) __builtin_trap();
    const unsigned lane = threadIdx.x;
    return (int)sim_exchange((unsigned)src, [=](const unsigned long long* s) { return lane ? s[lane - 1] : (unsigned long long)(unsigned)old; });
}
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

inline void sim_lane_entry() {
    sim_w.body();
    ++sim_w.finished;                    // uc_link hands over to the next lane, the last lane's to the host
}
inline void sim_launch(std::function<void()> body, dim3 grid, dim3 block) {
    if (block.x != kSimLanes) __builtin_trap();
    constexpr size_t kStack = 256 * 1024;
    std::vector<char> stacks(kStack * kSimLanes);
    sim_w.body = body;
    for (unsigned b = 0; b < grid.x; ++b) {
        for (unsigned l = 0; l < kSimLanes; ++l) {
            getcontext(&sim_w.lane[l]);
            sim_w.lane[l].uc_stack.ss_sp = stacks.data() + kStack * l;
            sim_w.lane[l].uc_stack.ss_size = kStack;
            sim_w.lane[l].uc_link = l + 1 < kSimLanes ? &sim_w.lane[l + 1] : &sim_w.host;
            makecontext(&sim_w.lane[l], sim_lane_entry, 0);
        }
        blockIdx.x = b;
        threadIdx.x = 0;
        sim_w.finished = 0;
        swapcontext(&sim_w.host, &sim_w.lane[0]);
        if (sim_w.finished != kSimLanes) __builtin_trap();      // a lane was left behind at a rendezvous
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) sim_launch([=] { kernel(__VA_ARGS__); }, grid, block)
