// tests/native/hipshim_wg/hip/hip_runtime.h -- TEST ONLY: just enough of HIP for tests/native/sim_lineest.cpp,
// tests/native/sim_train.cpp and tests/native/sim_distort.cpp to compile text_alignment_amd/csrc/ta_lineest.hip,
// ta_train.hip and ta_distort.hip for the HOST.  Beside tests/native/hipshim (one wave of 64 lanes, wave-wide
// operations), which stays what it is for the sims that use it; this one is for kernels whose only meeting point is
// __syncthreads(): workgroups of the launch's block.x lanes (64 .. 512, a multiple of 64), a grid in x, y and z, one workgroup after the other (blockIdx.x fastest, z slowest) on the
// calling thread -- every launch is synchronous and streams are ignored.  LDS arrays are function-local statics.
//
// A workgroup starts with lane 0 alone, as a coroutine (ucontext).  If lane 0 ends without having met a barrier, the other
// lanes are plain calls, one after the other: most workgroups of a grid are of that kind, or have nothing to do at
// all.  At lane 0's first __syncthreads() the other lanes become coroutines too, and from then on a barrier is a
// rendezvous: a lane that reaches one hands over to the next lane, the last lane back to lane 0, so nobody passes it before
// everybody has arrived.  A lane that leaves a loop body early (`continue`) simply arrives at the next barrier first.  All
// lanes of a workgroup must meet the same number of barriers; a lane left behind, or a barrier met by a lane after lane 0
// ended without one, aborts with a message.
// Under AddressSanitizer every switch is announced (sanitizer/common_interface_defs.h: start / finish_switch_fiber), so
// the sanitizer knows which stack it is on.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/common_interface_defs.h>
#define SIM_FIBER_LEAVE(save, bottom, size) __sanitizer_start_switch_fiber(save, bottom, size)
#define SIM_FIBER_ARRIVE(save, bottom, size) __sanitizer_finish_switch_fiber(save, bottom, size)
#else
#define SIM_FIBER_LEAVE(save, bottom, size) ((void)0)
#define SIM_FIBER_ARRIVE(save, bottom, size) ((void)0)
#endif

// kernels have internal linkage, templates too: the LDS arrays inside them are then ordinary statics, which
// AddressSanitizer puts red zones around (it leaves COMDAT data, as an instantiation's statics would be, unguarded)
#define __global__ static
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
inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) { memset(p, v, bytes); return hipSuccess; }

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
extern dim3 threadIdx, blockIdx, gridDim, blockDim;
using std::max;
using std::min;

// explicit single operations: the plain operators (build with -ffp-contract=off)
inline double __dmul_rn(double a, double b) { return a * b; }
inline double __dadd_rn(double a, double b) { return a + b; }
inline float __fdiv_rn(float a, float b) { return a / b; }
inline float __fsub_rn(float a, float b) { return a - b; }
inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
inline unsigned atomicMax(unsigned* p, unsigned v) { const unsigned old = *p; if (v > old) *p = v; return old; }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    if (v > old) *p = v;
    return old;
}
inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }

constexpr unsigned kSimMaxLanes = 512;
constexpr size_t kSimStack = 128 * 1024;
struct sim_group {
    ucontext_t host, lane[kSimMaxLanes];
    unsigned lanes;                     // of the running launch: its block.x
    std::vector<char> stacks;
    const void* host_bottom;            // the calling thread's stack, as the sanitizer names it
    size_t host_size;
    bool spawned;                       // lanes 1 .. are coroutines: lane 0 has met a barrier
    unsigned finished;
    std::function<void()> body;
};
extern sim_group sim_g;

inline void sim_die(const char* what) { fprintf(stderr, "hipshim_wg: %s\n", what); abort(); }

inline void sim_lane_entry() {
    SIM_FIBER_ARRIVE(nullptr, threadIdx.x == 0 ? &sim_g.host_bottom : nullptr, threadIdx.x == 0 ? &sim_g.host_size : nullptr);
    sim_g.body();
    ++sim_g.finished;
    // on to the next lane (it waits in its last barrier); from the last lane, or from a lane 0 that met no barrier, to the host
    const unsigned me = threadIdx.x;
    if (sim_g.spawned && me + 1 < sim_g.lanes) {
        threadIdx.x = me + 1;
        SIM_FIBER_LEAVE(nullptr, sim_g.stacks.data() + kSimStack * (me + 1), kSimStack);
        setcontext(&sim_g.lane[me + 1]);
    }
    SIM_FIBER_LEAVE(nullptr, sim_g.host_bottom, sim_g.host_size);
    setcontext(&sim_g.host);
}
inline void sim_make_lane(unsigned l) {
    getcontext(&sim_g.lane[l]);
    sim_g.lane[l].uc_stack.ss_sp = sim_g.stacks.data() + kSimStack * l;
    sim_g.lane[l].uc_stack.ss_size = kSimStack;
    sim_g.lane[l].uc_link = nullptr;                        // (never taken: a lane ends with a setcontext of its own)
    makecontext(&sim_g.lane[l], sim_lane_entry, 0);
}
inline void __syncthreads() {
    const unsigned me = threadIdx.x, next = (me + 1) % sim_g.lanes;
    if (!sim_g.spawned) {
        if (me != 0) sim_die("a lane met a barrier after lane 0 had ended without one");
        for (unsigned l = 1; l < sim_g.lanes; ++l) sim_make_lane(l);
        sim_g.spawned = true;
    }
    void* fake = nullptr;
    threadIdx.x = next;
    SIM_FIBER_LEAVE(&fake, sim_g.stacks.data() + kSimStack * next, kSimStack);
    swapcontext(&sim_g.lane[me], &sim_g.lane[next]);
    SIM_FIBER_ARRIVE(fake, nullptr, nullptr);
    threadIdx.x = me;
}

inline void sim_launch(std::function<void()> body, dim3 grid, dim3 block) {
    if (block.x == 0 || block.x > kSimMaxLanes || block.x % 64 != 0 || block.y != 1 || block.z != 1)
        sim_die("a launch this shim does not run");
    if (sim_g.stacks.empty()) sim_g.stacks.resize(kSimStack * kSimMaxLanes);
    sim_g.lanes = block.x;
    sim_g.body = body;
    gridDim = grid;
    blockDim = block;
    for (unsigned bz = 0; bz < grid.z; ++bz)
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            blockIdx = dim3(bx, by, bz);
            threadIdx = dim3(0, 0, 0);
            sim_g.spawned = false;
            sim_g.finished = 0;
            sim_make_lane(0);
            void* fake = nullptr;
            SIM_FIBER_LEAVE(&fake, sim_g.stacks.data(), kSimStack);
            swapcontext(&sim_g.host, &sim_g.lane[0]);
            SIM_FIBER_ARRIVE(fake, nullptr, nullptr);
            if (!sim_g.spawned) {
                for (unsigned l = 1; l < sim_g.lanes; ++l) {
                    threadIdx.x = l;
                    body();
                    ++sim_g.finished;
                }
            }
            if (sim_g.finished != sim_g.lanes) sim_die("a lane was left behind at a barrier");
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) sim_launch([=] { kernel(__VA_ARGS__); }, grid, block)
