// forced_common.h -- what the two forced-alignment kernels share (ta_forced.hip: a lattice per line, DESIGN.md section
// 14.7; ta_forced_page.hip: one lattice through all lines of a page, section 14.8): the sizes, the choice of the variant,
// the packing of the moves, the integer emission score and the two ways a value goes from lane to lane of one wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kMaxNo = TA_TRAIN_MAX_CLASSES;
constexpr int kChunk = 8;                              // timesteps of emission scores per LDS buffer
constexpr int kWalk = 32;                              // timesteps of moves per walk block (TA_FORCED_WALK_BLOCK)
constexpr int kPf = kChunk * kMaxNo / 64;              // probabilities a lane holds for the chunk ahead
constexpr long long kNeg = -(1ll << 50);
static_assert(kWalk == TA_FORCED_WALK_BLOCK, "the header documents the walk's block");
static_assert(2 * TA_FORCED_MAX_TARGET + 1 <= 64 * 32, "the widest variant holds every state");

// states per lane for a lattice of S states
__host__ __device__ inline int forced_k(int S) { return S <= 128 ? 2 : S <= 256 ? 4 : S <= 512 ? 8 : S <= 1024 ? 16 : 32; }
// rows of 64 move words for T timesteps
__host__ __device__ inline int64_t forced_ws_rows(int T, int K) { return K == 32 ? 2 * (int64_t)T : (T + 16 / K - 1) / (16 / K); }

// the emission score of a probability in units of 2^-16 bit: no transcendental, the same integers everywhere
__host__ __device__ inline int emission_q(float p) {
    float a = p > 0x1p-17f ? p : 0x1p-17f;             // NaN, 0 and negatives: the floor
    a = a < 1.0f ? a : 1.0f;
    uint32_t u;
    __builtin_memcpy(&u, &a, 4);
    const int e = (int)(u >> 23) - 127;
    const uint32_t g = (u & 0x7FFFFFu) >> 7;
    return e * 65536 + (int)(g + ((((g * (65536u - g)) >> 16) * 22713u) >> 16));
}

// LDS written by one lane and read by another of the SAME wave: a wave's LDS operations are carried out in program order,
// so all it takes is that the compiler keeps them in that order -- no s_barrier, and above all no wait for the
// probability loads that are in flight for the next chunk (which the fence of __syncthreads() would bring)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane l takes lane l - 1's value, lane 0 takes `edge`
__device__ __forceinline__ long long from_left(long long v, long long edge) {
    const int lo = __builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(edge >> 32), (int)(v >> 32), 0x138, 0xf, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// lane l takes lane l + 1's value, lane 63 takes `edge`
__device__ __forceinline__ long long from_right(long long v, long long edge) {
    const int lo = __builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(edge >> 32), (int)(v >> 32), 0x130, 0xf, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

constexpr int variant_bit(int K) { return K == 2 ? 1 : K == 4 ? 2 : K == 8 ? 4 : K == 16 ? 8 : 16; }

}  // namespace
