// lstm_seq_common.h -- what the five recurrence kernels of the line recogniser (K3: ta_lstm.hip, ta_lstm_f64.hip)
// have in common besides their matrix part: the group's metadata, "which step of its line is step t of direction
// dir", the h0 loop, the x tile of the 16-line f32 kernels, and a compile-time loop.
//
// Device only, everything forced inline, templated on the group size G and -- where kernel arguments are read -- on
// the argument struct (LstmArgs and Seq64Args name these fields alike).  The kernels keep their own __shared__
// arrays, declared where they always were, and hand them in by reference: a helper that OWNED the three metadata
// arrays (one __shared__ struct) moved every LDS offset of the kernel and turned ds_read_b128 into pairs of
// ds_read2_b64 inside the timestep loops.
//
// What is NOT here although all five kernels have it: the read of c0 / tstart (two lines per kernel).  Every form of
// a shared helper tried for it changed a timestep loop -- the four-line f32 kernel's first step gets peeled (1 387 ->
// 1 849 instructions), the others' loops are scheduled differently -- so it stays spelled out, and with it the one
// difference that is meant: the f32 kernels read c0 whenever it is given, the f64 kernels only where tstart > 0 (a
// sequence that starts here starts from c = 0, whatever the buffer holds).  The f64 kernels also keep their own
// spelling of the step's row, for the same reason, and they and the four-line f32 kernel their own h0 loop, which
// through load_h0 compiles to other code in front of the timestep loop (profiles/lstm_refactor.txt has the figures).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ta_seq {

constexpr int kNi = 48;            // input rows (normalised line height)
constexpr int kNs = 100;           // LSTM states per direction
constexpr int kXK = 52;            // the x part of a step's input: [1, x(48), 3 zero pads]

// A kernel's group metadata: references to its own three __shared__ arrays, one entry per line slot.
template <int G>
struct GroupView {
    int (&line)[G];                // line id, -1 = empty slot
    int (&T)[G];                   // timesteps (0 for an empty slot)
    long long (&row)[G];           // first row
};
// threads 0 .. G - 1 fill the arrays; the caller's barrier publishes them
template <int G, class Args>
__device__ __forceinline__ void group_load(const GroupView<G>& g, const Args& a, int grp, int tid) {
    if (tid < G) {
        const int id = a.group_lines[grp * G + tid];
        g.line[tid] = id;
        g.T[tid] = id >= 0 ? a.T[id] : 0;
        g.row[tid] = id >= 0 ? a.row_off[id] : 0;
    }
}
template <int G>
__device__ __forceinline__ int group_tmax(const GroupView<G>& g) {
    int Tmax = 0;
#pragma unroll
    for (int s = 0; s < G; ++s) Tmax = max(Tmax, g.T[s]);
    return Tmax;
}

// The timestep of a line of T > 0 steps that step t of the group's loop works on: a line shorter than the group's
// longest stays on its last step (what it computes there is never stored), and the reverse direction runs on
// xs[::-1] (Reversed(LSTM)).  The row of that step is the line's first row + this.
__device__ __forceinline__ int step_index(int dir, int t, int T) {
    const int tt = t < T ? t : T - 1;
    return dir ? T - 1 - tt : tt;
}

// h_{-1} of continued sequences: every (slot, unit) of the group's lines goes to the kernel's own store(slot, unit, h)
template <int G, class H, class Store>
__device__ __forceinline__ void load_h0(const GroupView<G>& g, const H* h0, int dir, int tid, int nthreads, Store store) {
    if (h0) {
        for (int e = tid; e < G * kNs; e += nthreads) {
            const int slot = e / kNs, u = e % kNs;
            const int id = g.line[slot];
            if (id >= 0) store(slot, u, h0[((size_t)id * 2 + dir) * kNs + u]);
        }
    }
}

// element e of the [G][52] x tile of step t, row = [1, x_t, 0, 0, 0] of the slot's line (zeros for an empty slot)
template <int G>
__device__ __forceinline__ float x_tile_value(const GroupView<G>& g, const float* x, int dir, int e, int t) {
    const int slot = e / kXK, kp = e % kXK;
    if (kp == 0) return 1.0f;
    if (kp > kNi) return 0.0f;
    const int Tl = g.T[slot];
    if (Tl <= 0) return 0.0f;
    const int tt = step_index(dir, t, Tl);
    return x[(g.row[slot] + tt) * kNi + (kp - 1)];
}

// f(IntTag<B>{}), f(IntTag<B + 1>{}), ... f(IntTag<E - 1>{}): a loop whose index is a compile-time constant in the
// body (decltype(i)::value), for what an instruction wants as an immediate
template <int I> struct IntTag { static constexpr int value = I; };
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(IntTag<B>{});
        static_for<B + 1, E>(f);
    }
}

}  // namespace ta_seq
