// forced_common.h -- the building blocks of the eight forced-alignment kernel files (DESIGN.md sections 14.7 .. 14.15):
// ta_forced.hip (a lattice per line), ta_forced_page.hip (one lattice through all lines of a page), ta_forced_omit.hip (a
// path that may omit characters), ta_forced_page_omit.hip (both), ta_forced_conf.hip (max-marginals),
// ta_forced_post.hip (sum-product posteriors), ta_forced_page_conf.hip (max-marginals on the page's lattice) and
// ta_forced_page_post.hip (sum-product posteriors on the page's lattice).
//   sizes     kChunk, kWalk, kPf, kNeg; forced_k, forced_ws_rows, omit_bit_rows, variant_bit, walk_rows
//   score     emission_q
//   lanes     wave_lds_sync, from_left, from_right; dpp_or_self, max64, wave_max_scan (the two kernels with omission)
//   checks    line_ok (a line's own numbers), labels_ok, queries_ok, slot_filled / slot_line (the kSlots kernels)
//   set-up    lane_labels (lab[], skip, skipf of a lane, for a line or a window of a page)
//   feed      Feed: prefetch a chunk's probabilities into registers, publish them as scores in the LDS buffer in turn
//   step      forced_step (stay / advance / skip for a lane's K states, with the moves it took); ta_forced.hip and the
//             forward fill of ta_forced_conf.hip spell it out
//   moves     store_moves, stage_moves (forced_page_common.h's page_walk spells it out), staged_move, peak_frame
//   omission  omit_seed, omit_step (ta_forced_omit.hip spells both out), store_bits, omit_end, far_source: the two kernels
//             with omission, ta_forced_omit.hip and ta_forced_page_omit.hip
//   host      forced_preamble, forced_ws_guard, forced_ws_small, forced_check_lines, forced_check_chunk, variants_up_to,
//             forced_check_slots, forced_launch_variants
// forced_two_fill.h, on top of this header, holds what ta_forced_conf.hip and ta_forced_post.hip alone share: their
// arguments, their kernels' prologue and the control structure of their two fills; forced_post_cells.h, on top of that, the
// sum-product arithmetic ta_forced_post.hip and ta_forced_page_post.hip share; forced_page_common.h what
// ta_forced_page.hip and ta_forced_page_omit.hip alone share: arguments, limits, prologue, the fill's control structure,
// walk, peaks and the host's checks of a page list.
// A piece is shared in a kernel only where the kernel's instruction stream allows it ("Shared
// pieces of the forced-alignment kernels"; profiles/forced_refactor.txt, profiles/forced_two_fill.txt,
// profiles/forced_page_shared.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

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
// rows of 64 bit words for T timesteps (the kernels with omission: a bit per state and timestep)
__host__ __device__ inline int64_t omit_bit_rows(int T, int K) { return (T + 32 / K - 1) / (32 / K); }
// steps per move word, and the move rows of a walk block
constexpr int steps_per_word(int K) { return K == 32 ? 1 : 16 / K; }
constexpr int walk_rows(int K) { return K == 32 ? 2 * kWalk : kWalk / steps_per_word(K); }

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

// one DPP move of an int64: a lane the control gives no source (or whose row the mask leaves out) keeps its own value
template <int kCtrl, int kRowMask>
__device__ __forceinline__ long long dpp_or_self(long long v) {
    const int lo = __builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, kRowMask, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(v >> 32), (int)(v >> 32), kCtrl, kRowMask, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

// inclusive max-scan over the 64 lanes: Hillis-Steele inside a row of 16, then the rows' last lanes broadcast
__device__ __forceinline__ long long wave_max_scan(long long v) {
    v = max64(v, dpp_or_self<0x111, 0xf>(v));          // row_shr:1
    v = max64(v, dpp_or_self<0x112, 0xf>(v));          // row_shr:2
    v = max64(v, dpp_or_self<0x114, 0xf>(v));          // row_shr:4
    v = max64(v, dpp_or_self<0x118, 0xf>(v));          // row_shr:8
    v = max64(v, dpp_or_self<0x142, 0xa>(v));          // row_bcast:15 into rows 1 and 3
    v = max64(v, dpp_or_self<0x143, 0xc>(v));          // row_bcast:31 into rows 2 and 3
    return v;
}

constexpr int variant_bit(int K) { return K == 2 ? 1 : K == 4 ? 2 : K == 8 ? 4 : K == 16 ? 8 : 16; }

// ---- checks on a line's own device numbers ---------------------------------------------------------------------------------

// every bound a per-line kernel relies on (the host checked its copies as well).  a: the entry's arguments (no, rows,
// nlabels, ws_bytes, variants); r0, l0, w0: the line's first row, first label and workspace offset; need(): the bytes of its
// piece, asked only once T and L are known to be in range
template <class Args, class Need>
__device__ __forceinline__ bool line_ok(const Args& a, int T, int L, int64_t r0, int64_t l0, int64_t w0, Need need) {
    return a.no >= 2 && a.no <= kMaxNo && T >= 1 && T <= TA_TRAIN_MAX_T && L >= 1 && L <= TA_FORCED_MAX_TARGET &&
           2 * L + 1 <= T && r0 >= 0 && r0 + T <= a.rows && l0 >= 0 && l0 + L <= a.nlabels && w0 >= 0 &&
           (w0 & 15) == 0 && w0 + need() <= a.ws_bytes && (a.variants & variant_bit(forced_k(2 * L + 1))) != 0;
}

// every label a class that is no blank
__device__ __forceinline__ bool labels_ok(const int32_t* cs, int n, int no, int lane) {
    bool bad = false;
    for (int i = lane; i < n; i += 64) bad |= cs[i] < 1 || cs[i] >= no;
    return !__any(bad);
}

// every query a frame of the line, none before the one in front of it; the queries lie kStride words apart
template <int kStride>
__device__ __forceinline__ bool queries_ok(const int32_t* tq, int L, int T, int lane) {
    bool bad = false;
    for (int i = lane; i < L; i += 64) {
        const int t = tq[(int64_t)i * kStride];
        bad |= t < 0 || t >= T || (i >= 1 && t < tq[(int64_t)(i - 1) * kStride]);
    }
    return !__any(bad);
}

// the kSlots kernels: block b is a packed slot.  A slot behind count[0] -- or any slot of a call whose count[0] is negative --
// is not filled; a filled slot's line is acc_line[b], -1 where that is none of the chunk's lines
__device__ __forceinline__ bool slot_filled(const int64_t* count, int b) {
    const int64_t filled = count[0];
    return filled >= 0 && b < filled;
}
__device__ __forceinline__ int slot_line(const int32_t* acc_line, int nlines_all, int b) {
    const int q = __builtin_amdgcn_readfirstlane(acc_line[b]);
    return q >= 0 && q < nlines_all ? q : -1;
}

// ---- a lane's labels -------------------------------------------------------------------------------------------------------

// The K / 2 labels of lane `lane` among the characters [first, end) of the text cs (a line: 0 and L; a page's window: lo
// and hi), 0 behind the end.  Returns skip, bit j: label j may be reached over the blank in front of it; *skipf (where
// asked for), bit j: from label j the blank behind it may be skipped.
template <int H>
__device__ __forceinline__ unsigned lane_labels(const int32_t* cs, int first, int end, int lane, int (&lab)[H],
                                                unsigned* skipf = nullptr) {
    unsigned skip = 0, back = 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const int i = first + lane * H + j;
        lab[j] = i < end ? cs[i] : 0;
        if (i >= 1 && i < end && cs[i] != cs[i - 1]) skip |= 1u << j;
        if (skipf && i + 1 < end && cs[i + 1] != cs[i]) back |= 1u << j;
    }
    if (skipf) *skipf = back;
    return skip;
}

// ---- the emission feed -----------------------------------------------------------------------------------------------------

// The probability rows of kChunk timesteps are loaded a chunk ahead into registers (prefetch), turned into scores once per
// (timestep, class) and published in one of the two LDS buffers of `tab`, taken in turn; the reader hands over with
// wave_lds_sync().  V and `emit`: int and emission_q, or the posterior's float and emission_f.
template <class V>
struct Feed {
    V* tab;
    int no, lane;
    float pf[kPf];
    __device__ __forceinline__ Feed(V* tab_, int no_, int lane_) : tab(tab_), no(no_), lane(lane_) {}
    // chunk c of a line's T rows at P; zeros for a chunk that does not exist
    __device__ __forceinline__ void prefetch(const float* P, int T, int c) {
        const int t0 = c * kChunk;
        const int cnt = c < 0 ? 0 : (T - t0 < kChunk ? T - t0 : kChunk) * no;     // <= 0 behind the last chunk
        const float* src = P + (int64_t)t0 * no;
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            const int idx = j * 64 + lane;
            pf[j] = idx < cnt ? src[idx] : 0.0f;
        }
    }
    // pf -> the buffer of the g-th chunk
    template <class Emit>
    __device__ __forceinline__ V* publish(int g, Emit emit) {
        V* buf = tab + (g & 1) * (kChunk * kMaxNo);
#pragma unroll
        for (int j = 0; j < kPf; ++j) buf[j * 64 + lane] = emit(pf[j]);
        return buf;
    }
};

// ---- the step --------------------------------------------------------------------------------------------------------------

// One frame of the lattice for a lane's K states: a state takes the best of stay / advance / skip (ties in that order) and
// adds its emission score; `left` is the left lane's last value.  Returns two move bits per state.  kFirst: the first
// frame of a line behind a page's first, in which a label state has no stay candidate.
template <int K, bool kFirst>
__device__ __forceinline__ unsigned long long forced_step(long long (&v)[K], long long left, unsigned skip,
                                                          const int (&lab)[K / 2], const int* q, int qb) {
    unsigned long long mv = 0;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {                 // downwards: v[k - 1] and v[k - 2] are still the old frame's
        long long best = (kFirst && (k & 1)) ? kNeg : v[k];
        unsigned m = 0;
        const long long adv = k >= 1 ? v[k - 1] : left;
        if (adv > best) { best = adv; m = 1; }
        if (k & 1) {
            const long long sk = k >= 2 ? v[k - 2] : left;
            if (((skip >> (k >> 1)) & 1u) && sk > best) { best = sk; m = 2; }
            v[k] = best + q[lab[k >> 1]];
        } else {
            v[k] = best + qb;
        }
        mv |= (unsigned long long)m << (2 * k);
    }
    return mv;
}

// ---- the moves: stored by the fill, staged and decoded by the walk ---------------------------------------------------------

// step t's move word of a lane into the line's rows of 64 words: 16 / K steps per 32-bit word (acc gathers them), K = 32
// two words per step
template <int K>
__device__ __forceinline__ void store_moves(uint32_t* moves, int t, int T, int lane, unsigned long long mv, uint32_t& acc) {
    constexpr int SPW = steps_per_word(K);
    if (K == 32) {
        moves[(int64_t)(2 * t) * 64 + lane] = (uint32_t)mv;
        moves[(int64_t)(2 * t + 1) * 64 + lane] = (uint32_t)(mv >> 32);
    } else {
        acc |= (uint32_t)mv << ((2 * K * (t % SPW)) & 31);
        if (t % SPW == SPW - 1 || t == T - 1) {
            moves[(int64_t)(t / SPW) * 64 + lane] = acc;
            acc = 0;
        }
    }
}

// the move rows of the walk block that starts at timestep `base` into LDS, coalesced; between two __syncthreads()
template <int K>
__device__ __forceinline__ void stage_moves(uint32_t* stage, const uint32_t* moves, int base, int64_t nrows, int lane) {
    const int64_t g0 = K == 32 ? 2 * (int64_t)base : base / steps_per_word(K);
    for (int r = 0; r < walk_rows(K) && g0 + r < nrows; ++r) stage[r * 64 + lane] = moves[(g0 + r) * 64 + lane];
}

// the move of state k of lane l at step tt of the staged block
template <int K>
__device__ __forceinline__ unsigned staged_move(const uint32_t* stage, int tt, int l, int k) {
    constexpr int SPW = steps_per_word(K);
    if (K == 32) return (stage[(2 * tt + (k >> 4)) * 64 + l] >> (2 * (k & 15))) & 3u;
    return (stage[(tt / SPW) * 64 + l] >> (2 * K * (tt % SPW) + 2 * k)) & 3u;
}

// the first frame of tf .. tl at which class c has its largest q
__device__ __forceinline__ int peak_frame(const float* P, int no, int c, int tf, int tl) {
    int bt = tf, bq = INT32_MIN;
    for (int t = tf; t <= tl; ++t) {
        const int qv = emission_q(P[(int64_t)t * no + c]);
        if (qv > bq) { bq = qv; bt = t; }
    }
    return bt;
}

// ---- omission: what ta_forced_omit.hip and ta_forced_page_omit.hip share ---------------------------------------------------
// a[x] = v[x] + omit * ceil(x / 2), Pm[x] = max(a[0 .. x]); pen0 = omit * (the lane's first character), so that state k of a
// lane has a = v[k] + pen0 + omit * ((k + 1) >> 1).  A page forms all of it in WINDOW coordinates.

// frame 0 where every state may start the path: the characters in front are paid for
// (ta_forced_omit.hip spells it out: as a call its K = 32 kernel takes 51 AGPRs for 28)
template <int K>
__device__ __forceinline__ void omit_seed(long long (&v)[K], const int (&lab)[K / 2], const int* q, int qb, long long omit,
                                          long long pen0) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (long long)((k & 1) ? q[lab[k >> 1]] : qb) - (pen0 + omit * (k >> 1));
}

// One frame for a lane's K states, upwards (o1 and o2 carry the old row's v[k - 1] and v[k - 2]): stay / advance / skip /
// far, ties in that order; move code 3 = far.  It scans a[] and notes in `bits` which states set a new prefix maximum.
// kFirst, the first frame of a line behind a page's first, takes the far candidates from pbuf instead, the OLD window's
// prefix maxima (d: old window states in front of the new window), and gives a label state no stay candidate.
// ta_forced_omit.hip spells the kFirst = false form out: as a call its K = 16 and K = 32 kernels spill scalars and K = 32
// works out of twice the AGPRs.
template <int K, bool kFirst>
__device__ __forceinline__ unsigned long long omit_step(long long (&v)[K], long long left, unsigned skip,
                                                        const int (&lab)[K / 2], const int* q, int qb, long long omit,
                                                        long long pen0, int lane, const long long* pbuf, int d,
                                                        uint32_t& bits) {
    unsigned long long mv = 0;
    long long run = kNeg, pm_even = kNeg;
    if (!kFirst) {
        long long but_last = kNeg;
#pragma unroll
        for (int k = 0; k < K - 1; ++k) but_last = max64(but_last, v[k] + pen0 + omit * ((k + 1) >> 1));
        const long long total = max64(but_last, v[K - 1] + pen0 + omit * (K >> 1));
        run = from_left(wave_max_scan(total), kNeg);                       // Pm of the state in front of the lane
        pm_even = from_left(max64(run, but_last), kNeg);                   // Pm[2 i - 2] of the lane's first character
    }
    long long o1 = left, o2 = kNeg, far = kNeg;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const long long old = v[k];
        if (!kFirst) {
            const long long ak = old + pen0 + omit * ((k + 1) >> 1);
            if (ak >= run) bits |= 1u << k;
            run = max64(run, ak);
            if (!(k & 1)) {
                far = pm_even - (pen0 + omit * (k >> 1));                  // lane 0's first character: kNeg, never taken
                pm_even = run;
            }
        } else if (!(k & 1)) {
            const int x = lane * K + k + d - 2;                            // 2 i - 2 in the old window
            const long long pm = x < 0 ? kNeg : pbuf[x < 64 * K ? x : 64 * K - 1];
            far = pm - (pen0 + omit * ((k >> 1) + (d >> 1)));
        }
        long long best = (kFirst && (k & 1)) ? kNeg : old;
        unsigned m = 0;
        if (o1 > best) { best = o1; m = 1; }
        if ((k & 1) && ((skip >> (k >> 1)) & 1u) && o2 > best) { best = o2; m = 2; }
        if (far > best) { best = far; m = 3; }
        v[k] = best + ((k & 1) ? q[lab[k >> 1]] : qb);
        mv |= (unsigned long long)m << (2 * k);
        o2 = o1;
        o1 = old;
    }
    return mv;
}

// step t's bits of a lane into the line's rows of 64 bit words: 32 / K steps per word (accb gathers them)
template <int K>
__device__ __forceinline__ void store_bits(uint32_t* bitrows, int t, int T, int lane, uint32_t bits, uint32_t& accb) {
    constexpr int SPB = 32 / K;
    accb |= bits << ((K * (t % SPB)) & 31);
    if (t % SPB == SPB - 1 || t == T - 1) {
        bitrows[(int64_t)(t / SPB) * 64 + lane] = accb;
        accb = 0;
    }
}

// The end rule: fin[s] = v[s] - omit * (n - ceil(s / 2)) over the states s <= 2 n, s = off + the lane's K r; the largest,
// the largest s on a tie.  Every lane's best goes through LDS and every lane reads all 64.  Returns s, -1 where there is
// none; the fence in between also lets the walk read what the fill stored.
template <int K>
__device__ __forceinline__ int omit_end(const long long (&v)[K], long long omit, int off, int n, int lane, long long* fin_v,
                                        int* fin_s, long long* best) {
    long long bv = kNeg * 2;
    int bs = -1;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = off + lane * K + r;
        const long long f = v[r] - omit * (long long)(n - ((s + 1) >> 1));
        if (s <= 2 * n && f >= bv) { bv = f; bs = s; }
    }
    fin_v[lane] = bv;
    fin_s[lane] = bs;
    __threadfence();                                   // the moves, the bits and the -1 frames are read back by other lanes
    __syncthreads();
    *best = kNeg * 2;
    int s = -1;
    for (int l = 0; l < 64; ++l) {
        const long long f = fin_v[l];
        if (fin_s[l] >= 0 && f >= *best) { *best = f; s = fin_s[l]; }
    }
    return s;
}

// the far move's source: the first set bit at or below state x of the staged bit row (tt: the frame in the block), -1
// where there is none; x lies in 0 .. 64 K - 1
template <int K>
__device__ __forceinline__ int far_source(const uint32_t* bitstage, int tt, int x, int lane) {
    constexpr int SPB = 32 / K;
    const int lx = x / K, kx = x % K, sh = (K * (tt % SPB)) & 31;
    const uint32_t* row = bitstage + (tt / SPB) * 64;
    uint32_t w = (row[lane] >> sh) & (uint32_t)((1ull << K) - 1);
    if (lane > lx) w = 0;
    if (lane == lx) w &= (uint32_t)((2ull << kx) - 1);
    const unsigned long long has = __ballot(w != 0);
    if (has == 0) return -1;                           // cannot happen: the first state's bit is always set
    const int lt = 63 - __builtin_clzll(has);
    uint32_t wt = (row[lt] >> sh) & (uint32_t)((1ull << K) - 1);
    if (lt == lx) wt &= (uint32_t)((2ull << kx) - 1);
    return lt * K + 31 - __builtin_clz(wt);
}

// ---- host: what the entries check before a launch --------------------------------------------------------------------------

// What every entry refuses first, in this order: a negative size, `no` outside its range, what the entry alone refuses
// (`own`: its message, or nullptr), then -- unless there is nothing to do (`empty`) -- a null pointer and a workspace off its
// 16 bytes.  *go: the entry goes on; otherwise it returns what this returns.
inline int forced_preamble(bool negative, int no, const char* own, bool empty, bool null, const void* workspace, bool* go) {
    *go = false;
    if (negative) return ta_fail(TA_EINVAL, "negative size");
    if (no < 2 || no > kMaxNo) return ta_fail(TA_EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES");
    if (own) return ta_fail(TA_EINVAL, own);
    if (empty) return TA_OK;
    if (null) return ta_fail(TA_EINVAL, "null pointer argument");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return ta_fail(TA_EINVAL, "workspace not 16-byte aligned");
    *go = true;
    return TA_OK;
}

// the (T, L) for which a *_workspace_bytes function has an answer
inline bool forced_ws_guard(int32_t T, int32_t L) {
    return !(T < 1 || T > TA_TRAIN_MAX_T || L < 1 || L > TA_FORCED_MAX_TARGET || 2 * (int64_t)L + 1 > T);
}

// the refusal of a workspace below what ws_name, the exported function, says the lines (or pages) need
inline int forced_ws_small(const char* lines, const char* ws_name) {
    char msg[128];
    snprintf(msg, sizeof(msg), "workspace smaller than the %s' %s", lines, ws_name);
    return ta_fail(TA_EINVAL, msg);
}

// the host's copies of a line list: every line inside the limits, the lines inside rows, nlabels and the workspace, whose
// pieces are ws_bytes(T, L) (ws_name: the exported function that tells a caller so).  *variants: a bit per K to launch.
template <class WsBytes>
inline int forced_check_lines(const int32_t* T_host, const int32_t* L_host, int nlines, int64_t rows, int64_t nlabels,
                              int64_t workspace_bytes, WsBytes ws_bytes, const char* ws_name, int* variants) {
    int64_t need = 0, sum_t = 0, sum_l = 0;
    *variants = 0;
    for (int b = 0; b < nlines; ++b) {
        const int t = T_host[b], l = L_host[b];
        if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
        if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
        if (l < 1) return ta_fail(TA_EINVAL, "a line without text");
        if (l > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a text has more than TA_FORCED_MAX_TARGET characters");
        if (2 * (int64_t)l + 1 > t) return ta_fail(TA_EINVAL, "a text's 2 L + 1 states exceed its line's timesteps");
        need += ws_bytes(t, l);
        *variants |= variant_bit(forced_k(2 * l + 1));
        sum_t += t;
        sum_l += l;
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (sum_l > nlabels) return ta_fail(TA_EINVAL, "the lines' texts exceed nlabels");
    if (workspace_bytes < need) return forced_ws_small("lines", ws_name);
    return TA_OK;
}

// the host's copies of a chunk's lines, each with the cap on the text it may receive: every line inside the limits and the
// lines inside rows.  *need: the sum of ws_bytes(T, cap) over the lines that can receive text; *capmax: their largest cap,
// 0 where no line can take a slot
template <class WsBytes>
inline int forced_check_chunk(const int32_t* T_all_host, const int32_t* Lcap_host, int nlines_all, int64_t rows,
                              WsBytes ws_bytes, int64_t* need, int* capmax) {
    int64_t sum_t = 0;
    *need = 0;
    *capmax = 0;
    for (int q = 0; q < nlines_all; ++q) {
        const int t = T_all_host[q], cap = Lcap_host[q];
        if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
        if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
        if (cap < 0) return ta_fail(TA_EINVAL, "a negative cap");
        if (cap > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a cap above TA_FORCED_MAX_TARGET characters");
        sum_t += t;
        if (cap == 0) continue;                        // a line that can receive no text: no piece, no variant
        if (2 * (int64_t)cap + 1 > t) return ta_fail(TA_EINVAL, "a cap's 2 L + 1 states exceed its line's timesteps");
        *need += ws_bytes(t, cap);
        *capmax = cap > *capmax ? cap : *capmax;
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    return TA_OK;
}

// a text within its cap may need any variant up to the cap's
inline int variants_up_to(int kmax) {
    int variants = 0;
    for (int k = 2; k <= kmax; k *= 2) variants |= variant_bit(k);
    return variants;
}

// The host's part of a kSlots entry whose workspace is sized by the labels (ta_forced_confidence_lines,
// ta_forced_posterior_lines): forced_check_chunk's refusals, then the workspace rule -- ws_bytes(label_cap, largest cap),
// the exported function ws_name.  *kmax: the widest variant to launch, 0 where no line can take a slot (nothing to launch).
template <class WsBytes>
inline int forced_check_slots(const int32_t* T_all_host, const int32_t* Lcap_host, int nlines_all, int64_t rows,
                              int64_t label_cap, int64_t workspace_bytes, WsBytes ws_bytes, const char* ws_name, int* kmax) {
    int64_t pieces;                                    // none per line
    int capmax;
    *kmax = 0;
    const int rc = forced_check_chunk(T_all_host, Lcap_host, nlines_all, rows, [](int, int) { return 0; }, &pieces, &capmax);
    if (rc != TA_OK) return rc;
    const int64_t need = ws_bytes(label_cap, capmax);
    if (need < 0) return ta_fail(TA_ELIMIT, "label_cap beyond what a workspace can be sized for");
    if (workspace_bytes < need) {
        char msg[128];
        snprintf(msg, sizeof(msg), "workspace smaller than %s", ws_name);
        return ta_fail(TA_EINVAL, msg);
    }
    if (capmax > 0) *kmax = forced_k(2 * capmax + 1);
    return TA_OK;
}

// One launch per variant that `variants` calls for, K = 2 .. 32 in turn; launch(kc) launches the kernel of
// K = decltype(kc)::value over all blocks.
template <class Launch>
hipError_t forced_launch_variants(int variants, Launch launch) {
    hipError_t e = hipSuccess;
    auto one = [&](auto kc) {
        if (e != hipSuccess || !(variants & variant_bit(decltype(kc)::value))) return;
        launch(kc);
        e = hipGetLastError();
    };
    one(std::integral_constant<int, 2>());
    one(std::integral_constant<int, 4>());
    one(std::integral_constant<int, 8>());
    one(std::integral_constant<int, 16>());
    one(std::integral_constant<int, 32>());
    return e;
}

}  // namespace
