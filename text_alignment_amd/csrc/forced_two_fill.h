// forced_two_fill.h -- what ta_forced_conf.hip (max-marginals) and ta_forced_post.hip (sum-product posteriors) have in
// common: ONE wave runs a forward and a backward fill over a line's lattice and combines the two at the query frame of every
// character (DESIGN.md sections 14.10 and 14.11; "Shared pieces of the forced-alignment kernels" in 14.7).  Stated once here:
//   TwoFillArgs          the arguments both kernels take, a line list from the host or packed slots on the device
//   two_fill_prologue    a block's way to its line: slot handling, the checks on the line's own numbers, the statuses
//   two_fill_best        the LDS reduction of a combine, 64 candidates -> 8 -> 1
//   two_fill<K, kStride, R>   the control structure of the two fills: chunk parity of the two LDS buffers, the query cursor
//                        in both directions, where the backward fill starts and stops
// R, a struct of static members per file, is the arithmetic: the types V (a state's value), E (an emission in LDS), Line
// (TwoFillLine and the line's outputs) and Red (the LDS of a combine); kRowBytes, the bytes of a forward row per state of
// a lane (64 lanes' values); zero, one, emit, first (a state's value in frame 0 from its emission) and left (the left lane's
// value); chunk_begin (once per chunk, before its frames), forward and backward (a frame for a lane's K states; backward
// fetches its own two right-lane values); store_row, forward_done (after the forward fill) and combine, whose reduction is
// two_fill_best over R's Cand, put, get and better.  The cells stay in R: routed through forced_step or a generic join
// they cost registers and change the max-plus values below kNeg (profiles/forced_two_fill.txt).
#pragma once
#include "forced_common.h"

namespace {

struct TwoFillArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off; const int32_t* t_query;
    int32_t nlines, no, variants; int64_t rows, nlabels;     // variants: a bit per K that this call launches
    unsigned char* ws; int64_t ws_bytes;
    int32_t* status;
    // the kSlots entries alone: block k is a packed slot, its line acc_line[k] of the chunk's nlines_all lines (row_off, T
    // and Lcap per CHUNK line; labels, lab_off, L per slot), count[0] the slots that are filled, align_status what
    // ta_forced_align_lines gave the slot, frames where it left the slot's t_peak; kmax the widest variant launched
    const int32_t* acc_line; const int64_t* count; const int32_t* Lcap; const int32_t* align_status; const int32_t* frames;
    int32_t nlines_all, kmax;
};

struct TwoFillLine {
    const float* P;            // the line's first probability row
    const int32_t* cs;         // its labels
    const int32_t* tq;         // its query frames, kStride words apart
    unsigned char* fwd;        // its piece of the workspace: row i = the forward fill at tq[i]
    int T, L, no;
};

// the piece of the workspace for a line of L characters, a forward row per character; and what a kSlots entry needs for
// label_cap labels in lines of at most Lcap_max characters: every slot's piece lies (row bytes of the widest variant) x
// lab_off in, which no other slot's piece reaches since the slots' labels do not overlap
template <class R>
__host__ __device__ inline int64_t two_fill_ws_bytes(int L) { return R::kRowBytes * (int64_t)forced_k(2 * L + 1) * L; }
template <class R>
inline int64_t two_fill_slots_ws_bytes(int64_t label_cap, int32_t Lcap_max) {
    if (label_cap < 0 || label_cap > INT64_MAX / (R::kRowBytes * 32) || Lcap_max < 0 || Lcap_max > TA_FORCED_MAX_TARGET) return -1;
    if (Lcap_max == 0) return 0;
    return R::kRowBytes * (int64_t)forced_k(2 * Lcap_max + 1) * label_cap;
}

// Block b's line, or false where the block has nothing (more) to do.  One launch per variant the host's copies call for,
// each over all lines, as forced_align_kernel: a line belongs to the launch of ITS K (from the device's L) and the others
// leave at once; a line that fails the checks, or whose K no launch of this call covers, is refused by every launch alike.
// kSlots: the blocks are the packed slots ta_harvest_pack left on the device, behind ta_forced_align_lines.  A slot behind
// count[0] -- or any slot of a call whose count[0] is negative -- leaves before it has read or written anything else; a filled
// slot the aligner did not give TA_FORCED_OK is skipped under a status of its own and nothing of it is read; any other
// finds its line through acc_line, is held to that line's cap on top of the checks below and takes its queries from its
// own rows of frames (t_peak, TA_FORCED_FIELDS words apart).  *first_label: where the line's rows of the per-label outputs begin.
// All of this is over before two_fill's registers are live.
template <int K, bool kSlots, class R>
__device__ __forceinline__ bool two_fill_prologue(const TwoFillArgs& a, int b, int lane, TwoFillLine* ln, int64_t* first_label) {
    auto refuse = [&](int status) {
        if (lane == 0) a.status[b] = status;
        return false;
    };
    int q = b;                                         // the line whose rows and timesteps block b takes
    if (kSlots) {
        if (!slot_filled(a.count, b)) return false;
        if (__builtin_amdgcn_readfirstlane(a.align_status[b]) != TA_FORCED_OK) return refuse(TA_FORCED_SKIPPED);
        q = slot_line(a.acc_line, a.nlines_all, b);
        if (q < 0) return refuse(TA_FORCED_BOUNDS);
    }
    const int T = __builtin_amdgcn_readfirstlane(a.T[q]), L = __builtin_amdgcn_readfirstlane(a.L[b]);
    const int64_t r0 = a.row_off[q], l0 = a.lab_off[b];
    // beyond what the host chose the variants for
    if (kSlots && L > __builtin_amdgcn_readfirstlane(a.Lcap[q])) return refuse(TA_FORCED_BOUNDS);
    // (slots: the product stays far inside 64 bits once l0 is known to lie inside the labels)
    const int64_t w0 = !kSlots ? a.ws_off[b] : l0 >= 0 && l0 <= a.nlabels ? R::kRowBytes * (int64_t)a.kmax * l0 : -1;
    if (!line_ok(a, T, L, r0, l0, w0, [&] { return two_fill_ws_bytes<R>(L); })) return refuse(TA_FORCED_BOUNDS);
    if (forced_k(2 * L + 1) != K) return false;        // wave-uniform
    const int32_t* cs = a.labels + l0;
    const int32_t* tq = kSlots ? a.frames + TA_FORCED_FIELDS * l0 + 2 : a.t_query + l0;
    if (!labels_ok(cs, L, a.no, lane)) return refuse(TA_FORCED_LABEL);
    if (!queries_ok<kSlots ? TA_FORCED_FIELDS : 1>(tq, L, T, lane)) return refuse(TA_FORCED_QUERY);
    *ln = TwoFillLine{a.probs + r0 * a.no, cs, tq, a.ws + w0, T, L, a.no};
    *first_label = l0;
    return true;
}

// The best of the 64 lanes' candidates, in R's order (R::better(a, b): a goes before b), through the first 72 entries of
// the combine's LDS: 64 -> 8 -> 1.  Lane 0's result is the wave's; the caller hands `red` on with a wave_lds_sync().
template <class R>
__device__ __forceinline__ typename R::Cand two_fill_best(typename R::Red* red, int lane, typename R::Cand mine) {
    using Cand = typename R::Cand;
    auto best_of_8 = [&](int at) {
        Cand m = R::get(red, at);
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const Cand c = R::get(red, at + j);
            if (R::better(c, m)) m = c;
        }
        return m;
    };
    R::put(red, lane, mine);
    wave_lds_sync();
    if (lane < 8) R::put(red, 64 + lane, best_of_8(8 * lane));
    wave_lds_sync();
    return lane == 0 ? best_of_8(64) : mine;
}

// The two fills of one line, lane l holding the K consecutive states l K .. l K + K - 1 as V registers (the layout of
// forced_common.h).  Neither fill stores moves, and there is no barrier in a fill (wave_lds_sync).
//   forward   frame 0 seeds states 0 and 1; from then on only the left lane's last value crosses a lane boundary.  The row
//             of every query frame is kept (store_row), row i for character i: queries do not decrease, so one cursor
//             meets them in order, and equal neighbouring queries store the same row twice.
//   backward  starts from `one` in the last two states and walks from the last chunk of emissions to the first: the
//             emission of frame t takes the fill from t to t - 1, so frame 0's emission is never applied.  At a query
//             frame the character's forward row comes back (combine): L times per line, not T times.
// Chunk c's emissions lie in LDS buffer c & 1 in both directions, published from the registers the chunk before (behind,
// in the backward fill) was prefetched into.
template <int K, int kStride, class R>
__device__ __forceinline__ void two_fill(const typename R::Line& ln, int lane, typename R::E* tab, typename R::Red* red) {
    using V = typename R::V;
    using E = typename R::E;
    const int T = ln.T, L = ln.L, no = ln.no, S = 2 * L + 1;
    int lab[K / 2];                                    // labels per lane
    unsigned skipf;
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab, &skipf);
    V v[K];
    Feed<E> feed(tab, no, lane);
    const int nchunks = (T + kChunk - 1) / kChunk;

    // ---- forward fill; the row of every query frame is kept -------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = R::zero();
    auto query = [&](int i) { return i >= 0 && i < L ? __builtin_amdgcn_readfirstlane(ln.tq[(int64_t)i * kStride]) : -1; };
    int cur = 0, want = query(0);                      // wave-uniform: the next character whose query is still ahead
    feed.prefetch(ln.P, T, 0);
    for (int c = 0; c < nchunks; ++c) {
        const E* buf = feed.publish(c, R::emit);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        R::chunk_begin(v);
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const E* q = buf + (t - t0) * no;
            if (t == 0) {
                if (lane == 0) { v[0] = R::first(q[0]); v[1] = R::first(q[lab[0]]); }
            } else {
                R::forward(v, R::left(v[K - 1]), skip, lab, q);
            }
            while (want == t) {
                R::store_row(ln, cur, lane, v);
                ++cur;
                want = query(cur);
            }
        }
    }
    R::forward_done(ln, lane, S, v, red);

    // ---- backward fill, and the combine at every query frame -----------------------------------------------------------
    cur = L - 1;
    want = query(cur);
    auto combine_at = [&](int frame) {                 // the characters queried at `frame`, the one v holds
        while (want == frame) {
            R::combine(ln, cur, lane, S, v, red);
            --cur;
            want = query(cur);
        }
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = lane * K + k;
        v[k] = s == S - 1 || s == S - 2 ? R::one() : R::zero();
    }
    combine_at(T - 1);
    feed.prefetch(ln.P, T, nchunks - 1);
    for (int c = nchunks - 1; c >= 0; --c) {
        const E* buf = feed.publish(c, R::emit);
        feed.prefetch(ln.P, T, c - 1);
        wave_lds_sync();
        R::chunk_begin(v);
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t1 - 1; t >= t0 && t >= 1; --t) {  // the emission of frame t takes the fill from t to t - 1
            R::backward(v, skipf, lab, buf + (t - t0) * no);
            combine_at(t - 1);
        }
    }
}

}  // namespace
