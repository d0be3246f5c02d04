// forced_page_omit.h -- the page-scope kernel with omission, described at the top of
// ta_forced_page_omit.hip: page_omit_rows, OmitCell and forced_page_omit_kernel<K, Args>.  It is a header because it is
// instantiated in TWO translation units -- ta_forced_page_omit.hip (Args = PageArgs: ta_forced_align_pages_omit) and
// ta_forced_page_omit_gated.hip (Args = GatedPageArgs: ta_forced_align_pages_omit_gated, section 14.17) -- as
// forced_page_strict.h is for the strict kernel, and for the same reason: a unit each leaves the five existing variants
// instruction for instruction what they were (profiles/forced_page_omit_gated.txt).
#pragma once
#include "forced_page_common.h"

namespace {

__host__ __device__ inline int64_t page_omit_rows(int T, int K) { return forced_ws_rows(T, K) + omit_bit_rows(T, K); }

// the cell of page_fill: omit_step and the bit rows behind a line's moves.  At a line boundary the old registers are masked
// to the old window and scanned in old coordinates: that scan's bits are the new line's bit row of frame 0 (bits0), and its
// prefix maxima go through LDS beside the values (pbuf), where omit_step<K, true> finds its far candidates
template <int K>
struct OmitCell {
    int lane;
    long long omit, pen0;                              // pen0 = omit * (the lane's first window character)
    long long* pbuf;
    uint32_t* bitrows;
    uint32_t bits0, bits, accb;
    __device__ __forceinline__ void line(uint32_t* moves, int T) {
        bitrows = moves + forced_ws_rows(T, K) * 64;
        bits0 = accb = 0;
    }
    __device__ __forceinline__ void leave(long long (&v)[K], int wold, long long* vbuf) {
        long long but_last = kNeg;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            if (lane * K + r > wold) v[r] = kNeg;
            if (r < K - 1) but_last = max64(but_last, v[r] + pen0 + omit * ((r + 1) >> 1));
        }
        const long long total = max64(but_last, v[K - 1] + pen0 + omit * (K >> 1));
        long long run = from_left(wave_max_scan(total), kNeg);
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const long long ar = v[r] + pen0 + omit * ((r + 1) >> 1);
            if (ar >= run) bits0 |= 1u << r;
            run = max64(run, ar);
            vbuf[lane * K + r] = v[r];
            pbuf[lane * K + r] = run;
        }
    }
    __device__ __forceinline__ void seed(long long (&v)[K], const int (&lab)[K / 2], const int* q, int qb) {
        bits = 0;
        omit_seed<K>(v, lab, q, qb, omit, pen0);
    }
    template <bool kFirst>
    __device__ __forceinline__ unsigned long long step(long long (&v)[K], long long left, unsigned skip,
                                                       const int (&lab)[K / 2], const int* q, int qb, int d) {
        bits = kFirst ? bits0 : 0;
        return omit_step<K, kFirst>(v, left, skip, lab, q, qb, omit, pen0, lane, pbuf, d, bits);
    }
    __device__ __forceinline__ void stored(int t, int T) { store_bits<K>(bitrows, t, T, lane, bits, accb); }
};

// Args = GatedPageArgs (forced_page_common.h; kGated), as forced_page_strict.h's kernel takes it: the gate stands in front of
// the price's range check and of page_head -- a page with a reason leaves with TA_FORCED_SKIPPED before one of its numbers
// is read, it may have no lines or no text -- and behind page_head the page's variant may not exceed the one its cap sized
// the workspace for: refused by every launch alike, as page_head's refusals are
template <int K, class Args = PageArgs>
__global__ __launch_bounds__(64) void forced_page_omit_kernel(Args a) {
    constexpr bool kGated = std::is_same<Args, GatedPageArgs>::value;
    constexpr int kRows = walk_rows(K) + kWalk * K / 32;               // move and bit rows of a walk block
    constexpr int kWords = kRows * 64 > 2 * kChunk * kMaxNo ? kRows * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long pbuf[64 * K];                 // ... and the old window's prefix maxima of a[]
    __shared__ long long fin_v[64];
    __shared__ int fin_s[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    if constexpr (kGated) {
        if (a.gate[b] != 0) {                          // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_SKIPPED;
            return;
        }
    }
    if (a.omit < 0 || a.omit > TA_FORCED_OMIT_MAX) {   // wave-uniform
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    auto too_many_frames = [&](long long mine) {       // the lanes' shares through LDS, every lane reads all 64
        fin_v[lane] = mine;
        __syncthreads();
        long long all = 0;
        for (int l = 0; l < 64; ++l) all += fin_v[l];
        __syncthreads();
        return all > kMaxFrames;
    };
    PageHead h;
    if (!page_head(a, b, lane, kMaxChars, page_omit_rows, too_many_frames, h)) return;
    if constexpr (kGated) {
        const int w = a.cap[b];
        if (w < 0 || w > TA_FORCED_MAX_TARGET || h.KP > window_k(w)) {                             // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
            return;
        }
    }
    if (h.KP != K) return;                             // wave-uniform: the page belongs to another launch of this call
    if (!labels_ok(h.cs, h.n, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    int32_t* frames = a.frames + TA_FORCED_PAGE_FIELDS * h.c0;
    for (int64_t i = lane; i < (int64_t)TA_FORCED_PAGE_FIELDS * h.n; i += 64) frames[i] = TA_FORCED_OMITTED;

    long long v[K];
    const long long omit = a.omit;
    OmitCell<K> cell{lane, omit, omit * (long long)(lane * (K / 2)), pbuf};
    const int lo_last = page_fill<K>(a, h, lane, reinterpret_cast<int*>(stage), vbuf, v, cell);

    // ---- end: the largest fin over the last window's states up to 2 n, the largest s on a tie ----------------------------
    long long best;
    const int s = omit_end<K>(v, omit, 2 * lo_last, h.n, lane, fin_v, fin_s, &best);
    if (best < kDead || s < 0) {                       // wave-uniform; cannot happen within the limits
        if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
        return;
    }
    page_walk<K, true>(a, stage, h.l0, h.nl, s, frames, lane);
    __threadfence();
    __syncthreads();
    page_peaks<true>(a, h, frames, lane);
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

}  // namespace
