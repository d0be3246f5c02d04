// forced_page_strict.h -- the strict page-scope kernel, described at the top of ta_forced_page.hip:
// StrictCell and forced_page_kernel<K, Args>.  It is a header because it is instantiated in TWO translation units --
// ta_forced_page.hip (Args = PageArgs: ta_forced_align_pages) and ta_forced_page_gated.hip (Args = GatedPageArgs:
// ta_forced_align_pages_gated, section 14.14).  One unit with both moved the instruction streams of the five existing
// variants (register allocation and scheduling, a kernel's code depending on its neighbours in the module); a unit each
// leaves them instruction for instruction what they were (profiles/forced_page_gated.txt).
#pragma once
#include "forced_page_common.h"

namespace {

// the cell of page_fill: forced_step, the old window masked into vbuf, and nothing of its own per line or frame
template <int K>
struct StrictCell {
    int lane;
    __device__ __forceinline__ void line(uint32_t*, int) {}
    __device__ __forceinline__ void leave(long long (&v)[K], int wold, long long* vbuf) {
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int j = lane * K + r;
            vbuf[j] = j <= wold ? v[r] : kNeg;
        }
    }
    __device__ __forceinline__ void seed(long long (&v)[K], const int (&lab)[K / 2], const int* q, int qb) {
        if (lane == 0) { v[0] = qb; v[1] = q[lab[0]]; }
    }
    template <bool kFirst>
    __device__ __forceinline__ unsigned long long step(long long (&v)[K], long long left, unsigned skip,
                                                       const int (&lab)[K / 2], const int* q, int qb, int) {
        return forced_step<K, kFirst>(v, left, skip, lab, q, qb);
    }
    __device__ __forceinline__ void stored(int, int) {}
};

// Args = GatedPageArgs (forced_page_common.h; kGated): the gate stands in front of page_head -- a page with a reason leaves with TA_FORCED_SKIPPED
// before one of its numbers is read, it may have no lines or no text -- and the page's variant may not exceed the one its cap
// sized the workspace for: refused by every launch alike, as page_head's refusals are
template <int K, class Args = PageArgs>
__global__ __launch_bounds__(64) void forced_page_kernel(Args a) {
    constexpr bool kGated = std::is_same<Args, GatedPageArgs>::value;
    constexpr int kWords = walk_rows(K) * 64 > 2 * kChunk * kMaxNo ? walk_rows(K) * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long vend[2];
    const int b = blockIdx.x, lane = threadIdx.x;
    if constexpr (kGated) {
        if (a.gate[b] != 0) {                          // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_SKIPPED;
            return;
        }
    }
    PageHead h;
    if (!page_head(a, b, lane, kMaxText, forced_ws_rows, [](long long) { return false; }, h)) return;
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
    const int n = h.n;

    long long v[K];
    StrictCell<K> cell{lane};
    const int lo_last = page_fill<K>(a, h, lane, reinterpret_cast<int*>(stage), vbuf, v, cell);

    // ---- end: the last window ends at the page's last state (hi = n): window state 2 (n - lo_last) is page state 2 n; the
    // last character's state lies in front of an empty last window and is not live then
    if (lane == 0) vend[0] = vend[1] = kNeg;
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = 2 * lo_last + lane * K + r;
        if (s == 2 * n) vend[0] = v[r];
        if (s == 2 * n - 1) vend[1] = v[r];
    }
    __threadfence();                                   // the moves are read back below, by other lanes
    __syncthreads();
    const long long e0 = vend[0], e1 = vend[1];
    const long long best = e1 > e0 ? e1 : e0;
    if (best < kDead) {                                // wave-uniform
        if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
        return;
    }
    int32_t* frames = a.frames + TA_FORCED_PAGE_FIELDS * h.c0;
    page_walk<K, false>(a, stage, h.l0, h.nl, e1 > e0 ? 2 * n - 1 : 2 * n, frames, lane);      // on a tie the last blank
    __threadfence();
    __syncthreads();
    page_peaks<false>(a, h, frames, lane);
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

}  // namespace
