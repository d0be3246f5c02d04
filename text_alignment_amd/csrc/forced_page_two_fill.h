// forced_page_two_fill.h -- what ta_forced_page_conf.hip (max-marginals at page scope) and
// ta_forced_page_post.hip (sum-product posteriors at page scope, section 14.15) have in common: ONE wave runs a forward and
// a backward fill over the lattice of ALL the lines of a page -- windows that move from line to line, no character across a
// line break -- and combines the two at the query frame (line, t) of every character ("Shared pieces of the
// forced-alignment kernels" in 14.7).  Stated once here, on top of forced_page_common.h (the layout, page_head) and
// forced_two_fill.h (two_fill_best):
//   PageTwoFillArgs      the arguments both kernels take; each file's struct adds its outputs
//   page_queries_ok      the checks on a page's queries, TA_FORCED_QUERY
//   PageCursor           the query cursor, wave-uniform, in both directions
//   page_two_fill<K, R>  the kernel's body: the head, the two fills and the combine at every query frame
//   page_two_fill_call   the body of the two extern "C" entries
// R, a struct of static members per file, is the arithmetic: the types V (a state's value), E (an emission in LDS), Args,
// Buf (the LDS a line boundary goes through) and Red (the LDS of a combine); rows_of (the 256-byte rows of a page's piece of
// the workspace); zero, one, emit, first (a state's value in frame 0 from its emission), left and left_edge (the left lane's
// value; in the first frame of a line behind the first, lane 0 takes the state in front of the new window) and apply (an
// emission on a value: add against multiply); put_v / get_v (a state through Buf, a state that is not live as zero) and edge
// (get, where the posterior normalises); end_put / end_get (a value through Red); chunk_begin; forward<K, kFirst>, backward
// and boundary (the cell of a frame for a lane's K states -- boundary: the second half of a backward line boundary, in which
// a label state has no stay candidate and nothing is left above the new window's last state); store_row, forward_done
// (false: TA_FORCED_NOPATH) and combine, whose reduction is two_fill_best.  The cells stay in R, as forced_two_fill.h's do;
// so does the callable handed to page_head (the page's frames against the file's cap, through the file's own LDS).
// What each kernel's instruction stream made of these pieces: profiles/forced_page_two_fill.txt.
#pragma once
#include "forced_page_common.h"
#include "forced_two_fill.h"

namespace {

struct PageTwoFillArgs : PageArgs {
    const int32_t* query;      // [nlabels][TA_FORCED_PAGE_FIELDS]: field 0 the line, field 3 the frame
};

// TA_FORCED_QUERY for a line outside the page, a frame outside its line, an own state outside its line's window, and
// queries that decrease in (line, frame) order
__device__ __forceinline__ bool page_queries_ok(const PageTwoFillArgs& a, const PageHead& h, const int32_t* qs, int b, int lane) {
    bool bad = false;
    for (int i = lane; i < h.n; i += 64) {
        const int k = qs[TA_FORCED_PAGE_FIELDS * (int64_t)i], t = qs[TA_FORCED_PAGE_FIELDS * (int64_t)i + 3];
        if (k < 0 || k >= h.nl) { bad = true; continue; }
        bad |= t < 0 || t >= a.T[h.l0 + k] || i < a.lo[h.l0 + k] || i >= a.hi[h.l0 + k];
        if (i >= 1) {
            const int kp = qs[TA_FORCED_PAGE_FIELDS * (int64_t)(i - 1)], tp = qs[TA_FORCED_PAGE_FIELDS * (int64_t)(i - 1) + 3];
            bad |= kp > k || (kp == k && tp > t);
        }
    }
    if (__any(bad)) {
        if (lane == 0) a.status[b] = TA_FORCED_QUERY;
        return false;
    }
    return true;
}

// the query cursor, wave-uniform: the next character whose query is still ahead, its line and its frame
struct PageCursor {
    const int32_t* qs;
    int n, cur, wk, wt;
    __device__ __forceinline__ void fetch() {
        const bool in = cur >= 0 && cur < n;
        wk = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur]) : -1;
        wt = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur + 3]) : -1;
    }
    __device__ __forceinline__ void start(int at) { cur = at; fetch(); }
    __device__ __forceinline__ bool at(int k, int t) const { return wk == k && wt == t; }
};

// Block b's page, if it is variant K's: page_head<true> (the page's ONE workspace piece, `over` the file's cap on the
// page's frames), labels_ok and page_queries_ok; then the two fills.  No barrier inside a fill (wave_lds_sync).
//   forward   page_fill's control structure without moves.  Over a boundary the values go through vbuf masked to the old
//             window's live states and come back shifted by 2 (lo_{k+1} - lo_k).  At a character's query frame the lane
//             stores its row in the query line's window coordinates: queries do not decrease, so one cursor meets them in
//             order.  forward_done sees the page's last two states.
//   backward  from the last line to the first, a line's chunks from last to first; the chunk "ahead" of a line's first
//             chunk is the previous line's last.  The emission of frame t takes the fill from t to t - 1.  The step over a
//             line boundary is split: the emission of frame (k, 0) is applied in window k's coordinates and labels, the
//             values go through vbuf masked to window k's live states and come back shifted into window k - 1's
//             coordinates, labels and skip bits are loaded again, and R::boundary finishes the step.  The skip bits are
//             those of the page's text, not of the window's: over a boundary a skip may end in a character behind the window.
//   combine   at a query frame the character's forward row comes back to the lane that stored it: n times per page.
template <int K, class R, class Over>
__device__ __forceinline__ void page_two_fill(const typename R::Args& a, typename R::E* tab, typename R::Buf vbuf,
                                              typename R::Red* red, Over over) {
    using V = typename R::V;
    using E = typename R::E;
    const int b = blockIdx.x, lane = threadIdx.x;
    PageHead h;
    if (!page_head<true>(a, b, lane, kMaxText, R::rows_of, over, h)) return;
    if (h.KP != K) return;                             // wave-uniform: the page belongs to another launch of this call
    if (!labels_ok(h.cs, h.n, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    const int n = h.n, nl = h.nl, no = a.no;
    const int64_t l0 = h.l0;
    PageCursor q{a.query + TA_FORCED_PAGE_FIELDS * h.c0, n, 0, -1, -1};
    if (!page_queries_ok(a, h, q.qs, b, lane)) return;
    unsigned char* rows = a.ws + a.ws_off[b];          // row i: the forward fill at character i's query frame

    V v[K];
    int lab[K / 2];
    Feed<E> feed(tab, no, lane);
    int g = 0;                                         // chunks so far: the LDS buffer in turn

    // ---- forward fill; the row of every query frame is kept --------------------------------------------------------------
    {
#pragma unroll
        for (int r = 0; r < K; ++r) v[r] = R::zero();
        q.fetch();
        int T = __builtin_amdgcn_readfirstlane(a.T[l0]);
        const float* P = a.probs + a.row_off[l0] * no;
        feed.prefetch(P, T, 0);
        int lo_old = 0, hi_old = 0;
        for (int k = 0; k < nl; ++k) {
            const int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]), hi = __builtin_amdgcn_readfirstlane(a.hi[l0 + k]);
            V edge = R::zero();
            const int d = 2 * (lo - lo_old);           // old window states in front of the new window
            if (k > 0) {                               // from the old window's lanes and registers to the new one's
                const int wold = 2 * (hi_old - lo_old);
                wave_lds_sync();
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r;
                    R::put_v(vbuf, j, j <= wold, v[r]);
                }
                wave_lds_sync();
                if (d >= 1) edge = R::edge(vbuf, d - 1);               // d - 1 < wold: lo <= hi_old
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r + d;
                    v[r] = j < 64 * K ? R::get_v(vbuf, j) : R::zero();
                }
            }
            const unsigned skip = lane_labels(h.cs, lo, hi, lane, lab);
            // the line behind, for the chunk ahead of this line's last
            const bool more = k + 1 < nl;
            const int Tn = more ? __builtin_amdgcn_readfirstlane(a.T[l0 + k + 1]) : 0;
            const float* Pn = more ? a.probs + a.row_off[l0 + k + 1] * no : P;
            const int nchunks = (T + kChunk - 1) / kChunk;
            for (int c = 0; c < nchunks; ++c, ++g) {
                const E* buf = feed.publish(g, R::emit);
                if (c + 1 < nchunks) feed.prefetch(P, T, c + 1);
                else feed.prefetch(Pn, Tn, 0);
                wave_lds_sync();
                R::chunk_begin(v);
                const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
                for (int t = t0; t < t1; ++t) {
                    const E* e = buf + (t - t0) * no;
                    if (t == 0) {
                        if (k == 0) {
                            if (lane == 0) { v[0] = R::first(e[0]); v[1] = R::first(e[lab[0]]); }
                        } else {
                            R::template forward<K, true>(v, R::left_edge(v[K - 1], edge, lane), skip, lab, e);
                        }
                    } else {
                        R::template forward<K, false>(v, R::left(v[K - 1]), skip, lab, e);
                    }
                    while (q.at(k, t)) {
                        R::store_row(rows, q.cur, lane, v);
                        ++q.cur;
                        q.fetch();
                    }
                }
            }
            lo_old = lo;
            hi_old = hi;
            P = Pn;
            T = Tn;
        }
        // the end: the last window ends at the page's last state (hi = n); an empty last window does not hold 2 n - 1
        if (lane == 0) { R::end_put(red, 0, R::zero()); R::end_put(red, 1, R::zero()); }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int s = 2 * lo_old + lane * K + r;
            if (s == 2 * n) R::end_put(red, 0, v[r]);
            if (s == 2 * n - 1) R::end_put(red, 1, v[r]);
        }
        __syncthreads();                               // (a row is read back by the very lane that stored it)
        const V e0 = R::end_get(red, 0), e1 = R::end_get(red, 1);
        __syncthreads();
        if (!R::forward_done(a, b, lane, e0, e1)) {    // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
            return;
        }
    }

    // ---- backward fill, and the combine at every query frame ------------------------------------------------------------
    q.start(n - 1);
    int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + nl - 1]), hi = n;
    auto combine_at = [&](int k, int t) {              // the characters queried at frame (k, t), the one v holds
        while (q.at(k, t)) {
            R::combine(a, h, rows, q.cur, lo, hi, lane, v, red);
            wave_lds_sync();                           // red is free again
            --q.cur;
            q.fetch();
        }
    };
    int T = __builtin_amdgcn_readfirstlane(a.T[l0 + nl - 1]);
    const float* P = a.probs + a.row_off[l0 + nl - 1] * no;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = 2 * lo + lane * K + r;
        v[r] = s == 2 * n || s == 2 * n - 1 ? R::one() : R::zero();
    }
    combine_at(nl - 1, T - 1);
    feed.prefetch(P, T, (T + kChunk - 1) / kChunk - 1);
    for (int k = nl - 1; k >= 0; --k) {
        unsigned skipf;
        lane_labels(h.cs, lo, n, lane, lab, &skipf);   // from the page's whole text: a skip may end behind the window
        // the line in front, for the chunk "ahead" of this line's first
        const int Tp = k > 0 ? __builtin_amdgcn_readfirstlane(a.T[l0 + k - 1]) : 0;
        const float* Pp = k > 0 ? a.probs + a.row_off[l0 + k - 1] * no : P;
        const int nchunks = (T + kChunk - 1) / kChunk;
        const E* e0 = tab;                             // frame 0's emissions: the first row of chunk 0's buffer
        for (int c = nchunks - 1; c >= 0; --c, ++g) {
            const E* buf = feed.publish(g, R::emit);
            if (c >= 1) feed.prefetch(P, T, c - 1);
            else feed.prefetch(Pp, Tp, (Tp + kChunk - 1) / kChunk - 1);        // (k = 0: no such chunk, zeros)
            wave_lds_sync();
            R::chunk_begin(v);
            e0 = buf;
            const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
            for (int t = t1 - 1; t >= t0 && t >= 1; --t) {             // the emission of frame t takes the fill from t to t - 1
                R::template backward<K>(v, skipf, lab, buf + (t - t0) * no);
                combine_at(k, t - 1);
            }
        }
        if (k == 0) break;                             // the page's first frame: its emission is never applied
        // ---- over the line boundary: frame (k, 0)'s emission in window k, then into window k - 1 --------------------------
        {
            const E eb = e0[0];
            const int wlast = 2 * (hi - lo);
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                R::put_v(vbuf, j, j <= wlast, R::apply(v[r], (r & 1) ? e0[lab[r >> 1]] : eb));
            }
            wave_lds_sync();
        }
        const int lo_new = __builtin_amdgcn_readfirstlane(a.lo[l0 + k - 1]), hi_new = __builtin_amdgcn_readfirstlane(a.hi[l0 + k - 1]);
        {
            const int d = 2 * (lo - lo_new);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r - d;        // the state in window k's coordinates
                v[r] = j >= 0 ? R::get_v(vbuf, j) : R::zero();
            }
            unsigned skipb;
            lane_labels(h.cs, lo_new, n, lane, lab, &skipb);
            R::template boundary<K>(v, skipb, 2 * (hi_new - lo_new), lane);
        }
        lo = lo_new;
        hi = hi_new;
        P = Pp;
        T = Tp;
        combine_at(k - 1, T - 1);
    }
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// The body of ta_forced_page_confidence and ta_forced_page_posterior behind their argument struct `a` (variants not yet
// set): forced_preamble (outputs_null: the file's own pointers), forced_check_pages' refusals with the file's cap on a
// page's frames -- its workspace rule, a piece per line, asks nothing here -- then the page's rule, ONE piece of
// bytes_of(characters, the page's variant) bytes per page (ws_name: the exported function that tells a caller so), and
// launch(kc, a) for every variant the pages call for.
template <class Args, class Bytes, class Launch>
inline int page_two_fill_call(Args a, bool outputs_null, const int32_t* T_host, const int64_t* line_first_host,
                              const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host, int64_t max_frames,
                              const char* max_frames_msg, const char* ws_name, const char* launch_name, Bytes bytes_of,
                              Launch launch) {
    bool go;
    const int rc = forced_preamble(a.npages < 0 || a.nlines < 0 || a.rows < 0 || a.nlabels < 0 || a.ws_bytes < 0, a.no, nullptr,
                                   a.npages == 0,
                                   !a.probs || !a.row_off || !a.T || !a.line_first || !a.lo || !a.hi || !a.labels || !a.lab_off ||
                                       !a.ws_off || !a.query || !T_host || !line_first_host || !lo_host || !hi_host ||
                                       !lab_off_host || !a.ws || outputs_null || !a.status,
                                   a.ws, &go);
    if (!go) return rc;
    const int rc2 = forced_check_pages(T_host, line_first_host, lo_host, hi_host, lab_off_host, a.npages, a.nlines, a.rows,
                                       a.nlabels, a.ws_bytes, [](int, int) { return (int64_t)0; }, kMaxText,
                                       "a page's text is too long", max_frames, max_frames_msg, ws_name, &a.variants);
    if (rc2 != TA_OK) return rc2;
    int64_t need = 0;
    for (int p = 0; p < a.npages && need <= a.ws_bytes; ++p) {             // (a piece is at most 2^44 bytes)
        int kp = 2;
        for (int64_t q = line_first_host[p]; q < line_first_host[p + 1]; ++q) {
            const int kw = window_k(hi_host[q] - lo_host[q]);
            kp = kw > kp ? kw : kp;
        }
        need += bytes_of(lab_off_host[p + 1] - lab_off_host[p], kp);
    }
    if (a.ws_bytes < need) return forced_ws_small("pages", ws_name);
    const hipError_t e = forced_launch_variants(a.variants, [&](auto kc) { launch(kc, a); });
    if (e != hipSuccess) return ta_fail_hip(e, launch_name);
    return TA_OK;
}

}  // namespace
