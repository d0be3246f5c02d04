// ta_forced_page_conf.hip -- per-character confidence at page scope from max-marginals: for a
// query frame (line, t) per character i of a page's text, the total of the best legal path through ALL the lines of the
// page that spends that frame in the character's own state 2 i + 1, minus the total of the best one that spends it in any
// other live state, and that state.  Integers only, on the lattice of ta_forced_page.hip (windows that move from line to
// line, no character across a line break); the checker of record is tests/forced_page_conf_ref.py.
//
// forced_page_conf_kernel<K>, one wave per page, the layout of forced_page_common.h: lane l holds the K consecutive
// WINDOW states l K .. l K + K - 1 (page state minus 2 lo_k) of the line it is in as int64 registers.  ONE wave runs both
// fills, one after the other, with no barrier inside a fill (wave_lds_sync), as two_fill does for a line:
//   head      page_head<true>: the page's ONE workspace piece (512 K n bytes, a forward row per character), a page
//             of more than 2^25 frames refused (G 2048 and the reachability test stay exact), then labels_ok and the
//             queries: TA_FORCED_QUERY for a line outside the page, a frame outside its line, an own state outside its
//             line's window, and queries that decrease in (line, frame) order.
//   forward   A: page_fill's control structure without moves; the cell is forced_step without them.  At a character's
//             query frame the lane stores its row, K coalesced 8-byte stores, in the query line's window coordinates.  A
//             best end below -2^49: TA_FORCED_NOPATH, and the outputs are left alone.
//   backward  B, from the last line to the first, a line's chunks from last to first; the chunk "ahead" of a line's first
//             chunk is the previous line's last.  Inside a line the step is ta_forced_conf.hip's (the RIGHT lane's first two
//             values, wave_shl:1).  The step over a line boundary is split: the emission of frame (k + 1, 0) is added in
//             window k + 1's coordinates and labels, the values go through vbuf masked to window k + 1's live states and
//             come back shifted by 2 (lo_{k+1} - lo_k) into window k's coordinates, labels and skip bits are loaded again,
//             and the max has no stay candidate for a label state.  The skip bits are those of the page's text, not of
//             the window's: over a boundary a skip may end in a character behind window k.
//   masks     the forward fill leaves junk above a window's last state (a state reads lower states only, so no live state
//             ever reads it).  The backward fill reads HIGHER states: at every boundary the states above the new window's
//             last state are set to -2^50, and from there they only go down (every emission is <= 0).
//   combine   at a query frame the character's forward row comes back, G = A + B where both are above -2^49 (else exactly
//             -2^50), states beyond the window's last state left out, G 2048 + (2047 - window state) reduced 64 -> 8 -> 1
//             (two_fill_best's shape): the largest value at the smallest state.  n times per page, not once per frame.
// Every bound is re-checked on the page's own device numbers before anything is read through it; a refused page gets a
// status and touches nothing else.
#include "forced_page_common.h"

namespace {

constexpr long long kReach = -(1ll << 49);

struct PageConfArgs : PageArgs {
    const int32_t* query;      // [nlabels][TA_FORCED_PAGE_FIELDS]: field 0 the line, field 3 the frame
    int64_t* confidence;
    int32_t* rival;
};

// a page's ONE piece of the workspace: a forward row of 64 K int64 per character, 512 K n bytes, in rows of 256 bytes
__host__ __device__ inline int64_t page_conf_rows(int n, int K) { return 2 * (int64_t)K * n; }
__host__ __device__ inline int64_t page_conf_bytes(int64_t n, int K) { return 256 * page_conf_rows((int)n, K); }

// a frame inside a line, downwards in time: ta_forced_conf.hip's ConfCells::backward
template <int K>
__device__ __forceinline__ void page_conf_backward(long long (&v)[K], unsigned skipf, const int (&lab)[K / 2], const int* q) {
    const int qb = q[0];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += (k & 1) ? q[lab[k >> 1]] : qb;
    const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
    for (int k = 0; k < K; ++k) {                      // upwards: v[k + 1] and v[k + 2] still carry frame t
        long long best = v[k];
        const long long adv = k + 1 < K ? v[(k + 1) % K] : r0;
        if (adv > best) best = adv;
        if (k & 1) {
            const long long sk = k + 2 < K ? v[(k + 2) % K] : r1;
            if (((skipf >> (k >> 1)) & 1u) && sk > best) best = sk;
        }
        v[k] = best;
    }
}

// the K / 2 labels of a lane in the window that starts at character lo, and bit j of the result: from label j the blank
// behind it may be skipped.  Both from the page's whole text: a state above the window's last is below kReach whatever
// is added to it, and over a line boundary a skip may end behind the window.
template <int H>
__device__ __forceinline__ unsigned page_conf_labels(const int32_t* cs, int lo, int n, int lane, int (&lab)[H]) {
    unsigned skipf;
    lane_labels(cs, lo, n, lane, lab, &skipf);
    return skipf;
}

template <int K>
__global__ __launch_bounds__(64) void forced_page_conf_kernel(PageConfArgs a) {
    __shared__ int qtab[2 * kChunk * kMaxNo];          // two chunks of emission scores (8 KiB)
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long red[73];                      // a combine's 64 candidates, 8 partial maxima, the own state's value
    const int b = blockIdx.x, lane = threadIdx.x;
    auto too_many_frames = [&](long long mine) {       // the lanes' shares through LDS, every lane reads all 64
        red[lane] = mine;
        __syncthreads();
        long long all = 0;
        for (int l = 0; l < 64; ++l) all += red[l];
        __syncthreads();
        return all > kMaxFrames;
    };
    PageHead h;
    if (!page_head<true>(a, b, lane, kMaxText, page_conf_rows, too_many_frames, h)) return;
    if (h.KP != K) return;                             // wave-uniform: the page belongs to another launch of this call
    if (!labels_ok(h.cs, h.n, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    const int n = h.n, nl = h.nl, no = a.no;
    const int64_t l0 = h.l0;
    const int32_t* qs = a.query + TA_FORCED_PAGE_FIELDS * h.c0;
    {
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const int k = qs[TA_FORCED_PAGE_FIELDS * (int64_t)i], t = qs[TA_FORCED_PAGE_FIELDS * (int64_t)i + 3];
            if (k < 0 || k >= nl) { bad = true; continue; }
            bad |= t < 0 || t >= a.T[l0 + k] || i < a.lo[l0 + k] || i >= a.hi[l0 + k];
            if (i >= 1) {
                const int kp = qs[TA_FORCED_PAGE_FIELDS * (int64_t)(i - 1)], tp = qs[TA_FORCED_PAGE_FIELDS * (int64_t)(i - 1) + 3];
                bad |= kp > k || (kp == k && tp > t);
            }
        }
        if (__any(bad)) {
            if (lane == 0) a.status[b] = TA_FORCED_QUERY;
            return;
        }
    }
    long long* rows = reinterpret_cast<long long*>(a.ws + a.ws_off[b]);     // row i: 64 K values, register r at r * 64 + lane
    int64_t* conf = a.confidence + h.c0;
    int32_t* rival = a.rival + h.c0;

    long long v[K];
    int lab[K / 2];
    Feed<int> feed(qtab, no, lane);
    // the query cursor, wave-uniform: the next character whose query is still ahead, its line and its frame
    int cur = 0, wk = -1, wt = -1;
    auto fetch = [&]() {
        const bool in = cur >= 0 && cur < n;
        wk = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur]) : -1;
        wt = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur + 3]) : -1;
    };
    int g = 0;                                         // chunks so far: the LDS buffer in turn

    // ---- forward fill: page_fill without moves; the row of every query frame is kept ------------------------------------
    {
#pragma unroll
        for (int r = 0; r < K; ++r) v[r] = kNeg;
        fetch();
        int T = __builtin_amdgcn_readfirstlane(a.T[l0]);
        const float* P = a.probs + a.row_off[l0] * no;
        feed.prefetch(P, T, 0);
        int lo_old = 0, hi_old = 0;
        for (int k = 0; k < nl; ++k) {
            const int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]), hi = __builtin_amdgcn_readfirstlane(a.hi[l0 + k]);
            long long edge = kNeg;
            const int d = 2 * (lo - lo_old);           // old window states in front of the new window
            if (k > 0) {                               // from the old window's lanes and registers to the new one's
                const int wold = 2 * (hi_old - lo_old);
                wave_lds_sync();
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r;
                    vbuf[j] = j <= wold ? v[r] : kNeg;
                }
                wave_lds_sync();
                if (d >= 1) edge = vbuf[d - 1];        // d - 1 < wold: lo <= hi_old
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r + d;
                    v[r] = j < 64 * K ? vbuf[j] : kNeg;
                }
            }
            const unsigned skip = lane_labels(h.cs, lo, hi, lane, lab);
            const bool more = k + 1 < nl;
            const int Tn = more ? __builtin_amdgcn_readfirstlane(a.T[l0 + k + 1]) : 0;
            const float* Pn = more ? a.probs + a.row_off[l0 + k + 1] * no : P;
            const int nchunks = (T + kChunk - 1) / kChunk;
            for (int c = 0; c < nchunks; ++c, ++g) {
                const int* qbuf = feed.publish(g, emission_q);
                if (c + 1 < nchunks) feed.prefetch(P, T, c + 1);
                else feed.prefetch(Pn, Tn, 0);
                wave_lds_sync();
                const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
                for (int t = t0; t < t1; ++t) {
                    const int* q = qbuf + (t - t0) * no;
                    const int qb = q[0];
                    if (t == 0) {
                        if (k == 0) {
                            if (lane == 0) { v[0] = qb; v[1] = q[lab[0]]; }
                        } else {
                            forced_step<K, true>(v, from_left(v[K - 1], edge), skip, lab, q, qb);
                        }
                    } else {
                        forced_step<K, false>(v, from_left(v[K - 1], kNeg), skip, lab, q, qb);
                    }
                    while (wk == k && wt == t) {
                        long long* row = rows + (int64_t)cur * (64 * K);
#pragma unroll
                        for (int r = 0; r < K; ++r) row[r * 64 + lane] = v[r];
                        ++cur;
                        fetch();
                    }
                }
            }
            lo_old = lo;
            hi_old = hi;
            P = Pn;
            T = Tn;
        }
        // the end: the last window ends at the page's last state (hi = n)
        if (lane == 0) red[0] = red[1] = kNeg;
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int s = 2 * lo_old + lane * K + r;
            if (s == 2 * n) red[0] = v[r];
            if (s == 2 * n - 1) red[1] = v[r];
        }
        __syncthreads();                               // (a row is read back by the very lane that stored it)
        const long long e0 = red[0], e1 = red[1];
        __syncthreads();
        if ((e1 > e0 ? e1 : e0) < kDead) {             // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
            return;
        }
    }

    // ---- backward fill, and the combine at every query frame ------------------------------------------------------------
    cur = n - 1;
    fetch();
    int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + nl - 1]), hi = n;
    auto combine_at = [&](int k, int t) {              // the characters queried at frame (k, t), the one v holds B of
        while (wk == k && wt == t) {
            const long long* row = rows + (int64_t)cur * (64 * K);
            const int own = 2 * (cur - lo) + 1, wlast = 2 * (hi - lo);
            long long key = kNeg * 2048;               // below every candidate's
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                const long long fa = row[r * 64 + lane];               // what this very lane stored in the forward fill
                const long long gs = fa > kReach && v[r] > kReach ? fa + v[r] : kNeg;
                const long long cand = gs * 2048 + (2047 - j);          // the larger value first, then the smaller state
                if (j == own) red[72] = gs;
                else if (j <= wlast && cand > key) key = cand;
            }
            // two_fill_best's 64 -> 8 -> 1
            red[lane] = key;
            wave_lds_sync();
            if (lane < 8) {
                long long m = red[8 * lane];
#pragma unroll
                for (int j = 1; j < 8; ++j) m = max64(m, red[8 * lane + j]);
                red[64 + lane] = m;
            }
            wave_lds_sync();
            if (lane == 0) {
                long long m = red[64];
#pragma unroll
                for (int j = 1; j < 8; ++j) m = max64(m, red[64 + j]);
                conf[cur] = red[72] - (m >> 11);
                rival[cur] = 2 * lo + 2047 - (int)(m & 2047);
            }
            wave_lds_sync();                           // red is free again
            --cur;
            fetch();
        }
    };
    int T = __builtin_amdgcn_readfirstlane(a.T[l0 + nl - 1]);
    const float* P = a.probs + a.row_off[l0 + nl - 1] * no;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = 2 * lo + lane * K + r;
        v[r] = s == 2 * n || s == 2 * n - 1 ? 0 : kNeg;
    }
    combine_at(nl - 1, T - 1);
    feed.prefetch(P, T, (T + kChunk - 1) / kChunk - 1);
    for (int k = nl - 1; k >= 0; --k) {
        const unsigned skipf = page_conf_labels(h.cs, lo, n, lane, lab);
        // the line in front, for the chunk "ahead" of this line's first
        const int Tp = k > 0 ? __builtin_amdgcn_readfirstlane(a.T[l0 + k - 1]) : 0;
        const float* Pp = k > 0 ? a.probs + a.row_off[l0 + k - 1] * no : P;
        const int nchunks = (T + kChunk - 1) / kChunk;
        const int* q0 = qtab;                          // frame 0's scores: the first row of chunk 0's buffer
        for (int c = nchunks - 1; c >= 0; --c, ++g) {
            const int* qbuf = feed.publish(g, emission_q);
            if (c >= 1) feed.prefetch(P, T, c - 1);
            else feed.prefetch(Pp, Tp, (Tp + kChunk - 1) / kChunk - 1);        // (k = 0: no such chunk, zeros)
            wave_lds_sync();
            q0 = qbuf;
            const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
            for (int t = t1 - 1; t >= t0 && t >= 1; --t) {             // the emission of frame t takes the fill from t to t - 1
                page_conf_backward<K>(v, skipf, lab, qbuf + (t - t0) * no);
                combine_at(k, t - 1);
            }
        }
        if (k == 0) break;                             // the page's first frame: its emission is never applied
        // ---- over the line boundary: frame (k, 0)'s emission in window k, then into window k - 1 --------------------------
        {
            const int qb = q0[0], wlast = 2 * (hi - lo);
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                vbuf[j] = j <= wlast ? v[r] + ((r & 1) ? q0[lab[r >> 1]] : qb) : kNeg;
            }
            wave_lds_sync();
        }
        const int lo_new = __builtin_amdgcn_readfirstlane(a.lo[l0 + k - 1]), hi_new = __builtin_amdgcn_readfirstlane(a.hi[l0 + k - 1]);
        {
            const int d = 2 * (lo - lo_new), wlast = 2 * (hi_new - lo_new);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r - d;        // the state in window k's coordinates
                v[r] = j >= 0 ? vbuf[j] : kNeg;
            }
            const unsigned skipb = page_conf_labels(h.cs, lo_new, n, lane, lab);
            const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
            for (int r = 0; r < K; ++r) {              // upwards; a label state has no stay candidate
                long long best = (r & 1) ? kNeg : v[r];
                const long long adv = r + 1 < K ? v[(r + 1) % K] : r0;
                if (adv > best) best = adv;
                if (r & 1) {
                    const long long sk = r + 2 < K ? v[(r + 2) % K] : r1;
                    if (((skipb >> (r >> 1)) & 1u) && sk > best) best = sk;
                }
                v[r] = lane * K + r <= wlast ? best : kNeg;             // nothing above the new window's last state
            }
        }
        lo = lo_new;
        hi = hi_new;
        P = Pp;
        T = Tp;
        combine_at(k - 1, T - 1);
    }
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

}  // namespace

extern "C" int64_t ta_forced_page_confidence_workspace_bytes(int64_t n, int32_t K) {
    if (n < 1 || n > kMaxText || !(K == 2 || K == 4 || K == 8 || K == 16 || K == 32)) return -1;
    return page_conf_bytes(n, K);
}

extern "C" int ta_forced_page_confidence(const float* probs, const int64_t* row_off, const int32_t* T,
                                         const int64_t* line_first, const int32_t* lo, const int32_t* hi,
                                         const int32_t* labels, const int64_t* lab_off, const int64_t* ws_off,
                                         const int32_t* query, int32_t npages, int32_t nlines, int32_t no, int64_t rows,
                                         int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                                         const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host,
                                         void* workspace, int64_t workspace_bytes, int64_t* confidence, int32_t* rival,
                                         int32_t* status, void* stream) {
    bool go;
    const int rc = forced_preamble(npages < 0 || nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr,
                                   npages == 0,
                                   !probs || !row_off || !T || !line_first || !lo || !hi || !labels || !lab_off || !ws_off ||
                                       !query || !T_host || !line_first_host || !lo_host || !hi_host || !lab_off_host ||
                                       !workspace || !confidence || !rival || !status,
                                   workspace, &go);
    if (!go) return rc;
    int variants;
    // forced_check_pages' refusals; its workspace rule (a piece per line) asks nothing here, the page's rule follows
    const int rc2 = forced_check_pages(T_host, line_first_host, lo_host, hi_host, lab_off_host, npages, nlines, rows, nlabels,
                                       workspace_bytes, [](int, int) { return (int64_t)0; }, kMaxText, "a page's text is too long",
                                       kMaxFrames, "a page has more than 2^25 frames", "ta_forced_page_confidence_workspace_bytes",
                                       &variants);
    if (rc2 != TA_OK) return rc2;
    int64_t need = 0;
    for (int p = 0; p < npages && need <= workspace_bytes; ++p) {          // (a piece is at most 2^43 bytes)
        int kp = 2;
        for (int64_t q = line_first_host[p]; q < line_first_host[p + 1]; ++q) {
            const int kw = window_k(hi_host[q] - lo_host[q]);
            kp = kw > kp ? kw : kp;
        }
        need += page_conf_bytes(lab_off_host[p + 1] - lab_off_host[p], kp);
    }
    if (workspace_bytes < need) return forced_ws_small("pages", "ta_forced_page_confidence_workspace_bytes");
    const PageConfArgs a{{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                          nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, nullptr, nullptr, status, 0},
                         query, confidence, rival};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_conf_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_conf_kernel launch");
    return TA_OK;
}
