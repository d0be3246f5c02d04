// forced_page_common.h -- what ta_forced_page.hip (one strict path through all lines of a page) and
// ta_forced_page_omit.hip (the same on the lattice with the far move, section 14.12) have in common, and what
// ta_forced_page_conf.hip (max-marginals on the strict page lattice, section 14.13) and ta_forced_page_post.hip (sum-product
// posteriors on it, section 14.15) take of it: ONE wave per page, lane l holding the K consecutive WINDOW states
// l K .. l K + K - 1 (page state minus 2 lo_k) of the line it is in.
// Stated once here, on top of forced_common.h:
//   limits          kDead, kMaxText (strict), kMaxChars and kMaxFrames (with omission)
//   PageArgs        the arguments both kernels take; omit is 0 in the strict entry; GatedPageArgs: gate and cap on top
//   window_k        the variant of a window
//   page_head       the kernel's prologue: every bound on the page's own numbers and the page's variant (kPerPage: the
//                   workspace is one piece per page, ta_forced_page_conf.hip's)
//   page_fill       the fill's control structure: the lines, the chunks that restart with every line and look ahead into
//                   the next, the re-basing of the values from one window to the next through vbuf, the moves
//   page_walk       the walk back through the lines, kOmit: with the bit rows and the far move
//   page_peaks      a lane per character
//   host            page_workspace_bytes, forced_check_pages (every refusal of the entries' loop over pages)
// C, a struct per file, is the cell of page_fill: line (a line's own set-up), leave (the first half of a line boundary:
// the old window's values into vbuf, and what else the cell hands on), seed (frame 0 of the page), step<kFirst> (a frame
// for a lane's K states, kFirst: frame 0 of a line behind the first) and stored (after a frame's moves are stored).
// page_walk stages its blocks in a loop of its own, not through stage_moves: as a call K = 32 unrolls it and the page is
// slower (profiles/forced_refactor.txt).  What each kernel's instruction stream made of these pieces:
// profiles/forced_page_shared.txt.
#pragma once
#include "forced_common.h"

namespace {

constexpr long long kDead = -(1ll << 49);              // a page whose best end lies below has no path
constexpr int kMaxText = 1 << 29;                      // strict: the states 0 .. 2 n stay inside an int
constexpr int kMaxChars = 1 << 20;                     // with omission: omit * n + 2^21 * frames < 2^48, nothing nears kDead
constexpr int64_t kMaxFrames = 1ll << 25;

struct PageArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int64_t* line_first; const int32_t* lo;
    const int32_t* hi; const int32_t* labels; const int64_t* lab_off; const int64_t* ws_off;
    int32_t npages, nlines, no, variants; int64_t rows, nlabels;
    unsigned char* ws; int64_t ws_bytes;
    int32_t* frames; int64_t* score; int32_t* status;
    int32_t omit;                                      // the price of a character in units of 2^-16 bit; strict: 0
};

// what the gated instantiations take on top (ta_forced_align_pages_gated, DESIGN.md section 14.14, and
// ta_forced_align_pages_omit_gated, section 14.17): per page a reason that lets the page pass (0) or not, and the widest
// window the host sized the workspace for.  Not fields of PageArgs: they would move the kernel arguments of the other page
// kernels, and their instruction streams with them.  Defined here, once, for the two headers that hold a gated kernel
// (forced_page_strict.h, forced_page_omit.h)
struct GatedPageArgs : PageArgs {
    const int32_t* gate; const int32_t* cap;
};

// the variant of a window of w characters
__host__ __device__ inline int window_k(int w) { return forced_k(2 * w + 1); }

// ---- the prologue ----------------------------------------------------------------------------------------------------------

struct PageHead {
    int64_t l0, c0;            // the page's first line and first label
    int nl, n;                 // its lines and characters
    const int32_t* cs;         // its labels
    int KP;                    // its variant, from the device's windows
};

// Every bound the kernel relies on, on the page's own numbers (the host checked its copies as well): false where block b
// has nothing (more) to do, a refused page's status written.  max_chars: the cap on the page's text; rows_of(T, K): the
// 256-byte rows of a line's workspace piece; over(frames): what the kernel alone refuses, asked the lane's share of the
// page's frames, wave-uniform and asked only of a page that passed so far.  A page that fails the checks, or whose
// variant no launch of this call covers, is refused by every launch alike; behind it the kernel leaves at once unless the
// page is its variant's (h.KP != K) and checks the labels (labels_ok): with those two inside, the strict kernels park 50
// more scalars in VGPR lanes.  All of this is over before the fill's registers are live.
// kPerPage (ta_forced_page_conf.hip): the workspace is ONE piece per page, ws_off [npages], of 256 * rows_of(n, KP) bytes.
template <bool kPerPage = false, class Rows, class Over>
__device__ __forceinline__ bool page_head(const PageArgs& a, int b, int lane, int max_chars, Rows rows_of, Over over,
                                          PageHead& h) {
    auto refuse = [&](int status) {
        if (lane == 0) a.status[b] = status;
        return false;
    };
    const int no = a.no;
    const int64_t l0 = a.line_first[b], l1 = a.line_first[b + 1], c0 = a.lab_off[b], c1 = a.lab_off[b + 1];
    bool ok = no >= 2 && no <= kMaxNo && l0 >= 0 && l0 < l1 && l1 <= a.nlines && c0 >= 0 && c0 < c1 && c1 <= a.nlabels &&
              c1 - c0 <= max_chars;
    if (!ok) return refuse(TA_FORCED_BOUNDS);          // wave-uniform
    const int nl = (int)(l1 - l0), n = (int)(c1 - c0);
    bool bad = false;
    int kmine = 2;
    long long tsum = 0;
    for (int k = lane; k < nl; k += 64) {
        const int64_t q = l0 + k;
        const int T = a.T[q], lo = a.lo[q], hi = a.hi[q];
        const int64_t r0 = a.row_off[q];
        bad |= T < 1 || T > TA_TRAIN_MAX_T || r0 < 0 || r0 + T > a.rows || lo < 0 || hi < lo || hi > n ||
               hi - lo > TA_FORCED_MAX_TARGET;
        if (k == 0) bad |= lo != 0;
        if (k == nl - 1) bad |= hi != n;
        if (k + 1 < nl) {
            const int lo2 = a.lo[q + 1], hi2 = a.hi[q + 1];
            bad |= lo2 < lo || lo2 > hi || hi2 < hi;
        }
        if (!bad) {
            const int kw = window_k(hi - lo);
            kmine = kw > kmine ? kw : kmine;
            tsum += T;
        }
    }
    if (__any(bad)) return refuse(TA_FORCED_BOUNDS);
    const int KP = __any(kmine == 32) ? 32 : __any(kmine == 16) ? 16 : __any(kmine == 8) ? 8 : __any(kmine == 4) ? 4 : 2;
    if (kPerPage) {
        const int64_t w0 = a.ws_off[b];
        bad |= w0 < 0 || (w0 & 15) != 0 || w0 + 256 * rows_of(n, KP) > a.ws_bytes;
    } else {
        for (int k = lane; k < nl; k += 64) {          // the lines' workspace pieces, sized by the page's variant
            const int64_t w0 = a.ws_off[l0 + k];
            bad |= w0 < 0 || (w0 & 15) != 0 || w0 + 256 * rows_of(a.T[l0 + k], KP) > a.ws_bytes;
        }
    }
    if (__any(bad) || over(tsum) || (a.variants & variant_bit(KP)) == 0) return refuse(TA_FORCED_BOUNDS);
    h.l0 = l0; h.c0 = c0; h.nl = nl; h.n = n; h.cs = a.labels + c0; h.KP = KP;
    return true;
}

// ---- the fill --------------------------------------------------------------------------------------------------------------

// The fill of a page, line after line; vlast: the last frame's values, in the window of the last line, whose lo it returns.
//   chunks    Feed's chunks of kChunk frames restart with every line; the chunk ahead of a line's last one is the next
//             line's first, and the LDS buffers go on taking turns (g).
//   boundary  the cell masks the old window's values into vbuf, indexed by the OLD window's state (cell.leave); they come
//             back shifted by d = 2 (lo_{k+1} - lo_k), states outside the old window NEG.  The state in front of the new
//             window, if the old one held it, is what lane 0 takes from its left in the first frame (edge).  The lane's
//             labels and skip bits are loaded again, and the first frame of the line runs step<true>.
//   moves     per line through store_moves, at the line's own piece of the workspace.
template <int K, class C>
__device__ __forceinline__ int page_fill(const PageArgs& a, const PageHead& h, int lane, int* qtab, long long* vbuf,
                                         long long (&vlast)[K], C& cell) {
    long long v[K];                                    // the fill's own: values a caller owns cost K = 8 a wave
    const int no = a.no, nl = h.nl;
    const int64_t l0 = h.l0;
    int lab[K / 2];                                    // labels per lane
    unsigned skip = 0;                                 // bit j: label j may be reached over the blank in front of it
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;
    Feed<int> feed(qtab, no, lane);
    int T = __builtin_amdgcn_readfirstlane(a.T[l0]);
    const float* P = a.probs + a.row_off[l0] * no;
    feed.prefetch(P, T, 0);
    int g = 0;                                         // chunks so far: the LDS buffer in turn
    int lo_old = 0, hi_old = 0;
    for (int k = 0; k < nl; ++k) {
        const int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]), hi = __builtin_amdgcn_readfirstlane(a.hi[l0 + k]);
        uint32_t* moves = reinterpret_cast<uint32_t*>(a.ws + a.ws_off[l0 + k]);
        cell.line(moves, T);
        long long edge = kNeg;
        const int d = 2 * (lo - lo_old);               // old window states in front of the new window
        if (k > 0) {                                   // from the old window's lanes and registers to the new one's
            cell.leave(v, 2 * (hi_old - lo_old), vbuf);
            wave_lds_sync();
            if (d >= 1) edge = vbuf[d - 1];            // d - 1 < wold: lo <= hi_old
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r + d;
                v[r] = j < 64 * K ? vbuf[j] : kNeg;
            }
        }
        skip = lane_labels(h.cs, lo, hi, lane, lab);
        // the line behind, for the chunk ahead of this line's last
        const bool more = k + 1 < nl;
        const int Tn = more ? __builtin_amdgcn_readfirstlane(a.T[l0 + k + 1]) : 0;
        const float* Pn = more ? a.probs + a.row_off[l0 + k + 1] * no : P;
        const int nchunks = (T + kChunk - 1) / kChunk;
        uint32_t acc = 0;
        for (int c = 0; c < nchunks; ++c, ++g) {
            const int* qbuf = feed.publish(g, emission_q);
            if (c + 1 < nchunks) feed.prefetch(P, T, c + 1);
            else feed.prefetch(Pn, Tn, 0);
            wave_lds_sync();
            const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
            for (int t = t0; t < t1; ++t) {
                const int* q = qbuf + (t - t0) * no;
                const int qb = q[0];
                unsigned long long mv = 0;
                if (t == 0) {
                    if (k == 0) cell.seed(v, lab, q, qb);
                    else mv = cell.template step<true>(v, from_left(v[K - 1], edge), skip, lab, q, qb, d);
                } else {
                    mv = cell.template step<false>(v, from_left(v[K - 1], kNeg), skip, lab, q, qb, 0);
                }
                store_moves<K>(moves, t, T, lane, mv, acc);
                cell.stored(t, T);
            }
        }
        lo_old = lo;
        hi_old = hi;
        P = Pn;
        T = Tn;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) vlast[k] = v[k];
    return lo_old;
}

// ---- the walk and the peaks ------------------------------------------------------------------------------------------------

// Back through the lines from page state s, wave-uniform, the moves of kWalk frames at a time through LDS (kOmit: and the
// bit rows behind them).  Lane 0 writes line / t_first / t_last when the path leaves a character's state.  kOmit: a far
// move (code 3) reads its frame's bit row -- frame 0 of a line k >= 1: in the PREVIOUS line's window coordinates -- and the
// characters it jumps are not written.  Between the fill's fence and the peaks'.
template <int K, bool kOmit>
__device__ __forceinline__ void page_walk(const PageArgs& a, uint32_t* stage, int64_t l0, int nl, int s, int32_t* frames,
                                          int lane) {
    constexpr int SPB = 32 / K;                        // frames per bit word
    constexpr int RPB = walk_rows(K);                  // move rows per walk block
    constexpr int BPB = kWalk / SPB;                   // bit rows per walk block
    int last = 0;
    bool inside = false;                               // the frame behind was spent in the same state
    for (int k = nl - 1; k >= 0 && s >= 0; --k) {
        const int Tk = __builtin_amdgcn_readfirstlane(a.T[l0 + k]), lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]);
        const int lo_prev = kOmit && k > 0 ? __builtin_amdgcn_readfirstlane(a.lo[l0 + k - 1]) : 0;
        const uint32_t* moves = reinterpret_cast<const uint32_t*>(a.ws + a.ws_off[l0 + k]);
        const int64_t nrows = forced_ws_rows(Tk, K), nbrows = omit_bit_rows(Tk, K);
        const uint32_t* bitrows = moves + nrows * 64;
        int base = -1;
        for (int t = Tk - 1; t >= 0 && s >= 0; --t) {
            if ((t & ~(kWalk - 1)) != base) {
                base = t & ~(kWalk - 1);
                __syncthreads();
                // stage_moves<K>, spelled out: as a call K = 32 unrolls it and the page is slower
                const int64_t g0 = K == 32 ? 2 * (int64_t)base : base / steps_per_word(K), b0 = base / SPB;
                for (int r = 0; r < RPB && g0 + r < nrows; ++r) stage[r * 64 + lane] = moves[(g0 + r) * 64 + lane];
                if (kOmit)
                    for (int r = 0; r < BPB && b0 + r < nbrows; ++r) stage[(RPB + r) * 64 + lane] = bitrows[(b0 + r) * 64 + lane];
                __syncthreads();
            }
            const int w = s - 2 * lo;                  // the state in the line's window
            if (w < 0 || w >= 64 * K) { s = -1; break; }               // never on a path that the fill found
            const int tt = t - base;
            unsigned m = staged_move<K>(stage, tt, w / K, w % K);
            if (t == 0 && k == 0) m = 1;               // the path starts here: whatever state this is, it is left
            if ((s & 1) && !inside) last = t;
            if ((s & 1) && m != 0 && lane == 0) {
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1)] = k;
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1) + 1] = t;
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1) + 2] = last;
            }
            inside = m == 0;
            if (kOmit && m == 3) {                     // far: down the bit row from 2 i - 2 to the first set bit
                const int from = t == 0 ? lo_prev : lo;                 // the window the bit row was written in
                int x = 2 * (w >> 1) - 2 + 2 * (lo - from);
                if (x < 0) { s = -1; break; }
                x = x < 64 * K ? x : 64 * K - 1;
                const int ws = far_source<K>(stage + RPB * 64, tt, x, lane);
                if (ws < 0) { s = -1; break; }
                s = 2 * from + ws;
            } else {
                s -= (int)m;
            }
        }
    }
}

// a lane per character scans its few frames for the first largest q.  A row the walk did not give a line and frames of
// that line: strict, t_peak = t_first; kOmit, the row is left alone (a character the path never entered keeps its -1)
template <bool kOmit>
__device__ __forceinline__ void page_peaks(const PageArgs& a, const PageHead& h, int32_t* frames, int lane) {
    for (int i = lane; i < h.n; i += 64) {
        const int k = frames[TA_FORCED_PAGE_FIELDS * i], tf = frames[TA_FORCED_PAGE_FIELDS * i + 1],
                  tl = frames[TA_FORCED_PAGE_FIELDS * i + 2], c = h.cs[i];
        const bool in = k >= 0 && k < h.nl && tf >= 0 && tl < a.T[h.l0 + k];
        if (kOmit && (!in || tl < tf)) continue;
        frames[TA_FORCED_PAGE_FIELDS * i + 3] = in ? peak_frame(a.probs + a.row_off[h.l0 + k] * a.no, a.no, c, tf, tl) : tf;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// the body of a *_workspace_bytes(nl, T, K) function: rows_of(T, K) rows of 256 bytes per line, -1 where there is no answer
template <class Rows>
inline int64_t page_workspace_bytes(int32_t nl, const int32_t* T, int32_t K, Rows rows_of) {
    if (nl < 1 || !T || !(K == 2 || K == 4 || K == 8 || K == 16 || K == 32)) return -1;
    int64_t total = 0;
    for (int k = 0; k < nl; ++k) {
        if (T[k] < 1 || T[k] > TA_TRAIN_MAX_T) return -1;
        total += 256 * rows_of(T[k], K);
    }
    return total;
}

// The host's copies of a page list, behind forced_preamble: the pages inside nlines and nlabels, every page with lines and
// a text of at most max_chars characters (max_chars_msg: the refusal beyond), every line and window inside the limits, the
// windows in reading order without a gap, at most max_frames frames per page (max_frames_msg), the lines inside rows and
// the workspace, whose pieces are rows_of(T, the page's variant) rows (ws_name: the exported function that tells a caller so).
// *variants: a bit per K to launch.
template <class Rows>
inline int forced_check_pages(const int32_t* T_host, const int64_t* line_first_host, const int32_t* lo_host,
                              const int32_t* hi_host, const int64_t* lab_off_host, int npages, int nlines, int64_t rows,
                              int64_t nlabels, int64_t workspace_bytes, Rows rows_of, int64_t max_chars,
                              const char* max_chars_msg, int64_t max_frames, const char* max_frames_msg, const char* ws_name,
                              int* variants) {
    if (line_first_host[0] != 0 || line_first_host[npages] != nlines) return ta_fail(TA_EINVAL, "line_first does not run from 0 to nlines");
    if (lab_off_host[0] < 0 || lab_off_host[npages] > nlabels) return ta_fail(TA_EINVAL, "the pages' texts exceed nlabels");
    int64_t need = 0, sum_t = 0;
    *variants = 0;
    for (int p = 0; p < npages; ++p) {
        const int64_t l0 = line_first_host[p], l1 = line_first_host[p + 1], n = lab_off_host[p + 1] - lab_off_host[p];
        if (l1 <= l0) return ta_fail(TA_EINVAL, "a page without lines");
        if (n < 1) return ta_fail(TA_EINVAL, "a page without text");
        if (n > max_chars) return ta_fail(TA_ELIMIT, max_chars_msg);
        int kp = 2;
        int64_t page_t = 0;
        for (int64_t q = l0; q < l1; ++q) {
            const int t = T_host[q], a = lo_host[q], b = hi_host[q];
            if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
            if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
            if (a < 0 || b < a || b > n) return ta_fail(TA_EINVAL, "a window outside its page's text");
            if (q == l0 && a != 0) return ta_fail(TA_EINVAL, "the first window does not start at the text's start");
            if (q == l1 - 1 && b != n) return ta_fail(TA_EINVAL, "the last window does not end at the text's end");
            if (q + 1 < l1 && (lo_host[q + 1] < a || lo_host[q + 1] > b || hi_host[q + 1] < b))
                return ta_fail(TA_EINVAL, "windows must move forwards and leave no character out");
            if (b - a > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a window of more than TA_FORCED_MAX_TARGET characters");
            const int kw = window_k(b - a);
            kp = kw > kp ? kw : kp;
            page_t += t;
        }
        if (page_t > max_frames) return ta_fail(TA_ELIMIT, max_frames_msg);
        sum_t += page_t;
        for (int64_t q = l0; q < l1; ++q) need += 256 * rows_of(T_host[q], kp);
        *variants |= variant_bit(kp);
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (workspace_bytes < need) return forced_ws_small("pages", ws_name);
    return TA_OK;
}

}  // namespace
