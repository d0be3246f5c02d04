// ta_forced_page.hip -- page-scope forced alignment: ONE best CTC path through the frames of all
// the lines of a page, so that the lattice, not the decoder's output, decides which transcript character lies on which
// line.  Integers only from the float32 probabilities on; the checker of record is tests/forced_page_ref.py.
//
// forced_page_kernel<K>, one wave per page: the page is one chain of dependent steps.  The page's labels give the states
// 0 .. 2 n; during the frames of line k only the states of its window of characters [lo_k, hi_k) are live, 2 lo_k ..
// 2 hi_k.  Lane l holds the K consecutive WINDOW states l K .. l K + K - 1 (page state minus 2 lo_k) as int64 registers;
// K = 2 .. 32 from the page's widest window (forced_k), even, and a window starts at an even page state, so blanks stay
// in even registers whatever the window.
//   fill   the cell is forced_step, the hand-over of one int64 per step from_left and the emission table Feed (chunks of
//          kChunk frames a chunk ahead through two LDS buffers, no barrier).  Chunks restart with every line; the chunk
//          ahead of a line's last one is the next line's first.  At a line boundary the values go through an LDS buffer
//          indexed by the OLD window's state and come back shifted by 2 (lo_{k+1} - lo_k); states outside the old window
//          read NEG.  The state in front of the new window, if the old one held it, is what lane 0 takes from its left in
//          the first frame.  The lane's labels and skip bits are loaded again (lane_labels on the window), and the first
//          frame of the line runs the step in which a label state has no stay candidate (kFirst): no character spans a
//          line break.  Registers beyond the window's last state hold values no live state ever reads (a state depends on
//          lower states only) and are masked at the next boundary.  A state without a live source drifts below NEG
//          instead of staying there; it can never reach a state with a path (a path costs less than 2^21 per frame), and
//          its moves are never walked.
//   moves  per line through store_moves, forced_ws_rows(T_k, K) rows of 64 words at the line's own piece.
//   walk   back through the lines from the better of the last two states, in page coordinates, the moves in blocks of
//          kWalk frames through LDS (staged_move).  Lane 0 writes line / t_first / t_last when the path leaves a
//          character's state.
//   peak   a lane per character scans its few frames for the first largest q (peak_frame).
// A page whose best end is below -2^49 has no path: TA_FORCED_NOPATH, nothing but its status is written.  Every bound is
// re-checked on the page's own device numbers before anything is read through it.
#include "forced_common.h"

namespace {

constexpr long long kDead = -(1ll << 49);

struct PageArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int64_t* line_first; const int32_t* lo;
    const int32_t* hi; const int32_t* labels; const int64_t* lab_off; const int64_t* ws_off;
    int32_t npages, nlines, no, variants; int64_t rows, nlabels;
    unsigned char* ws; int64_t ws_bytes;
    int32_t* frames; int64_t* score; int32_t* status;
};

// the variant of a window of w characters
__host__ __device__ inline int window_k(int w) { return forced_k(2 * w + 1); }

template <int K>
__global__ __launch_bounds__(64) void forced_page_kernel(PageArgs a) {
    constexpr int H = K / 2;                           // labels per lane
    constexpr int kWords = walk_rows(K) * 64 > 2 * kChunk * kMaxNo ? walk_rows(K) * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long vend[2];
    int* qtab = reinterpret_cast<int*>(stage);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int no = a.no;

    // ---- every bound the kernel relies on, on the page's own numbers -------------------------------------------------------
    const int64_t l0 = a.line_first[b], l1 = a.line_first[b + 1], c0 = a.lab_off[b], c1 = a.lab_off[b + 1];
    bool ok = no >= 2 && no <= kMaxNo && l0 >= 0 && l0 < l1 && l1 <= a.nlines && c0 >= 0 && c0 < c1 && c1 <= a.nlabels &&
              c1 - c0 <= (1 << 29);
    if (!ok) {                                         // wave-uniform
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    const int nl = (int)(l1 - l0), n = (int)(c1 - c0);
    bool bad = false;
    int kmine = 2;
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
        }
    }
    if (__any(bad)) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    const int KP = __any(kmine == 32) ? 32 : __any(kmine == 16) ? 16 : __any(kmine == 8) ? 8 : __any(kmine == 4) ? 4 : 2;
    for (int k = lane; k < nl; k += 64) {              // the lines' workspace pieces, sized by the page's variant
        const int64_t w0 = a.ws_off[l0 + k];
        bad |= w0 < 0 || (w0 & 15) != 0 || w0 + 256 * forced_ws_rows(a.T[l0 + k], KP) > a.ws_bytes;
    }
    if (__any(bad) || (a.variants & variant_bit(KP)) == 0) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (KP != K) return;                               // wave-uniform: the page belongs to another launch of this call
    const int32_t* cs = a.labels + c0;
    if (!labels_ok(cs, n, no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }

    // ---- fill -------------------------------------------------------------------------------------------------------------
    int lab[H];
    unsigned skip = 0;                                 // bit j: label j may be reached over the blank in front of it
    long long v[K];
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
        long long edge = kNeg;
        if (k > 0) {                                   // from the old window's lanes and registers to the new one's
            const int d = 2 * (lo - lo_old), wold = 2 * (hi_old - lo_old);
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                vbuf[j] = j <= wold ? v[r] : kNeg;
            }
            wave_lds_sync();
            if (d >= 1) edge = vbuf[d - 1];            // d - 1 < wold: lo <= hi_old
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r + d;
                v[r] = j < 64 * K ? vbuf[j] : kNeg;
            }
        }
        skip = lane_labels(cs, lo, hi, lane, lab);
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
                    if (k == 0) {
                        if (lane == 0) { v[0] = qb; v[1] = q[lab[0]]; }
                    } else {
                        mv = forced_step<K, true>(v, from_left(v[K - 1], edge), skip, lab, q, qb);
                    }
                } else {
                    mv = forced_step<K, false>(v, from_left(v[K - 1], kNeg), skip, lab, q, qb);
                }
                store_moves<K>(moves, t, T, lane, mv, acc);
            }
        }
        lo_old = lo;
        hi_old = hi;
        P = Pn;
        T = Tn;
    }
    // the last window ends at the page's last state (hi = n): window state 2 (n - lo_old) is page state 2 n; the last
    // character's state lies in front of an empty last window and is not live then
    if (lane == 0) vend[0] = vend[1] = kNeg;
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = 2 * lo_old + lane * K + r;
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
    int s = e1 > e0 ? 2 * n - 1 : 2 * n;               // on a tie the last blank
    int32_t* frames = a.frames + TA_FORCED_PAGE_FIELDS * c0;

    // ---- walk: wave-uniform, line after line backwards, the moves of kWalk frames at a time through LDS ------------------
    int last = 0;
    bool inside = false;                               // the frame behind was spent in the same state
    for (int k = nl - 1; k >= 0 && s >= 0; --k) {
        const int Tk = __builtin_amdgcn_readfirstlane(a.T[l0 + k]), lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]);
        const uint32_t* moves = reinterpret_cast<const uint32_t*>(a.ws + a.ws_off[l0 + k]);
        const int64_t nrows = forced_ws_rows(Tk, K);
        int base = -1;
        for (int t = Tk - 1; t >= 0 && s >= 0; --t) {
            if ((t & ~(kWalk - 1)) != base) {
                base = t & ~(kWalk - 1);
                __syncthreads();
                // stage_moves<K>, spelled out: as a call K = 32 unrolls it and the page is slower
                const int64_t g0 = K == 32 ? 2 * (int64_t)base : base / steps_per_word(K);
                for (int r = 0; r < walk_rows(K) && g0 + r < nrows; ++r) stage[r * 64 + lane] = moves[(g0 + r) * 64 + lane];
                __syncthreads();
            }
            const int w = s - 2 * lo;                  // the state in the line's window
            if (w < 0 || w >= 64 * K) { s = -1; break; }               // never on a path that the fill found
            unsigned m = staged_move<K>(stage, t - base, w / K, w % K);
            if (t == 0 && k == 0) m = 1;               // the path starts here: whatever state this is, it is left
            if ((s & 1) && !inside) last = t;
            if ((s & 1) && m != 0 && lane == 0) {
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1)] = k;
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1) + 1] = t;
                frames[TA_FORCED_PAGE_FIELDS * (s >> 1) + 2] = last;
            }
            inside = m == 0;
            s -= (int)m;
        }
    }
    __threadfence();
    __syncthreads();

    // ---- peak: a lane per character ----------------------------------------------------------------------------------------
    for (int i = lane; i < n; i += 64) {
        const int k = frames[TA_FORCED_PAGE_FIELDS * i], tf = frames[TA_FORCED_PAGE_FIELDS * i + 1],
                  tl = frames[TA_FORCED_PAGE_FIELDS * i + 2], c = cs[i];
        const bool in = k >= 0 && k < nl && tf >= 0 && tl < a.T[l0 + k];
        frames[TA_FORCED_PAGE_FIELDS * i + 3] = in ? peak_frame(a.probs + a.row_off[l0 + k] * no, no, c, tf, tl) : tf;
    }
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

}  // namespace

extern "C" int64_t ta_forced_page_workspace_bytes(int32_t nl, const int32_t* T, int32_t K) {
    if (nl < 1 || !T || !(K == 2 || K == 4 || K == 8 || K == 16 || K == 32)) return -1;
    int64_t total = 0;
    for (int k = 0; k < nl; ++k) {
        if (T[k] < 1 || T[k] > TA_TRAIN_MAX_T) return -1;
        total += 256 * forced_ws_rows(T[k], K);
    }
    return total;
}

extern "C" int32_t ta_forced_page_variant(int32_t width) {
    if (width < 0 || width > TA_FORCED_MAX_TARGET) return -1;
    return window_k(width);
}

extern "C" int ta_forced_align_pages(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                                     const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                                     const int64_t* ws_off, int32_t npages, int32_t nlines, int32_t no, int64_t rows,
                                     int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                                     const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host,
                                     void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score,
                                     int32_t* status, void* stream) {
    bool go;
    const int rc = forced_preamble(npages < 0 || nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr,
                                   npages == 0,
                                   !probs || !row_off || !T || !line_first || !lo || !hi || !labels || !lab_off || !ws_off ||
                                       !T_host || !line_first_host || !lo_host || !hi_host || !lab_off_host || !workspace ||
                                       !frames || !score || !status,
                                   workspace, &go);
    if (!go) return rc;
    if (line_first_host[0] != 0 || line_first_host[npages] != nlines) return ta_fail(TA_EINVAL, "line_first does not run from 0 to nlines");
    if (lab_off_host[0] < 0 || lab_off_host[npages] > nlabels) return ta_fail(TA_EINVAL, "the pages' texts exceed nlabels");
    int64_t need = 0, sum_t = 0;
    int variants = 0;
    for (int p = 0; p < npages; ++p) {
        const int64_t l0 = line_first_host[p], l1 = line_first_host[p + 1], n = lab_off_host[p + 1] - lab_off_host[p];
        if (l1 <= l0) return ta_fail(TA_EINVAL, "a page without lines");
        if (n < 1) return ta_fail(TA_EINVAL, "a page without text");
        if (n > (1 << 29)) return ta_fail(TA_ELIMIT, "a page's text is too long");
        int kp = 2;
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
            sum_t += t;
        }
        for (int64_t q = l0; q < l1; ++q) need += 256 * forced_ws_rows(T_host[q], kp);
        variants |= variant_bit(kp);
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (workspace_bytes < need) return forced_ws_small("pages", "ta_forced_page_workspace_bytes");
    const PageArgs a{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                     nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_kernel launch");
    return TA_OK;
}
