// ta_forced_page_omit.hip -- page-scope forced alignment whose path may OMIT characters of the text at a price per
// character: ONE best path through the frames of all the lines of a page (section 14.8) on the
// lattice with the far move (section 14.9), so that a character the scribe never wrote takes no frame from its
// neighbours, on its own line or across a line break.  Integers only from the float32 probabilities on; the checker of
// record is tests/forced_page_omit_ref.py.
//
// forced_page_omit_kernel<K>, one wave per page, laid out as forced_page_kernel<K>: lane l holds the WINDOW states
// l K .. l K + K - 1 (page state minus 2 lo_k) as int64, K from the page's widest window, one launch per variant.
//   fill    Feed, the chunks that restart with every line, store_moves and the re-basing through vbuf are the strict page
//           kernel's; the cell is the upward cell of the line kernel with omission (wave_max_scan, two from_left shifts,
//           a bit word per frame, move code 3 = far), with a[x] = v[x] + omit * ceil(x / 2) formed in WINDOW coordinates:
//           a window starts at an even page state, so another window's coordinates add the same omit * d to both sides
//           of every comparison.
//   break   the first frame of a line k >= 1 takes its far candidates from the OLD window, the 2 (lo_k - lo_{k-1}) states
//           that fall off the front included.  Before the re-basing the old registers are masked to the old window and
//           scanned in old coordinates; that scan's bits are the line's bit row of frame 0, and its prefix maxima Pm go
//           through LDS beside v (pbuf).  The first frame's state of window character i reads Pm[2 i + d - 2] - omit *
//           (i + d / 2), d = 2 (lo_k - lo_{k-1}), and a label state has no stay candidate.
//   start   every state of window 0 may start the path, the characters in front paid for.
//   end     fin[s] = v[s] - omit * (n - ceil(s / 2)) over s <= 2 n of the last window, the largest, the largest s on a
//           tie: every lane's best goes through LDS and every lane reads all 64.
//   walk    wave-uniform, back through the lines, moves and bits of kWalk frames at a time through LDS.  The frames are
//           set to -1 before the fill; a far move reads its frame's bit row (frame 0 of a line k >= 1: in the PREVIOUS
//           line's window coordinates) and the characters it jumps keep the -1.
//   peak    a lane per character; a row that still holds -1 is left alone.
// Workspace of line k: forced_ws_rows(T_k, K) rows of 64 move words, then omit_bit_rows(T_k, K) rows of 64 bit words as
// ta_forced_omit.hip lays them out; frame 0's bits are the boundary scan's, so the first-frame bit row needs no room of its
// own.  256-byte rows, plain vector stores.
// Limits: n <= 2^20 characters and at most 2^25 frames per page, so omit * n + 2^21 * frames < 2^48 and nothing approaches
// -2^49; under the rule every page has a path (the checker's docstring), TA_FORCED_NOPATH is kept for a score below -2^49
// all the same.  Every bound is re-checked on the page's own device numbers before anything is read through it; a refused
// page gets a status and touches nothing else.
// All five variants are built; K = 32 holds its values in 256 VGPRs and 126 AGPRs and 57 KiB of LDS, without scratch.
#include "forced_common.h"

namespace {

constexpr long long kDead = -(1ll << 49);
constexpr int kMaxChars = 1 << 20;
constexpr int64_t kMaxFrames = 1ll << 25;

struct PageOmitArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int64_t* line_first; const int32_t* lo;
    const int32_t* hi; const int32_t* labels; const int64_t* lab_off; const int64_t* ws_off;
    int32_t npages, nlines, no, variants, omit; int64_t rows, nlabels;
    unsigned char* ws; int64_t ws_bytes;
    int32_t* frames; int64_t* score; int32_t* status;
};

__host__ __device__ inline int window_k(int w) { return forced_k(2 * w + 1); }
__host__ __device__ inline int64_t page_omit_rows(int T, int K) { return forced_ws_rows(T, K) + omit_bit_rows(T, K); }

// One frame for a lane's K states, upwards (o1 and o2 carry the old row's v[k - 1] and v[k - 2]): stay / advance / skip /
// far, ties in that order.  A frame inside a line scans a[] and notes its bits; kFirst, the first frame of a line behind
// the page's first, takes the far candidates from pbuf, the old window's prefix maxima (d: old window states in front of
// the new window, dch = d / 2), and gives a label state no stay candidate.
template <int K, bool kFirst>
__device__ __forceinline__ unsigned long long page_omit_step(long long (&v)[K], long long left, unsigned skip,
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

// the far move's source: the first set bit at or below state x of the staged bit row (tt: the frame in the block)
template <int K>
__device__ __forceinline__ int far_source(const uint32_t* bitstage, int tt, int x, int lane) {
    constexpr int SPB = 32 / K;
    const int lx = x / K, kx = x % K, sh = (K * (tt % SPB)) & 31;
    const uint32_t* row = bitstage + (tt / SPB) * 64;
    uint32_t w = (row[lane] >> sh) & (uint32_t)((1ull << K) - 1);
    if (lane > lx) w = 0;
    if (lane == lx) w &= (uint32_t)((2ull << kx) - 1);
    const unsigned long long has = __ballot(w != 0);
    if (has == 0) return -1;                           // cannot happen: the window's first state is always finite
    const int lt = 63 - __builtin_clzll(has);
    uint32_t wt = (row[lt] >> sh) & (uint32_t)((1ull << K) - 1);
    if (lt == lx) wt &= (uint32_t)((2ull << kx) - 1);
    return lt * K + 31 - __builtin_clz(wt);
}

template <int K>
__global__ __launch_bounds__(64) void forced_page_omit_kernel(PageOmitArgs a) {
    constexpr int H = K / 2;                           // labels per lane
    constexpr int SPB = 32 / K;                        // frames per bit word
    constexpr int RPB = walk_rows(K);                  // move rows per walk block
    constexpr int BPB = kWalk / SPB;                   // bit rows per walk block
    constexpr int kWords = (RPB + BPB) * 64 > 2 * kChunk * kMaxNo ? (RPB + BPB) * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long pbuf[64 * K];                 // ... and the old window's prefix maxima of a[]
    __shared__ long long fin_v[64];
    __shared__ int fin_s[64];
    int* qtab = reinterpret_cast<int*>(stage);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int no = a.no;
    const long long omit = a.omit;

    // ---- every bound the kernel relies on, on the page's own numbers -------------------------------------------------------
    const int64_t l0 = a.line_first[b], l1 = a.line_first[b + 1], c0 = a.lab_off[b], c1 = a.lab_off[b + 1];
    bool ok = a.omit >= 0 && a.omit <= TA_FORCED_OMIT_MAX && no >= 2 && no <= kMaxNo && l0 >= 0 && l0 < l1 &&
              l1 <= a.nlines && c0 >= 0 && c0 < c1 && c1 <= a.nlabels && c1 - c0 <= kMaxChars;
    if (!ok) {                                         // wave-uniform
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    const int nl = (int)(l1 - l0), n = (int)(c1 - c0);
    bool bad = false;
    int kmine = 2;
    long long tsum = 0;
    for (int k = lane; k < nl; k += 64) {
        const int64_t q = l0 + k;
        const int T = a.T[q], lo = a.lo[q], hi = a.hi[q];
        const int64_t r0 = a.row_off[q];
        bad |= T < 1 || T > TA_TRAIN_MAX_T || r0 < 0 || r0 + T > a.rows || lo < 0 || hi < lo || hi > n || hi - lo > TA_FORCED_MAX_TARGET;
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
    if (__any(bad)) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    fin_v[lane] = tsum;
    __syncthreads();
    long long frames_all = 0;
    for (int l = 0; l < 64; ++l) frames_all += fin_v[l];
    __syncthreads();
    const int KP = __any(kmine == 32) ? 32 : __any(kmine == 16) ? 16 : __any(kmine == 8) ? 8 : __any(kmine == 4) ? 4 : 2;
    for (int k = lane; k < nl; k += 64) {              // the lines' workspace pieces, sized by the page's variant
        const int64_t w0 = a.ws_off[l0 + k];
        bad |= w0 < 0 || (w0 & 15) != 0 || w0 + 256 * page_omit_rows(a.T[l0 + k], KP) > a.ws_bytes;
    }
    if (__any(bad) || frames_all > kMaxFrames || (a.variants & variant_bit(KP)) == 0) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (KP != K) return;                               // wave-uniform: the page belongs to another launch of this call
    const int32_t* cs = a.labels + c0;
    if (!labels_ok(cs, n, no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    int32_t* frames = a.frames + TA_FORCED_PAGE_FIELDS * c0;
    for (int64_t i = lane; i < (int64_t)TA_FORCED_PAGE_FIELDS * n; i += 64) frames[i] = TA_FORCED_OMITTED;

    // ---- fill -------------------------------------------------------------------------------------------------------------
    const long long pen0 = omit * (long long)(lane * H);               // omit * (the lane's first window character)
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
        uint32_t* bitrows = moves + forced_ws_rows(T, K) * 64;
        long long edge = kNeg;
        uint32_t bits0 = 0;                            // the bits of the line's frame 0: the scan of the old window
        const int d = 2 * (lo - lo_old);
        if (k > 0) {                                   // from the old window's lanes and registers to the new one's
            const int wold = 2 * (hi_old - lo_old);
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
        uint32_t acc = 0, accb = 0;
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
                uint32_t bits = 0;
                if (t == 0) {
                    if (k == 0) {                      // every state may start the path: the characters in front are paid for
#pragma unroll
                        for (int r = 0; r < K; ++r) v[r] = (long long)((r & 1) ? q[lab[r >> 1]] : qb) - (pen0 + omit * (r >> 1));
                    } else {
                        bits = bits0;
                        mv = page_omit_step<K, true>(v, from_left(v[K - 1], edge), skip, lab, q, qb, omit, pen0, lane, pbuf, d,
                                                     bits);
                    }
                } else {
                    mv = page_omit_step<K, false>(v, from_left(v[K - 1], kNeg), skip, lab, q, qb, omit, pen0, lane, pbuf, 0,
                                                  bits);
                }
                store_moves<K>(moves, t, T, lane, mv, acc);
                accb |= bits << ((K * (t % SPB)) & 31);
                if (t % SPB == SPB - 1 || t == T - 1) {
                    bitrows[(int64_t)(t / SPB) * 64 + lane] = accb;
                    accb = 0;
                }
            }
        }
        lo_old = lo;
        hi_old = hi;
        P = Pn;
        T = Tn;
    }

    // ---- end: the largest fin over the last window's states up to 2 n, the largest s on a tie ----------------------------
    {
        long long bv = kNeg * 2;
        int bs = -1;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int s = 2 * lo_old + lane * K + r;
            const long long f = v[r] - omit * (long long)(n - ((s + 1) >> 1));
            if (s <= 2 * n && f >= bv) { bv = f; bs = s; }
        }
        fin_v[lane] = bv;
        fin_s[lane] = bs;
    }
    __threadfence();                                   // the moves, the bits and the -1 frames are read back below
    __syncthreads();
    long long best = kNeg * 2;
    int s = -1;
    for (int l = 0; l < 64; ++l) {
        const long long f = fin_v[l];
        if (fin_s[l] >= 0 && f >= best) { best = f; s = fin_s[l]; }
    }
    if (best < kDead || s < 0) {                       // wave-uniform; cannot happen within the limits
        if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
        return;
    }

    // ---- walk: wave-uniform, line after line backwards, moves and bits of kWalk frames at a time through LDS ------------
    const uint32_t* bitstage = stage + RPB * 64;
    int last = 0;
    bool inside = false;                               // the frame behind was spent in the same state
    for (int k = nl - 1; k >= 0 && s >= 0; --k) {
        const int Tk = __builtin_amdgcn_readfirstlane(a.T[l0 + k]), lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]);
        const int lo_prev = k > 0 ? __builtin_amdgcn_readfirstlane(a.lo[l0 + k - 1]) : 0;
        const uint32_t* moves = reinterpret_cast<const uint32_t*>(a.ws + a.ws_off[l0 + k]);
        const int64_t nrows = forced_ws_rows(Tk, K), nbrows = omit_bit_rows(Tk, K);
        const uint32_t* bitrows = moves + nrows * 64;
        int base = -1;
        for (int t = Tk - 1; t >= 0 && s >= 0; --t) {
            if ((t & ~(kWalk - 1)) != base) {
                base = t & ~(kWalk - 1);
                __syncthreads();
                const int64_t g0 = K == 32 ? 2 * (int64_t)base : base / steps_per_word(K), b0 = base / SPB;
                for (int r = 0; r < RPB && g0 + r < nrows; ++r) stage[r * 64 + lane] = moves[(g0 + r) * 64 + lane];
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
            if (m == 3) {                              // far: down the bit row from 2 i - 2 to the first set bit
                const int from = t == 0 ? lo_prev : lo;                 // the window the bit row was written in
                int x = 2 * (w >> 1) - 2 + 2 * (lo - from);
                if (x < 0) { s = -1; break; }
                x = x < 64 * K ? x : 64 * K - 1;
                const int ws = far_source<K>(bitstage, tt, x, lane);
                if (ws < 0) { s = -1; break; }
                s = 2 * from + ws;
            } else {
                s -= (int)m;
            }
        }
    }
    __threadfence();
    __syncthreads();

    // ---- peak: a lane per character; one the path never entered keeps its -1 -----------------------------------------------
    for (int i = lane; i < n; i += 64) {
        const int k = frames[TA_FORCED_PAGE_FIELDS * i], tf = frames[TA_FORCED_PAGE_FIELDS * i + 1],
                  tl = frames[TA_FORCED_PAGE_FIELDS * i + 2], c = cs[i];
        if (k < 0 || k >= nl || tf < 0 || tl < tf || tl >= a.T[l0 + k]) continue;
        frames[TA_FORCED_PAGE_FIELDS * i + 3] = peak_frame(a.probs + a.row_off[l0 + k] * no, no, c, tf, tl);
    }
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

}  // namespace

extern "C" int64_t ta_forced_page_omit_workspace_bytes(int32_t nl, const int32_t* T, int32_t K) {
    if (nl < 1 || !T || !(K == 2 || K == 4 || K == 8 || K == 16 || K == 32)) return -1;
    int64_t total = 0;
    for (int k = 0; k < nl; ++k) {
        if (T[k] < 1 || T[k] > TA_TRAIN_MAX_T) return -1;
        total += 256 * page_omit_rows(T[k], K);
    }
    return total;
}

extern "C" int ta_forced_align_pages_omit(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                                          const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                                          const int64_t* ws_off, int32_t npages, int32_t nlines, int32_t no, int64_t rows,
                                          int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                                          const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host,
                                          int32_t omit_q, void* workspace, int64_t workspace_bytes, int32_t* frames,
                                          int64_t* score, int32_t* status, void* stream) {
    bool go;
    const int rc = forced_preamble(npages < 0 || nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no,
                                   omit_q < 0 || omit_q > TA_FORCED_OMIT_MAX ? "omit_q outside 0 .. TA_FORCED_OMIT_MAX" : nullptr,
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
        if (n > kMaxChars) return ta_fail(TA_ELIMIT, "a page's text has more than 2^20 characters");
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
        if (page_t > kMaxFrames) return ta_fail(TA_ELIMIT, "a page has more than 2^25 frames");
        sum_t += page_t;
        for (int64_t q = l0; q < l1; ++q) need += 256 * page_omit_rows(T_host[q], kp);
        variants |= variant_bit(kp);
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (workspace_bytes < need) return forced_ws_small("pages", "ta_forced_page_omit_workspace_bytes");
    const PageOmitArgs a{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, omit_q,
                         rows, nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_omit_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_omit_kernel launch");
    return TA_OK;
}
