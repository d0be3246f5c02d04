// ta_forced_page_post.hip -- sum-product posteriors at page scope and the page's likelihood: for
// a query frame (line, t) per character i of a page's text, the mass of ALL legal paths through ALL the lines of the page
// that spend that frame in the character's own state 2 i + 1, the largest such mass over the other live states with the
// state that has it, and per page the mass Z of all paths.  The lattice is ta_forced_page.hip's (windows that move from
// line to line, no character across a line break), the arithmetic ta_forced_post.hip's (forced_post_cells.h: pairs
// (double, int), every + and * rounded once); the checker of record is tests/forced_page_post_ref.py, and every word
// written here equals it bit for bit.  Built with -ffp-contract=off.
//
// forced_page_post_kernel<K>, one wave per page, the layout of forced_page_common.h and the control structure of
// ta_forced_page_conf.hip: lane l holds the K consecutive WINDOW states l K .. l K + K - 1 (page state minus 2 lo_k) of the
// line it is in as (double, int) registers.  ONE wave runs both fills, with no barrier inside a fill (wave_lds_sync):
//   head      page_head<true>: the page's ONE workspace piece (768 K n bytes, a forward row per character: 64 K doubles,
//             then 64 K exponents), a page of more than 2^24 frames refused, then labels_ok and the queries
//             (TA_FORCED_QUERY as ta_forced_page_conf.hip's).
//   forward   PostCells::forward, the first frame of a line behind the first without a stay term for a label state.  Over
//             a boundary the values go through vbuf masked to the old window's live states and come back shifted by
//             2 (lo_{k+1} - lo_k).  At a character's query frame the lane stores its row in the query line's window
//             coordinates.  Z = a[2 n] + a[2 n - 1]; Z = 0: TA_FORCED_NOPATH, and the outputs are left alone.
//   backward  from the last line to the first, a line's chunks from last to first.  Inside a line PostCells::backward.  The
//             step over a line boundary is split: the emission of frame (k + 1, 0) is multiplied in in window k + 1's
//             coordinates and labels, the values go through vbuf masked to window k + 1's live states and come back shifted
//             into window k's coordinates, labels and skip bits (of the page's text) are loaded again, and a label state
//             has no stay term.
//   zeros     a state that is not live must be the pair zero wherever a sum reads it.  The forward fill reads lower states
//             only: what it leaves above a window's last state is never read by a live state, is masked at the next
//             boundary and is no candidate of a combine.  The backward fill reads HIGHER states: they are zero at the
//             page's end and set to zero at every boundary, and zero times an emission plus zero stays zero.
//   exponents a and b at one frame cover disjoint frames, so with at most 2^24 frames every real exponent, g's included,
//             lies above -17 2^24 - 2 and below 1.6 2^24: clear of zero's -2^29, and two of them add inside an int.
//   combine   at a query frame the character's forward row comes back to the lane that stored it, g = a b, every lane keeps
//             the best of its live states but the character's own, 64 -> 8 -> 1 (two_fill_best).  n times per page.
// Renormalised once per chunk (a line's chunks restart with the line, and a boundary step is the one frame 0 stands
// for): ta_forced_post.hip's bound on a significand's drift inside a chunk holds unchanged.
// Every bound is re-checked on the page's own device numbers before anything is read through it; a refused page gets a
// status and touches nothing else.
#include "forced_page_common.h"
#include "forced_post_cells.h"

namespace {

constexpr int64_t kMaxPostFrames = 1ll << 24;

struct PagePostArgs : PageArgs {
    const int32_t* query;      // [nlabels][TA_FORCED_PAGE_FIELDS]: field 0 the line, field 3 the frame
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state; double* z_m; int32_t* z_x;
};

// a page's ONE piece of the workspace: per character 64 K doubles and 64 K int32, 768 K n bytes, in rows of 256 bytes
__host__ __device__ inline int64_t page_post_rows(int n, int K) { return 3 * (int64_t)K * n; }
__host__ __device__ inline int64_t page_post_bytes(int64_t n, int K) { return 256 * page_post_rows((int)n, K); }

template <int K>
__global__ __launch_bounds__(64) void forced_page_post_kernel(PagePostArgs a) {
    __shared__ float etab[2 * kChunk * kMaxNo];        // two chunks of emissions (8 KiB)
    __shared__ double vbm[64 * K];                     // the values on their way from one window to the next
    __shared__ int vbx[64 * K];
    __shared__ PostRed red;
    __shared__ long long share[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    auto too_many_frames = [&](long long mine) {       // the lanes' shares through LDS, every lane reads all 64
        share[lane] = mine;
        __syncthreads();
        long long all = 0;
        for (int l = 0; l < 64; ++l) all += share[l];
        __syncthreads();
        return all > kMaxPostFrames;
    };
    PageHead h;
    if (!page_head<true>(a, b, lane, kMaxText, page_post_rows, too_many_frames, h)) return;
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
    unsigned char* rows = a.ws + a.ws_off[b];          // row i: 64 K doubles, then 64 K exponents; register r at r * 64 + lane
    auto row_m = [&](int i) { return reinterpret_cast<double*>(rows + (int64_t)i * (768 * K)); };
    auto row_x = [&](int i) { return reinterpret_cast<int*>(rows + (int64_t)i * (768 * K) + 512 * K); };
    const Val zero = PostCells::zero();

    Val v[K];
    int lab[K / 2];
    Feed<float> feed(etab, no, lane);
    // the query cursor, wave-uniform: the next character whose query is still ahead, its line and its frame
    int cur = 0, wk = -1, wt = -1;
    auto fetch = [&]() {
        const bool in = cur >= 0 && cur < n;
        wk = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur]) : -1;
        wt = in ? __builtin_amdgcn_readfirstlane(qs[TA_FORCED_PAGE_FIELDS * (int64_t)cur + 3]) : -1;
    };
    int g = 0;                                         // chunks so far: the LDS buffer in turn

    // ---- forward fill; the row of every query frame is kept --------------------------------------------------------------
    {
#pragma unroll
        for (int r = 0; r < K; ++r) v[r] = zero;
        fetch();
        int T = __builtin_amdgcn_readfirstlane(a.T[l0]);
        const float* P = a.probs + a.row_off[l0] * no;
        feed.prefetch(P, T, 0);
        int lo_old = 0, hi_old = 0;
        for (int k = 0; k < nl; ++k) {
            const int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + k]), hi = __builtin_amdgcn_readfirstlane(a.hi[l0 + k]);
            Val edge = zero;
            const int d = 2 * (lo - lo_old);           // old window states in front of the new window
            if (k > 0) {                               // from the old window's lanes and registers to the new one's
                const int wold = 2 * (hi_old - lo_old);
                wave_lds_sync();
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r;
                    vbm[j] = j <= wold ? v[r].m : 0.0;
                    vbx[j] = j <= wold ? v[r].x : kZeroX;
                }
                wave_lds_sync();
                // d - 1 < wold: lo <= hi_old.  Normalised as chunk_begin is about to do for v: a sum's two significands
                // must not lie further apart than a chunk lets them drift
                if (d >= 1) edge = normal(Val{vbm[d - 1], vbx[d - 1]});
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int j = lane * K + r + d;
                    v[r] = j < 64 * K ? Val{vbm[j], vbx[j]} : zero;
                }
            }
            const unsigned skip = lane_labels(h.cs, lo, hi, lane, lab);
            const bool more = k + 1 < nl;
            const int Tn = more ? __builtin_amdgcn_readfirstlane(a.T[l0 + k + 1]) : 0;
            const float* Pn = more ? a.probs + a.row_off[l0 + k + 1] * no : P;
            const int nchunks = (T + kChunk - 1) / kChunk;
            for (int c = 0; c < nchunks; ++c, ++g) {
                const float* ebuf = feed.publish(g, emission_f);
                if (c + 1 < nchunks) feed.prefetch(P, T, c + 1);
                else feed.prefetch(Pn, Tn, 0);
                wave_lds_sync();
                PostCells::chunk_begin(v);
                const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
                for (int t = t0; t < t1; ++t) {
                    const float* e = ebuf + (t - t0) * no;
                    if (t == 0) {
                        if (k == 0) {
                            if (lane == 0) { v[0] = PostCells::first(e[0]); v[1] = PostCells::first(e[lab[0]]); }
                        } else {
                            const Val left = left_of(v[K - 1]);
                            PostCells::forward<K, true>(v, lane == 0 ? edge : left, skip, lab, e);
                        }
                    } else {
                        PostCells::forward<K>(v, left_of(v[K - 1]), skip, lab, e);
                    }
                    while (wk == k && wt == t) {
                        double* rm = row_m(cur);
                        int* rx = row_x(cur);
#pragma unroll
                        for (int r = 0; r < K; ++r) {
                            rm[r * 64 + lane] = v[r].m;
                            rx[r * 64 + lane] = v[r].x;
                        }
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
        // Z: the last window ends at the page's last state (hi = n); an empty last window does not hold 2 n - 1
        if (lane == 0) { red.m[0] = red.m[1] = 0.0; red.x[0] = red.x[1] = kZeroX; }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int s = 2 * lo_old + lane * K + r;
            if (s == 2 * n) { red.m[0] = v[r].m; red.x[0] = v[r].x; }
            if (s == 2 * n - 1) { red.m[1] = v[r].m; red.x[1] = v[r].x; }
        }
        __syncthreads();                               // (a row is read back by the very lane that stored it)
        const Val z = normal(add(Val{red.m[0], red.x[0]}, Val{red.m[1], red.x[1]}));
        __syncthreads();
        if (z.m == 0.0) {                              // wave-uniform
            if (lane == 0) a.status[b] = TA_FORCED_NOPATH;
            return;
        }
        if (lane == 0) {
            a.z_m[b] = z.m;
            a.z_x[b] = z.x;
        }
    }

    // ---- backward fill, and the combine at every query frame ------------------------------------------------------------
    cur = n - 1;
    fetch();
    int lo = __builtin_amdgcn_readfirstlane(a.lo[l0 + nl - 1]), hi = n;
    auto combine_at = [&](int k, int t) {              // the characters queried at frame (k, t), the one v holds b of
        while (wk == k && wt == t) {
            const double* rm = row_m(cur);
            const int* rx = row_x(cur);
            const int own = 2 * (cur - lo) + 1, wlast = 2 * (hi - lo);
            PostCand best{kKeyNone, 0.0, 0};
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                // what this very lane stored in the forward fill
                const Val gs = normal(Val{rm[r * 64 + lane] * v[r].m, rx[r * 64 + lane] + v[r].x});
                const int gx = gs.m == 0.0 ? kKeyZero : gs.x;
                if (j == own) { red.m[72] = gs.m; red.x[72] = gx; }
                else if (j <= wlast && PostCells::better(PostCand{gx, gs.m, j}, best)) best = PostCand{gx, gs.m, j};
            }
            best = two_fill_best<PostCells>(&red, lane, best);
            if (lane == 0) {
                const int64_t at = h.c0 + cur;
                a.own_m[at] = red.m[72];
                a.own_x[at] = red.x[72] == kKeyZero ? 0 : red.x[72];
                a.rival_m[at] = best.m;
                a.rival_x[at] = best.x == kKeyZero ? 0 : best.x;
                a.rival_state[at] = 2 * lo + best.s;
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
        v[r] = s == 2 * n || s == 2 * n - 1 ? PostCells::one() : zero;
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
        const float* e0 = etab;                        // frame 0's emissions: the first row of chunk 0's buffer
        for (int c = nchunks - 1; c >= 0; --c, ++g) {
            const float* ebuf = feed.publish(g, emission_f);
            if (c >= 1) feed.prefetch(P, T, c - 1);
            else feed.prefetch(Pp, Tp, (Tp + kChunk - 1) / kChunk - 1);        // (k = 0: no such chunk, zeros)
            wave_lds_sync();
            PostCells::chunk_begin(v);
            e0 = ebuf;
            const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
            for (int t = t1 - 1; t >= t0 && t >= 1; --t) {             // the emission of frame t takes the fill from t to t - 1
                PostCells::backward<K>(v, skipf, lab, ebuf + (t - t0) * no);
                combine_at(k, t - 1);
            }
        }
        if (k == 0) break;                             // the page's first frame: its emission is never applied
        // ---- over the line boundary: frame (k, 0)'s emission in window k, then into window k - 1 --------------------------
        {
            const double eb = (double)e0[0];
            const int wlast = 2 * (hi - lo);
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r;
                vbm[j] = j <= wlast ? v[r].m * ((r & 1) ? (double)e0[lab[r >> 1]] : eb) : 0.0;
                vbx[j] = j <= wlast ? v[r].x : kZeroX;
            }
            wave_lds_sync();
        }
        const int lo_new = __builtin_amdgcn_readfirstlane(a.lo[l0 + k - 1]), hi_new = __builtin_amdgcn_readfirstlane(a.hi[l0 + k - 1]);
        {
            const int d = 2 * (lo - lo_new), wlast = 2 * (hi_new - lo_new);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int j = lane * K + r - d;        // the state in window k's coordinates
                v[r] = j >= 0 ? Val{vbm[j], vbx[j]} : zero;
            }
            unsigned skipb;
            lane_labels(h.cs, lo_new, n, lane, lab, &skipb);
            const Val r0 = right_of(v[0]), r1 = right_of(v[1]);
#pragma unroll
            for (int r = 0; r < K; ++r) {              // upwards; a label state has no stay term
                Val y = add((r & 1) ? zero : v[r], r + 1 < K ? v[(r + 1) % K] : r0);
                if (r & 1) {
                    const Val sk = r + 2 < K ? v[(r + 2) % K] : r1;
                    y = add(y, ((skipb >> (r >> 1)) & 1u) ? sk : zero);
                }
                v[r] = lane * K + r <= wlast ? y : zero;               // nothing above the new window's last state
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

extern "C" int64_t ta_forced_page_posterior_workspace_bytes(int64_t n, int32_t K) {
    if (n < 1 || n > kMaxText || !(K == 2 || K == 4 || K == 8 || K == 16 || K == 32)) return -1;
    return page_post_bytes(n, K);
}

extern "C" int ta_forced_page_posterior(const float* probs, const int64_t* row_off, const int32_t* T,
                                        const int64_t* line_first, const int32_t* lo, const int32_t* hi,
                                        const int32_t* labels, const int64_t* lab_off, const int64_t* ws_off,
                                        const int32_t* query, int32_t npages, int32_t nlines, int32_t no, int64_t rows,
                                        int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                                        const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host,
                                        void* workspace, int64_t workspace_bytes, double* own_m, int32_t* own_x,
                                        double* rival_m, int32_t* rival_x, int32_t* rival_state, double* z_m, int32_t* z_x,
                                        int32_t* status, void* stream) {
    bool go;
    const int rc = forced_preamble(npages < 0 || nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr,
                                   npages == 0,
                                   !probs || !row_off || !T || !line_first || !lo || !hi || !labels || !lab_off || !ws_off ||
                                       !query || !T_host || !line_first_host || !lo_host || !hi_host || !lab_off_host ||
                                       !workspace || !own_m || !own_x || !rival_m || !rival_x || !rival_state || !z_m ||
                                       !z_x || !status,
                                   workspace, &go);
    if (!go) return rc;
    int variants;
    // forced_check_pages' refusals; its workspace rule (a piece per line) asks nothing here, the page's rule follows
    const int rc2 = forced_check_pages(T_host, line_first_host, lo_host, hi_host, lab_off_host, npages, nlines, rows, nlabels,
                                       workspace_bytes, [](int, int) { return (int64_t)0; }, kMaxText, "a page's text is too long",
                                       kMaxPostFrames, "a page has more than 2^24 frames",
                                       "ta_forced_page_posterior_workspace_bytes", &variants);
    if (rc2 != TA_OK) return rc2;
    int64_t need = 0;
    for (int p = 0; p < npages && need <= workspace_bytes; ++p) {          // (a piece is at most 2^44 bytes)
        int kp = 2;
        for (int64_t q = line_first_host[p]; q < line_first_host[p + 1]; ++q) {
            const int kw = window_k(hi_host[q] - lo_host[q]);
            kp = kw > kp ? kw : kp;
        }
        need += page_post_bytes(lab_off_host[p + 1] - lab_off_host[p], kp);
    }
    if (workspace_bytes < need) return forced_ws_small("pages", "ta_forced_page_posterior_workspace_bytes");
    const PagePostArgs a{{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                          nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, nullptr, nullptr, status, 0},
                         query, own_m, own_x, rival_m, rival_x, rival_state, z_m, z_x};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_post_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_post_kernel launch");
    return TA_OK;
}
