// ta_forced_page_conf.hip -- per-character confidence at page scope from max-marginals: for a
// query frame (line, t) per character i of a page's text, the total of the best legal path through ALL the lines of the
// page that spends that frame in the character's own state 2 i + 1, minus the total of the best one that spends it in any
// other live state, and that state.  Integers only, on the lattice of ta_forced_page.hip (windows that move from line to
// line, no character across a line break); the checker of record is tests/forced_page_conf_ref.py.
//
// forced_page_conf_kernel<K>, one wave per page: lane l holds the K consecutive WINDOW states l K .. l K + K - 1 (page
// state minus 2 lo_k) of the line it is in as int64 registers.  The head, the control structure of the two fills and the
// query cursor are page_two_fill's (forced_page_two_fill.h, shared with ta_forced_page_post.hip); the arithmetic is
// PageConfCells below:
//   head      the page's ONE workspace piece is 512 K n bytes, a forward row per character; a page of more than 2^25
//             frames is refused (G 2048 and the reachability test stay exact).
//   forward   A: the cell is forced_step without its moves.  At a character's query frame the lane stores its row, K
//             coalesced 8-byte stores.  A best end below -2^49: TA_FORCED_NOPATH, and the outputs are left alone.
//   backward  B: inside a line the step is ta_forced_conf.hip's (the RIGHT lane's first two values, wave_shl:1); over a
//             line boundary the emission is added and the max has no stay candidate for a label state.
//   masks     the forward fill leaves junk above a window's last state (a state reads lower states only, so no live state
//             ever reads it).  The backward fill reads HIGHER states: at every boundary the states above the new window's
//             last state are set to -2^50, and from there they only go down (every emission is <= 0).
//   combine   G = A + B where both are above -2^49 (else exactly -2^50), states beyond the window's last state left out,
//             G 2048 + (2047 - window state) through two_fill_best: the largest value at the smallest state.
#include "forced_page_two_fill.h"

namespace {

constexpr long long kReach = -(1ll << 49);

struct PageConfArgs : PageTwoFillArgs {
    int64_t* confidence;
    int32_t* rival;
};

// a page's ONE piece of the workspace: a forward row of 64 K int64 per character, 512 K n bytes, in rows of 256 bytes
__host__ __device__ inline int64_t page_conf_rows(int n, int K) { return 2 * (int64_t)K * n; }
__host__ __device__ inline int64_t page_conf_bytes(int64_t n, int K) { return 256 * page_conf_rows((int)n, K); }

// page_two_fill's arithmetic: max-plus on int64 scores; row i is 64 K values, register r at r * 64 + lane
struct PageConfCells {
    using V = long long;
    using E = int;
    using Args = PageConfArgs;
    using Buf = long long*;    // [64 K]
    using Red = long long;     // [73]: 64 lanes' candidates, 8 partial maxima, the own state's value
    using Cand = long long;    // value and state packed: the largest key is the largest value at the smallest state
    __device__ static __forceinline__ void put(Red* red, int i, Cand c) { red[i] = c; }
    __device__ static __forceinline__ Cand get(const Red* red, int i) { return red[i]; }
    __device__ static __forceinline__ bool better(Cand a, Cand b) { return a > b; }
    __host__ __device__ static inline int64_t rows_of(int n, int K) { return page_conf_rows(n, K); }
    __device__ static __forceinline__ V zero() { return kNeg; }
    __device__ static __forceinline__ V one() { return 0; }
    __device__ static __forceinline__ E emit(float p) { return emission_q(p); }
    __device__ static __forceinline__ V first(E q) { return q; }
    __device__ static __forceinline__ V left(V v) { return from_left(v, kNeg); }
    __device__ static __forceinline__ V left_edge(V v, V edge, int) { return from_left(v, edge); }
    __device__ static __forceinline__ V apply(V v, E q) { return v + q; }
    __device__ static __forceinline__ void put_v(Buf buf, int j, bool live, V v) { buf[j] = live ? v : kNeg; }
    __device__ static __forceinline__ V get_v(Buf buf, int j) { return buf[j]; }
    __device__ static __forceinline__ V edge(Buf buf, int j) { return buf[j]; }
    __device__ static __forceinline__ void end_put(Red* red, int i, V v) { red[i] = v; }
    __device__ static __forceinline__ V end_get(const Red* red, int i) { return red[i]; }
    template <int K> __device__ static __forceinline__ void chunk_begin(V (&)[K]) {}

    template <int K, bool kFirst>
    __device__ static __forceinline__ void forward(V (&v)[K], V left, unsigned skip, const int (&lab)[K / 2], const E* q) {
        forced_step<K, kFirst>(v, left, skip, lab, q, q[0]);
    }

    // a frame inside a line, downwards in time: ta_forced_conf.hip's ConfCells::backward
    template <int K>
    __device__ static __forceinline__ void backward(V (&v)[K], unsigned skipf, const int (&lab)[K / 2], const E* q) {
        const int qb = q[0];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += (k & 1) ? q[lab[k >> 1]] : qb;
        const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
        for (int k = 0; k < K; ++k) {                  // upwards: v[k + 1] and v[k + 2] still carry frame t
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

    template <int K>
    __device__ static __forceinline__ void boundary(V (&v)[K], unsigned skipb, int wlast, int lane) {
        const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
        for (int r = 0; r < K; ++r) {                  // upwards; a label state has no stay candidate
            long long best = (r & 1) ? kNeg : v[r];
            const long long adv = r + 1 < K ? v[(r + 1) % K] : r0;
            if (adv > best) best = adv;
            if (r & 1) {
                const long long sk = r + 2 < K ? v[(r + 2) % K] : r1;
                if (((skipb >> (r >> 1)) & 1u) && sk > best) best = sk;
            }
            v[r] = lane * K + r <= wlast ? best : kNeg;                 // nothing above the new window's last state
        }
    }

    template <int K>
    __device__ static __forceinline__ void store_row(unsigned char* rows, int cur, int lane, const V (&v)[K]) {
        long long* row = reinterpret_cast<long long*>(rows) + (int64_t)cur * (64 * K);
#pragma unroll
        for (int r = 0; r < K; ++r) row[r * 64 + lane] = v[r];
    }

    // the best end below -2^49: no path
    __device__ static __forceinline__ bool forward_done(const Args&, int, int, V e0, V e1) { return (e1 > e0 ? e1 : e0) >= kDead; }

    // character `cur` at the frame v holds B of, in the window lo .. hi
    template <int K>
    __device__ static __forceinline__ void combine(const Args& a, const PageHead& h, const unsigned char* rows, int cur, int lo,
                                                   int hi, int lane, const V (&v)[K], Red* red) {
        const long long* row = reinterpret_cast<const long long*>(rows) + (int64_t)cur * (64 * K);
        const int own = 2 * (cur - lo) + 1, wlast = 2 * (hi - lo);
        long long key = kNeg * 2048;                   // below every candidate's
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int j = lane * K + r;
            const long long fa = row[r * 64 + lane];                   // what this very lane stored in the forward fill
            const long long gs = fa > kReach && v[r] > kReach ? fa + v[r] : kNeg;
            const long long cand = gs * 2048 + (2047 - j);              // the larger value first, then the smaller state
            if (j == own) red[72] = gs;
            else if (j <= wlast && cand > key) key = cand;
        }
        const long long m = two_fill_best<PageConfCells>(red, lane, key);
        if (lane == 0) {
            a.confidence[h.c0 + cur] = red[72] - (m >> 11);
            a.rival[h.c0 + cur] = 2 * lo + 2047 - (int)(m & 2047);
        }
    }
};

template <int K>
__global__ __launch_bounds__(64) void forced_page_conf_kernel(PageConfArgs a) {
    __shared__ int qtab[2 * kChunk * kMaxNo];          // two chunks of emission scores (8 KiB)
    __shared__ long long vbuf[64 * K];                 // the values on their way from one window to the next
    __shared__ long long red[73];
    const int lane = threadIdx.x;
    page_two_fill<K, PageConfCells>(a, qtab, vbuf, red, [&](long long mine) {      // the lanes' shares of the page's frames
        red[lane] = mine;                              // through LDS, every lane reads all 64
        __syncthreads();
        long long all = 0;
        for (int l = 0; l < 64; ++l) all += red[l];
        __syncthreads();
        return all > kMaxFrames;
    });
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
    const PageConfArgs a{{{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, 0, rows, nlabels,
                           static_cast<unsigned char*>(workspace), workspace_bytes, nullptr, nullptr, status, 0}, query},
                         confidence, rival};
    return page_two_fill_call(a, !confidence || !rival, T_host, line_first_host, lo_host, hi_host, lab_off_host, kMaxFrames,
                              "a page has more than 2^25 frames", "ta_forced_page_confidence_workspace_bytes",
                              "forced_page_conf_kernel launch", page_conf_bytes, [&](auto kc, const PageConfArgs& args) {
        hipLaunchKernelGGL((forced_page_conf_kernel<decltype(kc)::value>), dim3((unsigned)args.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), args);
    });
}
