// ta_forced_page_post.hip -- sum-product posteriors at page scope and the page's likelihood: for
// a query frame (line, t) per character i of a page's text, the mass of ALL legal paths through ALL the lines of the page
// that spend that frame in the character's own state 2 i + 1, the largest such mass over the other live states with the
// state that has it, and per page the mass Z of all paths.  The lattice is ta_forced_page.hip's (windows that move from
// line to line, no character across a line break), the arithmetic ta_forced_post.hip's (forced_post_cells.h: pairs
// (double, int), every + and * rounded once); the checker of record is tests/forced_page_post_ref.py, and every word
// written here equals it bit for bit.  Built with -ffp-contract=off.
//
// forced_page_post_kernel<K>, one wave per page: lane l holds the K consecutive WINDOW states l K .. l K + K - 1 (page
// state minus 2 lo_k) of the line it is in as (double, int) registers.  The head, the control structure of the two fills
// and the query cursor are page_two_fill's (forced_page_two_fill.h, shared with ta_forced_page_conf.hip); the arithmetic
// is PagePostCells below, PostCells with what a page adds:
//   head      the page's ONE workspace piece is 768 K n bytes, a forward row per character: 64 K doubles, then 64 K
//             exponents; a page of more than 2^24 frames is refused.
//   forward   PostCells::forward, the first frame of a line behind the first without a stay term for a label state.
//             Z = a[2 n] + a[2 n - 1]; Z = 0: TA_FORCED_NOPATH, and the outputs are left alone.
//   backward  inside a line PostCells::backward, spelled out below (profiles/forced_page_two_fill.txt, 3); over a line
//             boundary the emission is multiplied in and a label state has no stay term.
//   zeros     a state that is not live must be the pair zero wherever a sum reads it.  The forward fill reads lower states
//             only: what it leaves above a window's last state is never read by a live state, is masked at the next
//             boundary and is no candidate of a combine.  The backward fill reads HIGHER states: they are zero at the
//             page's end and set to zero at every boundary, and zero times an emission plus zero stays zero.
//   exponents a and b at one frame cover disjoint frames, so with at most 2^24 frames every real exponent, g's included,
//             lies above -17 2^24 - 2 and below 1.6 2^24: clear of zero's -2^29, and two of them add inside an int.
//   combine   g = a b, every lane keeps the best of its live states but the character's own, then two_fill_best.
// Renormalised once per chunk (a line's chunks restart with the line, and a boundary step is the one frame 0 stands
// for): ta_forced_post.hip's bound on a significand's drift inside a chunk holds unchanged.  The state in front of a new
// window (edge) is normalised as chunk_begin is about to do for v: a sum's two significands must not lie further apart
// than a chunk lets them drift.
#include "forced_page_two_fill.h"
#include "forced_post_cells.h"

namespace {

constexpr int64_t kMaxPostFrames = 1ll << 24;

struct PagePostArgs : PageTwoFillArgs {
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state; double* z_m; int32_t* z_x;
};

// a page's ONE piece of the workspace: per character 64 K doubles and 64 K int32, 768 K n bytes, in rows of 256 bytes
__host__ __device__ inline int64_t page_post_rows(int n, int K) { return 3 * (int64_t)K * n; }
__host__ __device__ inline int64_t page_post_bytes(int64_t n, int K) { return 256 * page_post_rows((int)n, K); }

struct PagePostBuf { double* m; int* x; };             // [64 K] each

// page_two_fill's arithmetic: PostCells' (forced_post_cells.h: zero, one, emit, first, left, chunk_begin, forward and the
// candidates of two_fill_best), and a page's own; row i is 64 K doubles, then 64 K exponents, register r at
// r * 64 + lane
struct PagePostCells : PostCells {
    using Args = PagePostArgs;
    using Buf = PagePostBuf;
    __host__ __device__ static inline int64_t rows_of(int n, int K) { return page_post_rows(n, K); }
    __device__ static __forceinline__ V left_edge(V v, V edge, int lane) {
        const Val left = left_of(v);
        return lane == 0 ? edge : left;
    }
    __device__ static __forceinline__ V apply(V v, E e) { return Val{v.m * (double)e, v.x}; }
    __device__ static __forceinline__ void put_v(Buf buf, int j, bool live, V v) {
        buf.m[j] = live ? v.m : 0.0;
        buf.x[j] = live ? v.x : kZeroX;
    }
    __device__ static __forceinline__ V get_v(Buf buf, int j) { return Val{buf.m[j], buf.x[j]}; }
    __device__ static __forceinline__ V edge(Buf buf, int j) { return normal(get_v(buf, j)); }
    __device__ static __forceinline__ void end_put(Red* red, int i, V v) { red->m[i] = v.m; red->x[i] = v.x; }
    __device__ static __forceinline__ V end_get(const Red* red, int i) { return Val{red->m[i], red->x[i]}; }
    template <int K> __device__ static __forceinline__ double* row_m(unsigned char* rows, int i) {
        return reinterpret_cast<double*>(rows + (int64_t)i * (768 * K));
    }
    template <int K> __device__ static __forceinline__ int* row_x(unsigned char* rows, int i) {
        return reinterpret_cast<int*>(rows + (int64_t)i * (768 * K) + 512 * K);
    }

    // PostCells::backward, spelled out with a frame's emissions read from LDS together, ahead of the products: through the
    // shared cell K = 32 waits for each read behind 4 instructions and measured 2 % slower than before the cell was shared
    template <int K>
    __device__ static __forceinline__ void backward(V (&v)[K], unsigned skipf, const int (&lab)[K / 2], const E* e) {
        const Val zero{0.0, kZeroX};
        const double eb = (double)e[0];
        float el[K / 2];
#pragma unroll
        for (int j = 0; j < K / 2; ++j) el[j] = e[lab[j]];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k].m *= (k & 1) ? (double)el[k >> 1] : eb;
        const Val r0 = right_of(v[0]), r1 = right_of(v[1]);
#pragma unroll
        for (int k = 0; k < K; ++k) {                  // upwards: v[k + 1] and v[k + 2] still carry frame t
            Val y = add(v[k], k + 1 < K ? v[(k + 1) % K] : r0);
            if (k & 1) {
                const Val sk = k + 2 < K ? v[(k + 2) % K] : r1;
                y = add(y, ((skipf >> (k >> 1)) & 1u) ? sk : zero);
            }
            v[k] = y;
        }
    }

    template <int K>
    __device__ static __forceinline__ void boundary(V (&v)[K], unsigned skipb, int wlast, int lane) {
        const Val zero = PostCells::zero();
        const Val r0 = right_of(v[0]), r1 = right_of(v[1]);
#pragma unroll
        for (int r = 0; r < K; ++r) {                  // upwards; a label state has no stay term
            Val y = add((r & 1) ? zero : v[r], r + 1 < K ? v[(r + 1) % K] : r0);
            if (r & 1) {
                const Val sk = r + 2 < K ? v[(r + 2) % K] : r1;
                y = add(y, ((skipb >> (r >> 1)) & 1u) ? sk : zero);
            }
            v[r] = lane * K + r <= wlast ? y : zero;                   // nothing above the new window's last state
        }
    }

    template <int K>
    __device__ static __forceinline__ void store_row(unsigned char* rows, int cur, int lane, const V (&v)[K]) {
        double* rm = row_m<K>(rows, cur);
        int* rx = row_x<K>(rows, cur);
#pragma unroll
        for (int r = 0; r < K; ++r) {
            rm[r * 64 + lane] = v[r].m;
            rx[r * 64 + lane] = v[r].x;
        }
    }

    // Z = a[2 n] + a[2 n - 1]; zero: no path
    __device__ static __forceinline__ bool forward_done(const Args& a, int b, int lane, V e0, V e1) {
        const Val z = normal(add(e0, e1));
        if (z.m == 0.0) return false;
        if (lane == 0) {
            a.z_m[b] = z.m;
            a.z_x[b] = z.x;
        }
        return true;
    }

    // character `cur` at the frame v holds b of, in the window lo .. hi
    template <int K>
    __device__ static __forceinline__ void combine(const Args& a, const PageHead& h, unsigned char* rows, int cur, int lo, int hi,
                                                   int lane, const V (&v)[K], Red* redp) {
        Red& red = *redp;
        const double* rm = row_m<K>(rows, cur);
        const int* rx = row_x<K>(rows, cur);
        const int own = 2 * (cur - lo) + 1, wlast = 2 * (hi - lo);
        PostCand best{kKeyNone, 0.0, 0};
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int j = lane * K + r;
            // what this very lane stored in the forward fill
            const Val gs = normal(Val{rm[r * 64 + lane] * v[r].m, rx[r * 64 + lane] + v[r].x});
            const int gx = gs.m == 0.0 ? kKeyZero : gs.x;
            if (j == own) { red.m[72] = gs.m; red.x[72] = gx; }
            else if (j <= wlast && better(PostCand{gx, gs.m, j}, best)) best = PostCand{gx, gs.m, j};
        }
        best = two_fill_best<PostCells>(redp, lane, best);
        if (lane == 0) {
            const int64_t at = h.c0 + cur;
            a.own_m[at] = red.m[72];
            a.own_x[at] = red.x[72] == kKeyZero ? 0 : red.x[72];
            a.rival_m[at] = best.m;
            a.rival_x[at] = best.x == kKeyZero ? 0 : best.x;
            a.rival_state[at] = 2 * lo + best.s;
        }
    }
};

template <int K>
__global__ __launch_bounds__(64) void forced_page_post_kernel(PagePostArgs a) {
    __shared__ float etab[2 * kChunk * kMaxNo];        // two chunks of emissions (8 KiB)
    __shared__ double vbm[64 * K];                     // the values on their way from one window to the next
    __shared__ int vbx[64 * K];
    __shared__ PostRed red;
    __shared__ long long share[64];
    const int lane = threadIdx.x;
    page_two_fill<K, PagePostCells>(a, etab, PagePostBuf{vbm, vbx}, &red, [&](long long mine) {       // the lanes' shares of the
        share[lane] = mine;                            // page's frames through LDS, every lane reads all 64
        __syncthreads();
        long long all = 0;
        for (int l = 0; l < 64; ++l) all += share[l];
        __syncthreads();
        return all > kMaxPostFrames;
    });
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
    const PagePostArgs a{{{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, 0, rows, nlabels,
                           static_cast<unsigned char*>(workspace), workspace_bytes, nullptr, nullptr, status, 0}, query},
                         own_m, own_x, rival_m, rival_x, rival_state, z_m, z_x};
    return page_two_fill_call(a, !own_m || !own_x || !rival_m || !rival_x || !rival_state || !z_m || !z_x, T_host,
                              line_first_host, lo_host, hi_host, lab_off_host, kMaxPostFrames, "a page has more than 2^24 frames",
                              "ta_forced_page_posterior_workspace_bytes", "forced_page_post_kernel launch", page_post_bytes,
                              [&](auto kc, const PagePostArgs& args) {
        hipLaunchKernelGGL((forced_page_post_kernel<decltype(kc)::value>), dim3((unsigned)args.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), args);
    });
}
