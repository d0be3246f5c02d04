// ta_errs.hip -- held-out scoring of line models on the GPU: unit-cost edit distance between a line's decoded class
// codes and its ground truth, the op counts of ONE alignment (fixed tie order) and the confusion matrix -- what
// `ocropus-errs` / `ocropus-econf` report (parity unpinned, the checker of record is
// tests/errs_ref.py).
//
// One wave per line, three stages:
//   filter   the decoded codes as ta_decode / ta_decode_summary left them (the length is read HERE, the host never
//            knew it): class 0 dropped, class 1 (" ") by the text kind, compacted into LDS by ballot / prefix count
//   fill     strips of 64 target columns, a lane per column along anti-diagonals: the left neighbour's value comes by
//            DPP (wave_shr:1), lane 0's from the previous strip's right edge column in LDS (updated in place: lane 63
//            writes row i 63 steps after lane 0 read it).  Two pointer bits per cell -- 0 match, 1 substitution,
//            2 insertion, 3 deletion, chosen in that order among the minima -- go to the workspace as two ballots per
//            step; every lane keeps the pair of one step in 64, so a strip's pointers leave as 1 KB stores.
//   walk     from (n, m) back to (0, 0), wave-uniform, through a 64-step window of the pointers in LDS; lane 0 counts
//            the matches per class in LDS and adds everything else into conf with integer atomics (order-free).
// Every bound is re-checked on the line's own device numbers before anything is read through it; a refused line gets
// errors = -1 and touches nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kMaxN = TA_ERRS_MAX_DECODED;
constexpr int kMaxM = TA_ERRS_MAX_TARGET;
constexpr int kMaxNc = TA_TRAIN_MAX_CLASSES + 1;       // class codes 0 .. No, No = "not in the codec"
static_assert(kMaxNc <= 255, "codes are staged as bytes");
static_assert(kMaxN + kMaxM < 65536, "a distance fits the 16-bit edge column");

struct ErrArgs {
    const int32_t* dec_c; const int64_t* dec_off; const int32_t* dec_n; int64_t dec_len;
    const int32_t* tgt; const int64_t* tgt_off; const int32_t* tgt_n; int64_t tgt_len;
    const int32_t* n_bound; const int64_t* ws_off;
    int32_t nlines, nclasses, kind;
    unsigned char* ws; int64_t ws_bytes;
    int32_t* per_line; unsigned long long* conf;
};

__host__ __device__ inline int64_t errs_ws_bytes(int n, int m) { return 16 * (int64_t)(n + 63) * ((m + 63) >> 6); }

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void refuse(int32_t* out, int lane) {
    if (lane < TA_ERRS_FIELDS) out[lane] = lane == 0 ? -1 : 0;
}

__global__ __launch_bounds__(64) void edit_distance_kernel(ErrArgs a) {
    __shared__ unsigned char sa[kMaxN + 12];          // the filtered decoded codes
    __shared__ unsigned char sg[kMaxM];               // the target codes
    __shared__ unsigned short edge[kMaxN + 3];        // D[i][64 s]: the column left of the strip being filled
    __shared__ ulonglong2 win[64];                    // pointer bits of 64 steps of one strip (walk)
    __shared__ int hist[kMaxNc];                      // matches per class
    __shared__ int dist_s;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nc = a.nclasses;
    int32_t* out = a.per_line + (int64_t)TA_ERRS_FIELDS * b;
    const int dn = uni(a.dec_n[b]), m = uni(a.tgt_n[b]), nb = uni(a.n_bound[b]);
    const int64_t d0 = a.dec_off[b], g0 = a.tgt_off[b], w0 = a.ws_off[b];
    // every bound the kernel relies on, on the line's own numbers (the host checked its copies as well)
    const bool ok = nb >= 0 && nb <= kMaxN && dn >= 0 && dn <= nb && d0 >= 0 && d0 + dn <= a.dec_len &&
                    m >= 0 && m <= kMaxM && g0 >= 0 && g0 + m <= a.tgt_len &&
                    w0 >= 0 && (w0 & 15) == 0 && w0 + errs_ws_bytes(nb, m) <= a.ws_bytes;
    if (!ok) { refuse(out, lane); return; }

    // ---- stage the target, filter the decoded codes ---------------------------------------------------------------
    bool bad = false;
    for (int j = lane; j < m; j += 64) {
        const int c = a.tgt[g0 + j];
        bad |= c < 1 || c >= nc;
        sg[j] = (unsigned char)c;
    }
    for (int c = lane; c < nc; c += 64) hist[c] = 0;
    int n = 0;
    bool prev_glyph = false;                           // the last code kept so far is no space (false at the start)
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < dn; base += 64) {
        const int idx = base + lane;
        const int c = idx < dn ? a.dec_c[d0 + idx] : 0;
        bad |= c < 0 || c >= nc;
        const unsigned long long nz = __ballot(c != 0), sp = __ballot(c == 1);
        bool keep = c != 0;
        if (c == 1) {
            if (a.kind == TA_ERRS_KIND_NOSPACE) keep = false;
            else {                                     // a space stays only behind a character that is none
                const unsigned long long before = nz & below;
                keep = before ? !((sp >> (63 - __builtin_clzll(before))) & 1ull) : prev_glyph;
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) sa[n + __builtin_popcountll(kept & below)] = (unsigned char)c;
        n += __builtin_popcountll(kept);
        if (nz) prev_glyph = !((sp >> (63 - __builtin_clzll(nz))) & 1ull);
    }
    for (int i = lane; i <= dn; i += 64) edge[i] = (unsigned short)i;      // D[i][0]
    if (__any(bad)) { refuse(out, lane); return; }
    __syncthreads();
    if (a.kind == TA_ERRS_KIND_EXACT && n > 0 && sa[n - 1] == 1) --n;      // runs are collapsed: at most one at the end
    n = uni(n);

    // ---- fill -----------------------------------------------------------------------------------------------------
    const int nstrips = (m + 63) >> 6, nsteps = n + 63;
    ulonglong2* wsl = reinterpret_cast<ulonglong2*>(a.ws + w0);
    if (lane == 0) dist_s = n;                                              // m = 0
    for (int s = 0; s < nstrips; ++s) {
        ulonglong2* wst = wsl + (size_t)s * nsteps;
        const int jc = 64 * s + lane + 1;                                   // the lane's column, 1-based
        const int gj = jc <= m ? (int)sg[jc - 1] : 0xFFFF;                  // beyond the target: equals no code
        int cur = jc, diag = jc - 1;                                        // D[0][jc], D[0][jc - 1]
        unsigned long long k0 = 0ull, k1 = 0ull;
        for (int t = 0; t < nsteps; ++t) {
            const int i = t + 1 - lane;                                     // the lane's row at this step
            int left = 0;
            if (lane == 0 && i <= n) left = edge[i];
            left = __builtin_amdgcn_update_dpp(left, cur, 0x138, 0xf, 0xf, false);      // wave_shr:1; lane 0 keeps its own
            int ptr = 0;
            if (i >= 1 && i <= n) {
                const int cost = (int)sa[i - 1] != gj;
                const int d = diag + cost, u = cur + 1, l = left + 1;
                const int best = min(d, min(u, l));
                ptr = d == best ? cost : (u == best ? 2 : 3);
                cur = best;
                diag = left;
                if (lane == 63) edge[i] = (unsigned short)best;
            }
            const unsigned long long b0 = __ballot(ptr & 1), b1 = __ballot(ptr >> 1);
            if ((t & 63) == lane) { k0 = b0; k1 = b1; }
            if ((t & 63) == 63 || t == nsteps - 1) {
                const int idx = (t & ~63) + lane;
                if (idx <= t) wst[idx] = make_ulonglong2(k0, k1);
            }
        }
        if (s == nstrips - 1 && lane == ((m - 1) & 63)) dist_s = cur;       // D[n][m]
        __syncthreads();
    }
    __threadfence();                                    // the pointers are read back below
    __syncthreads();

    // ---- walk -----------------------------------------------------------------------------------------------------
    int i = n, j = uni(m), subs = 0, ins = 0, dels = 0;
    int win_s = -1, win_base = 0;
    while (i > 0 || j > 0) {
        int x = 0, y = 0, ptr;
        if (j == 0) ptr = 2;
        else if (i == 0) ptr = 3;
        else {
            const int s = (j - 1) >> 6, l = (j - 1) & 63, t = i + l - 1;
            if (s != win_s || t < win_base) {
                __syncthreads();
                win_s = s;
                win_base = max(t - 63, 0);
                if (win_base + lane < nsteps) win[lane] = wsl[(size_t)s * nsteps + win_base + lane];
                __syncthreads();
            }
            const ulonglong2 e = win[t - win_base];
            ptr = uni((int)((e.x >> l) & 1ull) | ((int)((e.y >> l) & 1ull) << 1));
        }
        if (ptr != 3) x = sa[i - 1];
        if (ptr != 2) y = sg[j - 1];
        subs += ptr == 1; ins += ptr == 2; dels += ptr == 3;
        i -= ptr != 3;
        j -= ptr != 2;
        if (lane == 0) {
            if (x == y) ++hist[x];
            else atomicAdd(a.conf + (int64_t)x * nc + y, 1ull);
        }
    }
    __syncthreads();
    for (int c = lane; c < nc; c += 64)
        if (hist[c]) atomicAdd(a.conf + (int64_t)c * nc + c, (unsigned long long)hist[c]);
    if (lane == 0) {
        out[0] = dist_s; out[1] = n; out[2] = m; out[3] = subs; out[4] = ins; out[5] = dels;
    }
}

}  // namespace

extern "C" int64_t ta_errs_workspace_bytes(int32_t n_max, int32_t m) {
    if (n_max < 0 || m < 0) return TA_EINVAL;
    if (n_max > kMaxN || m > kMaxM) return TA_ELIMIT;
    return errs_ws_bytes(n_max, m);
}

extern "C" int ta_edit_distance(const int32_t* dec_c, const int64_t* dec_off, const int32_t* dec_n, int64_t dec_len,
                                const int32_t* targets, const int64_t* tgt_off, const int32_t* tgt_n, int64_t tgt_len,
                                const int32_t* n_bound, const int64_t* ws_off, int32_t nlines, int32_t nclasses,
                                int32_t kind, const int32_t* n_bound_host, const int32_t* tgt_n_host, void* workspace,
                                int64_t workspace_bytes, int32_t* per_line, int64_t* conf, void* stream) {
    if (nlines < 0 || dec_len < 0 || tgt_len < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative size");
    if (kind != TA_ERRS_KIND_EXACT && kind != TA_ERRS_KIND_NOSPACE) return ta_fail(TA_EINVAL, "kind must be TA_ERRS_KIND_EXACT or TA_ERRS_KIND_NOSPACE");
    if (nclasses < 2 || nclasses > kMaxNc) return ta_fail(TA_EINVAL, "nclasses outside 2 .. TA_TRAIN_MAX_CLASSES + 1");
    if (nlines == 0) return TA_OK;
    if (!dec_c || !dec_off || !dec_n || !targets || !tgt_off || !tgt_n || !n_bound || !ws_off || !n_bound_host ||
        !tgt_n_host || !workspace || !per_line || !conf)
        return ta_fail(TA_EINVAL, "null pointer argument");
    int64_t need = 0;
    for (int b = 0; b < nlines; ++b) {
        const int64_t w = ta_errs_workspace_bytes(n_bound_host[b], tgt_n_host[b]);
        if (w == TA_EINVAL) return ta_fail(TA_EINVAL, "negative line length");
        if (w == TA_ELIMIT) return ta_fail(TA_ELIMIT, "a line exceeds TA_ERRS_MAX_DECODED or TA_ERRS_MAX_TARGET");
        need += w;
    }
    if (workspace_bytes < need) return ta_fail(TA_EINVAL, "workspace smaller than the lines' ta_errs_workspace_bytes");
    ErrArgs a{dec_c, dec_off, dec_n, dec_len, targets, tgt_off, tgt_n, tgt_len, n_bound, ws_off, nlines, nclasses, kind,
              static_cast<unsigned char*>(workspace), workspace_bytes, per_line,
              reinterpret_cast<unsigned long long*>(conf)};
    hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)nlines), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "edit_distance_kernel launch");
    return TA_OK;
}
