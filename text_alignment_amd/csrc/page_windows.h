// page_windows.h -- page_windows_kernel<kOmit> and its launch, described at the top of ta_page_windows.hip.  It is a header
// because the kernel is instantiated in TWO translation units: ta_page_windows.hip (kOmit = false: ta_page_windows, the
// strict lattice's rule) and ta_page_windows_omit.hip (kOmit = true: ta_page_windows_omit, the rule
// of the lattice with omission, section 14.17).  The two differ in ONE test behind the first sweep: strict, a page with more
// characters than frames is TA_PAGE_SCOPE_FRAMES; with omission every page has a path, characters are not counted against
// frames, and a page beyond what ta_forced_align_pages_omit takes (kWinMaxChars, kWinMaxFrames) is TA_PAGE_SCOPE_TOO_LONG.
#pragma once
#include "forced_common.h"

namespace {

struct WinArgs {
    const int32_t* table; const int32_t* h_status; const int64_t* line_first; const int64_t* t_off; const int32_t* t_class;
    const int32_t* T; const uint8_t* plain;
    int32_t npages, nlines; int64_t t_len; int32_t margin;
    int32_t* lo; int32_t* hi; int32_t* reason;
};

constexpr long long kNone = -(1ll << 62);              // below every window bound and every line index
// kOmit: forced_page_common.h's kMaxChars and kMaxFrames (ta_page_windows_omit.hip holds them equal)
constexpr int kWinMaxChars = 1 << 20;
constexpr long long kWinMaxFrames = 1ll << 25;

// one sweep over the page's lines; kStore: lo / hi are written.  Returns (wave-uniform) whether a window is wider than
// TA_FORCED_MAX_TARGET; *frames: the page's timesteps
template <bool kStore>
__device__ __forceinline__ bool sweep(const WinArgs& a, int64_t l0, int nl, int n, int lane, long long* s_lo, long long* s_hi,
                                      long long* frames) {
    long long carry_last = -1, carry_hi = kNone;       // the latest line with a core, the running maximum of hi: all lanes
    long long lo_prev = 0, hi_prev = 0;                // lane 0's: the line in front of the tile
    long long tsum = 0;
    bool wide = false;
    for (int base = 0; base < nl; base += 64) {
        const int k = base + lane;
        const bool in = k < nl;
        const int32_t* row = a.table + (l0 + (in ? k : 0)) * TA_HARVEST_FIELDS;
        const int reason = in ? row[0] : TA_HARVEST_EMPTY;
        const bool text = in && (reason & (TA_HARVEST_EMPTY | TA_HARVEST_PAGE)) == 0;
        long long last = wave_max_scan(text ? (long long)k : -1);
        last = last > carry_last ? last : carry_last;
        long long end = 0;
        if (in && last >= 0) {
            const int32_t* r = a.table + (l0 + last) * TA_HARVEST_FIELDS;
            end = (long long)r[1] + r[2];
        }
        const long long start = text ? (long long)row[1] : end;
        long long lo = start - a.margin > 0 ? start - a.margin : 0;
        long long hi = end + a.margin < n ? end + a.margin : n;
        if (k == 0) lo = 0;
        if (k == nl - 1) hi = n;
        hi = wave_max_scan(in ? hi : kNone);
        hi = hi > carry_hi ? hi : carry_hi;
        if (in) tsum += a.T[l0 + k];
        wave_lds_sync();                               // the tile before has been read
        s_lo[lane] = lo;
        s_hi[lane] = hi;
        wave_lds_sync();
        if (lane == 0) {                               // the clamps, line after line
            const int cnt = nl - base < 64 ? nl - base : 64;
            for (int j = 0; j < cnt; ++j) {
                long long x = s_lo[j];
                if (base + j > 0) {
                    x = x > lo_prev ? x : lo_prev;
                    x = x < hi_prev ? x : hi_prev;
                }
                s_lo[j] = x;
                lo_prev = x;
                hi_prev = s_hi[j];
            }
        }
        wave_lds_sync();
        lo = s_lo[lane];
        wide |= in && hi - lo > TA_FORCED_MAX_TARGET;
        if (kStore && in) {
            a.lo[l0 + k] = (int32_t)lo;
            a.hi[l0 + k] = (int32_t)hi;
        }
        if (lane == 63) s_hi[64] = last;               // after an inclusive scan lane 63 holds the tile's
        wave_lds_sync();
        carry_last = s_hi[64];
        carry_hi = s_hi[63];
    }
    wave_lds_sync();
    s_hi[lane] = tsum;
    wave_lds_sync();
    long long total = 0;
    for (int j = 0; j < 64; ++j) total += s_hi[j];
    *frames = total;
    return __any(wide);
}

template <bool kOmit>
__global__ __launch_bounds__(64) void page_windows_kernel(WinArgs a) {
    __shared__ long long s_lo[64];
    __shared__ long long s_hi[65];                     // [64]: the latest line with a core, from tile to tile
    const int b = blockIdx.x, lane = threadIdx.x;
    auto leave = [&](int reason) {
        if (lane == 0) a.reason[b] = reason;
    };
    const int64_t l0 = a.line_first[b], l1 = a.line_first[b + 1], c0 = a.t_off[b], c1 = a.t_off[b + 1];
    if (l0 < 0 || l1 < l0 || l1 > a.nlines || c0 < 0 || c1 < c0 || c1 > a.t_len || c1 - c0 > INT32_MAX)
        return leave(TA_PAGE_WINDOWS_BOUNDS);          // wave-uniform, as every exit below
    const int nl = (int)(l1 - l0), n = (int)(c1 - c0);
    if (!a.plain[b]) return leave(TA_PAGE_SCOPE_NOT_PLAIN);
    if (a.h_status[b] != TA_HARVEST_OK) return leave(TA_PAGE_SCOPE_HARVEST);
    bool zero = false;
    for (int64_t i = lane; i < n; i += 64) zero |= a.t_class[c0 + i] == 0;
    if (__any(zero)) return leave(TA_PAGE_SCOPE_CLASS0);
    if (n < 1) return leave(TA_PAGE_SCOPE_NO_TEXT);
    if (nl < 1) return leave(TA_PAGE_SCOPE_WINDOWS);
    long long frames;
    if (sweep<false>(a, l0, nl, n, lane, s_lo, s_hi, &frames)) return leave(TA_PAGE_SCOPE_WINDOWS);
    if constexpr (kOmit) {
        if (n > kWinMaxChars || frames > kWinMaxFrames) return leave(TA_PAGE_SCOPE_TOO_LONG);
    } else {
        if (n > frames) return leave(TA_PAGE_SCOPE_FRAMES);
    }
    sweep<true>(a, l0, nl, n, lane, s_lo, s_hi, &frames);
    leave(TA_PAGE_SCOPE_REFINED);
}

// the body of both entries: the host refusals, one launch, a wave per page
template <bool kOmit>
inline int page_windows_launch(const int32_t* table, const int32_t* harvest_status, const int64_t* line_first,
                               const int64_t* t_off, const int32_t* t_class, const int32_t* T, const uint8_t* plain,
                               int32_t npages, int32_t nlines, int64_t t_len, int32_t margin, int32_t* lo, int32_t* hi,
                               int32_t* reason, void* stream) {
    if (npages < 0 || nlines < 0 || t_len < 0) return ta_fail(TA_EINVAL, "negative size");
    if (margin < 0) return ta_fail(TA_EINVAL, "negative margin");
    if (npages == 0) return TA_OK;
    if (!table || !harvest_status || !line_first || !t_off || !t_class || !T || !plain || !lo || !hi || !reason)
        return ta_fail(TA_EINVAL, "null pointer argument");
    const WinArgs a{table, harvest_status, line_first, t_off, t_class, T, plain, npages, nlines, t_len, margin, lo, hi, reason};
    hipLaunchKernelGGL(page_windows_kernel<kOmit>, dim3((unsigned)npages), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "page_windows_kernel launch");
    return TA_OK;
}

}  // namespace
