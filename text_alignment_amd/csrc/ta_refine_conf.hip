// ta_refine_conf.hip -- the refined lines' per-character confidences ("Inside the pipeline") and
// posteriors (section 14.11, "Inside the pipeline") spread over the pages' transcript characters and reduced per syllable,
// on the device: what forced.refine_pages does in Python behind its confidence / posterior call, as ONE launch each behind
// ta_forced_confidence_lines / ta_forced_posterior_lines and ta_refine_columns on the same stream.  One kernel body, two
// kinds of value:
//   ConfValues   the int64 confidence[lab_off[k] + i] as it is; "no value" is TA_NO_CONFIDENCE; a plain comparison of
//                int64 (the values may be 0 or negative).  Integers only; the checker is tests/refine_conf_ref.py.
//   PostValues   ldexp(own_m[lab_off[k] + i] / z_m[k], own_x[lab_off[k] + i] - z_x[k]): ONE IEEE double division and one
//                ldexp, the arithmetic of forced.posterior_values (no reciprocal, no fast-math; a result in the subnormal
//                range is rounded once, by ldexp).  "No value" is TA_NO_POSTERIOR, numpy's np.nan, written as a 64-bit
//                word; a value is one that is no NaN; a comparison of doubles.  The checker is tests/refine_post_ref.py.
//
// pages_kernel<V>, one wave per page; out and syl_out hold 64-bit words of either kind:
//   check    the page's own device numbers; a lane per line: every refined line has a filled slot whose status is
//            TA_FORCED_OK, whose labels lie inside label_cap and whose kept characters table[q][1] .. + L[k] lie inside
//            the page's; a lane per syllable: its range lies inside the page's characters.  A page that fails gets its
//            status and NOTHING else of it is written.
//   fill     out of the page's characters = "no value"
//   spread   line after line (wave-uniform), a lane per kept character: out[t_off[p] + table[q][1] + i] = the value of
//            character i of slot k.  ta_refine_columns holds the refined lines' kept ranges inside disjoint runs, so no
//            character is written twice.
//   reduce   a lane per syllable: the smallest value of its range, else "no value".
// out is read back by other lanes than wrote it: a fence and a barrier stand between the steps.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kF = TA_HARVEST_FIELDS;

struct ConfValues {
    const int64_t* confidence;
    static __device__ __forceinline__ int64_t none() { return TA_NO_CONFIDENCE; }
    static __device__ __forceinline__ bool has(int64_t w) { return w != TA_NO_CONFIDENCE; }
    static __device__ __forceinline__ bool less(int64_t a, int64_t b) { return a < b; }
    __device__ __forceinline__ int64_t at(int k, int64_t row) const { return confidence[row]; }
};

__device__ __forceinline__ double as_double(int64_t w) { double d; __builtin_memcpy(&d, &w, 8); return d; }

struct PostValues {
    const double* own_m; const int32_t* own_x; const double* z_m; const int32_t* z_x;
    static __device__ __forceinline__ int64_t none() { return TA_NO_POSTERIOR; }
    static __device__ __forceinline__ bool has(int64_t w) { return !isnan(as_double(w)); }
    static __device__ __forceinline__ bool less(int64_t a, int64_t b) { return as_double(a) < as_double(b); }
    __device__ __forceinline__ int64_t at(int k, int64_t row) const {
        const double v = ldexp(own_m[row] / z_m[k], own_x[row] - z_x[k]);
        int64_t w;
        __builtin_memcpy(&w, &v, 8);
        return w;
    }
};

template <class V>
struct PagesArgs {
    V values; const int64_t* lab_off; const int32_t* L; const int64_t* count; const int32_t* c_status;
    int32_t nslots; int64_t label_cap;
    const int32_t* table; const int64_t* line_first; const int32_t* refined; const int32_t* slot; int32_t nlines;
    const int64_t* t_off; int64_t t_len;
    const int32_t* syl_first; const int32_t* syl_last; const int64_t* syl_off; int64_t nsyl;
    int64_t* out; int64_t* syl_out; int32_t* status;
};

template <class V>
__global__ __launch_bounds__(64) void pages_kernel(PagesArgs<V> a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = a.t_off[p], t1 = a.t_off[p + 1], s0 = a.syl_off[p], s1 = a.syl_off[p + 1];
    const int64_t lf0 = a.line_first[p], lf1 = a.line_first[p + 1];
    // ---- check -------------------------------------------------------------------------------------------------------------
    const bool inside = lf0 >= 0 && lf0 <= lf1 && lf1 <= a.nlines && t0 >= 0 && t1 >= t0 && t1 <= a.t_len &&
                        t1 - t0 <= TA_HARVEST_MAX_COLUMNS && s0 >= 0 && s1 >= s0 && s1 <= a.nsyl;
    if (!inside) {
        if (lane == 0) a.status[p] = TA_CONF_PAGES_BOUNDS;
        return;
    }
    const int n = __builtin_amdgcn_readfirstlane((int)(t1 - t0));
    int64_t filled = a.count[0];
    filled = filled < 0 ? 0 : filled > a.nslots ? a.nslots : filled;
    bool noslot = false, notok = false, tbad = false, rbad = false;
    for (int64_t base = lf0; base < lf1; base += 64) {
        const int64_t q = base + lane;
        if (q < lf1 && a.refined[q] != 0) {
            const int k = a.slot[q];
            if (k < 0 || k >= filled) noslot = true;
            else if (a.c_status[k] != TA_FORCED_OK) notok = true;
            else {
                const int64_t l0 = a.lab_off[k];
                const int Lk = a.L[k], tf = a.table[kF * q + 1];
                tbad |= Lk < 1 || l0 < 0 || l0 + Lk > a.label_cap || tf < 0 || (int64_t)tf + Lk > n;
            }
        }
    }
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t j = base + lane;
        if (j < s1) {
            const int f = a.syl_first[j], l = a.syl_last[j];
            rbad |= f < 0 || l < f || l >= n;
        }
    }
    const int st = __any(rbad) ? TA_CONF_PAGES_RANGE : __any(tbad) ? TA_CONF_PAGES_TABLE : __any(noslot) ? TA_CONF_PAGES_SLOT :
                   __any(notok) ? TA_CONF_PAGES_STATUS : TA_CONF_PAGES_OK;
    if (st != TA_CONF_PAGES_OK) {
        if (lane == 0) a.status[p] = st;
        return;
    }

    // ---- fill, spread --------------------------------------------------------------------------------------------------------
    for (int64_t i = t0 + lane; i < t1; i += 64) a.out[i] = V::none();
    __threadfence();                                    // the same words are written again below, by other lanes
    __syncthreads();
    for (int64_t q = lf0; q < lf1; ++q) {
        if (__builtin_amdgcn_readfirstlane(a.refined[q]) == 0) continue;
        const int k = __builtin_amdgcn_readfirstlane(a.slot[q]);
        const int Lk = __builtin_amdgcn_readfirstlane(a.L[k]);
        const int64_t l0 = a.lab_off[k], at = t0 + a.table[kF * q + 1];
        for (int i = lane; i < Lk; i += 64) a.out[at + i] = a.values.at(k, l0 + i);
    }
    __threadfence();                                    // out is read back below, by other lanes
    __syncthreads();

    // ---- reduce ----------------------------------------------------------------------------------------------------------------
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t j = base + lane;
        if (j < s1) {
            const int f = a.syl_first[j], l = a.syl_last[j];
            int64_t best = V::none();
            for (int i = f; i <= l; ++i) {
                const int64_t c = a.out[t0 + i];
                if (V::has(c) && (!V::has(best) || V::less(c, best))) best = c;
            }
            a.syl_out[j] = best;
        }
    }
    if (lane == 0) a.status[p] = TA_CONF_PAGES_OK;
}

// what both entries refuse, and their one launch
template <class V>
int pages_call(bool null_values, const PagesArgs<V>& a, int32_t nprob, const char* where, void* stream) {
    if (nprob < 0 || a.nlines < 0 || a.nslots < 0 || a.label_cap < 0 || a.t_len < 0 || a.nsyl < 0)
        return ta_fail(TA_EINVAL, "negative size");
    if (a.nlines > TA_HARVEST_MAX_LINES) return ta_fail(TA_ELIMIT, "more than TA_HARVEST_MAX_LINES lines");
    if (nprob == 0) return TA_OK;
    if (null_values || !a.lab_off || !a.L || !a.count || !a.c_status || !a.table || !a.line_first || !a.refined || !a.slot ||
        !a.t_off || !a.syl_first || !a.syl_last || !a.syl_off || !a.out || !a.syl_out || !a.status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    hipLaunchKernelGGL(pages_kernel<V>, dim3((unsigned)nprob), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, where);
    return TA_OK;
}

}  // namespace

extern "C" int ta_confidence_pages(const int64_t* confidence, const int64_t* lab_off, const int32_t* L, const int64_t* count,
                                   const int32_t* conf_status, int32_t nslots, int64_t label_cap, const int32_t* table,
                                   const int64_t* line_first, const int32_t* refined, const int32_t* slot, int32_t nlines,
                                   const int64_t* t_off, int64_t t_len, const int32_t* syl_first, const int32_t* syl_last,
                                   const int64_t* syl_off, int64_t nsyl, int32_t nprob, int64_t* char_conf,
                                   int64_t* syl_conf, int32_t* status, void* stream) {
    const PagesArgs<ConfValues> a{{confidence}, lab_off, L, count, conf_status, nslots, label_cap, table, line_first, refined,
                                  slot, nlines, t_off, t_len, syl_first, syl_last, syl_off, nsyl, char_conf, syl_conf, status};
    return pages_call(!confidence, a, nprob, "confidence_pages_kernel launch", stream);
}

extern "C" int ta_posterior_pages(const double* own_m, const int32_t* own_x, const double* z_m, const int32_t* z_x,
                                  const int64_t* lab_off, const int32_t* L, const int64_t* count, const int32_t* post_status,
                                  int32_t nslots, int64_t label_cap, const int32_t* table, const int64_t* line_first,
                                  const int32_t* refined, const int32_t* slot, int32_t nlines, const int64_t* t_off,
                                  int64_t t_len, const int32_t* syl_first, const int32_t* syl_last, const int64_t* syl_off,
                                  int64_t nsyl, int32_t nprob, double* char_post, double* syl_post, int32_t* status,
                                  void* stream) {
    const PagesArgs<PostValues> a{{own_m, own_x, z_m, z_x}, lab_off, L, count, post_status, nslots, label_cap, table,
                                  line_first, refined, slot, nlines, t_off, t_len, syl_first, syl_last, syl_off, nsyl,
                                  reinterpret_cast<int64_t*>(char_post), reinterpret_cast<int64_t*>(syl_post), status};
    return pages_call(!own_m || !own_x || !z_m || !z_x, a, nprob, "posterior_pages_kernel launch", stream);
}
