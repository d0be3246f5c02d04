// ta_refine_conf.hip -- the refined lines' per-character confidences spread over the pages' transcript characters and
// reduced per syllable, on the device ("Inside the pipeline"): what forced.refine_pages does in
// Python behind its confidence call, as ONE launch behind ta_forced_confidence_lines and ta_refine_columns on the same
// stream.  Integers only; the checker of record is tests/refine_conf_ref.py.
//
// confidence_pages_kernel, one wave per page:
//   check    the page's own device numbers; a lane per line: every refined line has a filled slot whose confidence status
//            is TA_FORCED_OK, whose labels lie inside label_cap and whose kept characters table[q][1] .. + L[k] lie inside
//            the page's; a lane per syllable: its range lies inside the page's characters.  A page that fails gets its
//            status and NOTHING else of it is written.
//   fill     char_conf of the page's characters = TA_NO_CONFIDENCE
//   spread   line after line (wave-uniform), a lane per kept character: char_conf[t_off[p] + table[q][1] + i] =
//            confidence[lab_off[k] + i].  ta_refine_columns holds the refined lines' kept ranges inside disjoint runs, so
//            no character is written twice.
//   reduce   a lane per syllable: the smallest char_conf of its range among those that are not TA_NO_CONFIDENCE, else
//            TA_NO_CONFIDENCE.  A plain comparison of int64: the values may be 0 or negative.
// char_conf is read back by other lanes than wrote it: a fence and a barrier stand between the steps.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kF = TA_HARVEST_FIELDS;

struct ConfPagesArgs {
    const int64_t* confidence; const int64_t* lab_off; const int32_t* L; const int64_t* count; const int32_t* c_status;
    int32_t nslots; int64_t label_cap;
    const int32_t* table; const int64_t* line_first; const int32_t* refined; const int32_t* slot; int32_t nlines;
    const int64_t* t_off; int64_t t_len;
    const int32_t* syl_first; const int32_t* syl_last; const int64_t* syl_off; int64_t nsyl;
    int64_t* char_conf; int64_t* syl_conf; int32_t* status;
};

__global__ __launch_bounds__(64) void confidence_pages_kernel(ConfPagesArgs a) {
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
    for (int64_t i = t0 + lane; i < t1; i += 64) a.char_conf[i] = TA_NO_CONFIDENCE;
    __threadfence();                                    // the same words are written again below, by other lanes
    __syncthreads();
    for (int64_t q = lf0; q < lf1; ++q) {
        if (__builtin_amdgcn_readfirstlane(a.refined[q]) == 0) continue;
        const int k = __builtin_amdgcn_readfirstlane(a.slot[q]);
        const int Lk = __builtin_amdgcn_readfirstlane(a.L[k]);
        const int64_t l0 = a.lab_off[k], at = t0 + a.table[kF * q + 1];
        for (int i = lane; i < Lk; i += 64) a.char_conf[at + i] = a.confidence[l0 + i];
    }
    __threadfence();                                    // char_conf is read back below, by other lanes
    __syncthreads();

    // ---- reduce ----------------------------------------------------------------------------------------------------------------
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t j = base + lane;
        if (j < s1) {
            const int f = a.syl_first[j], l = a.syl_last[j];
            int64_t best = TA_NO_CONFIDENCE;
            for (int i = f; i <= l; ++i) {
                const int64_t c = a.char_conf[t0 + i];
                if (c != TA_NO_CONFIDENCE && (best == TA_NO_CONFIDENCE || c < best)) best = c;
            }
            a.syl_conf[j] = best;
        }
    }
    if (lane == 0) a.status[p] = TA_CONF_PAGES_OK;
}

}  // namespace

extern "C" int ta_confidence_pages(const int64_t* confidence, const int64_t* lab_off, const int32_t* L, const int64_t* count,
                                   const int32_t* conf_status, int32_t nslots, int64_t label_cap, const int32_t* table,
                                   const int64_t* line_first, const int32_t* refined, const int32_t* slot, int32_t nlines,
                                   const int64_t* t_off, int64_t t_len, const int32_t* syl_first, const int32_t* syl_last,
                                   const int64_t* syl_off, int64_t nsyl, int32_t nprob, int64_t* char_conf,
                                   int64_t* syl_conf, int32_t* status, void* stream) {
    if (nprob < 0 || nlines < 0 || nslots < 0 || label_cap < 0 || t_len < 0 || nsyl < 0)
        return ta_fail(TA_EINVAL, "negative size");
    if (nlines > TA_HARVEST_MAX_LINES) return ta_fail(TA_ELIMIT, "more than TA_HARVEST_MAX_LINES lines");
    if (nprob == 0) return TA_OK;
    if (!confidence || !lab_off || !L || !count || !conf_status || !table || !line_first || !refined || !slot || !t_off ||
        !syl_first || !syl_last || !syl_off || !char_conf || !syl_conf || !status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    const ConfPagesArgs a{confidence, lab_off, L, count, conf_status, nslots, label_cap, table, line_first, refined, slot,
                          nlines, t_off, t_len, syl_first, syl_last, syl_off, nsyl, char_conf, syl_conf, status};
    hipLaunchKernelGGL(confidence_pages_kernel, dim3((unsigned)nprob), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "confidence_pages_kernel launch");
    return TA_OK;
}
