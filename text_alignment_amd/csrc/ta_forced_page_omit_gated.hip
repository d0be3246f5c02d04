// ta_forced_page_omit_gated.hip -- the page aligner with omission without host windows:
// forced_page_omit.h's kernel with Args = GatedPageArgs, behind ta_page_windows_omit in the pipeline.  The host knows no
// window: it sizes every line's piece of the workspace by its page's cap -- move rows and bit rows each never decrease with
// the variant, so the piece holds whatever variant the device's windows call for -- and launches every variant up to the
// widest cap's; the device's windows pick the variant.  A unit of its own: see forced_page_omit.h.
#include "forced_page_omit.h"

extern "C" int64_t ta_forced_page_omit_gated_workspace_bytes(int32_t nl, const int32_t* T, int32_t cap) {
    if (cap < 0 || cap > TA_FORCED_MAX_TARGET) return -1;
    return page_workspace_bytes(nl, T, window_k(cap), page_omit_rows);
}

extern "C" int ta_forced_align_pages_omit_gated(const float* probs, const int64_t* row_off, const int32_t* T,
                                                const int64_t* line_first, const int32_t* lo, const int32_t* hi,
                                                const int32_t* labels, const int64_t* lab_off, const int64_t* ws_off,
                                                const int32_t* gate, const int32_t* cap, int32_t npages, int32_t nlines,
                                                int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                                                const int64_t* line_first_host, const int64_t* lab_off_host,
                                                const int32_t* cap_host, int32_t omit_q, void* workspace,
                                                int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status,
                                                void* stream) {
    bool go;
    const int rc = forced_preamble(npages < 0 || nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no,
                                   omit_q < 0 || omit_q > TA_FORCED_OMIT_MAX ? "omit_q outside 0 .. TA_FORCED_OMIT_MAX" : nullptr,
                                   npages == 0,
                                   !probs || !row_off || !T || !line_first || !lo || !hi || !labels || !lab_off || !ws_off ||
                                       !gate || !cap || !T_host || !line_first_host || !lab_off_host || !cap_host ||
                                       !workspace || !frames || !score || !status,
                                   workspace, &go);
    if (!go) return rc;
    // forced_check_pages' refusals that need no window, with the limits of the lattice with omission; a page without lines
    // or without text is the gate's to pass over
    if (line_first_host[0] != 0 || line_first_host[npages] != nlines) return ta_fail(TA_EINVAL, "line_first does not run from 0 to nlines");
    if (lab_off_host[0] < 0 || lab_off_host[npages] > nlabels) return ta_fail(TA_EINVAL, "the pages' texts exceed nlabels");
    int64_t need = 0, sum_t = 0;
    int capmax = 0;
    for (int p = 0; p < npages; ++p) {
        const int64_t l0 = line_first_host[p], l1 = line_first_host[p + 1], n = lab_off_host[p + 1] - lab_off_host[p];
        if (l1 < l0 || l1 > nlines) return ta_fail(TA_EINVAL, "line_first decreases");     // (beyond nlines: it has to, later)
        if (n < 0) return ta_fail(TA_EINVAL, "lab_off decreases");
        if (n > kMaxChars) return ta_fail(TA_ELIMIT, "a page's text has more than 2^20 characters");
        const int w = cap_host[p];
        if (w < 0) return ta_fail(TA_EINVAL, "a negative cap");
        if (w > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a cap of more than TA_FORCED_MAX_TARGET characters");
        int64_t page_t = 0;
        for (int64_t q = l0; q < l1; ++q) {
            const int t = T_host[q];
            if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
            if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
            page_t += t;
            need += 256 * page_omit_rows(t, window_k(w));
        }
        if (page_t > kMaxFrames) return ta_fail(TA_ELIMIT, "a page has more than 2^25 frames");
        sum_t += page_t;
        capmax = w > capmax ? w : capmax;
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (workspace_bytes < need) return forced_ws_small("pages", "ta_forced_page_omit_gated_workspace_bytes");
    const int variants = variants_up_to(window_k(capmax));
    const GatedPageArgs a{{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                           nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status, omit_q},
                          gate, cap};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_omit_kernel<decltype(kc)::value, GatedPageArgs>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_omit_kernel (gated) launch");
    return TA_OK;
}
