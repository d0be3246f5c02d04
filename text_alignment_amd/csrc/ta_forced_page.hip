// ta_forced_page.hip -- page-scope forced alignment: ONE best CTC path through the frames of all
// the lines of a page, so that the lattice, not the decoder's output, decides which transcript character lies on which
// line.  Integers only from the float32 probabilities on; the checker of record is tests/forced_page_ref.py.
//
// forced_page_kernel<K> (forced_page_strict.h: the kernel is instantiated here and, gated, in ta_forced_page_gated.hip), one
// wave per page: the page is one chain of dependent steps.  The page's labels give the states
// 0 .. 2 n; during the frames of line k only the states of its window of characters [lo_k, hi_k) are live, 2 lo_k ..
// 2 hi_k.  Lane l holds the K consecutive WINDOW states l K .. l K + K - 1 (page state minus 2 lo_k) as int64 registers;
// K = 2 .. 32 from the page's widest window (forced_k), even, and a window starts at an even page state, so blanks stay
// in even registers whatever the window.  The kernel reads as prologue, cell, boundary hook, end rule over
// forced_page_common.h, which it shares with ta_forced_page_omit.hip:
//   head   page_head: every bound re-checked on the page's own device numbers before anything is read through it; then
//          the exit of a page that belongs to another launch, and labels_ok.
//   fill   page_fill over StrictCell: the cell is forced_step.  At a line boundary StrictCell::leave masks the old window
//          into vbuf (states outside it NEG) and page_fill brings the values back shifted; the first frame of a line runs
//          the step in which a label state has no stay candidate (kFirst): no character spans a line break.  Registers
//          beyond the window's last state hold values no live state ever reads (a state depends on lower states only) and
//          are masked at the next boundary.  A state without a live source drifts below NEG instead of staying there; it
//          can never reach a state with a path (a path costs less than 2^21 per frame), and its moves are never walked.
//   end    the better of the last two states, on a tie the last blank.  A page whose best end is below kDead has no path:
//          TA_FORCED_NOPATH, nothing but its status is written.
//   walk   page_walk<K, false>, then page_peaks<false>.
#include "forced_page_strict.h"

extern "C" int64_t ta_forced_page_workspace_bytes(int32_t nl, const int32_t* T, int32_t K) {
    return page_workspace_bytes(nl, T, K, forced_ws_rows);
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
    int variants;
    const int rc2 = forced_check_pages(T_host, line_first_host, lo_host, hi_host, lab_off_host, npages, nlines, rows, nlabels,
                                       workspace_bytes, forced_ws_rows, kMaxText, "a page's text is too long", INT64_MAX, nullptr,
                                       "ta_forced_page_workspace_bytes", &variants);
    if (rc2 != TA_OK) return rc2;
    const PageArgs a{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                     nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status, 0};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_kernel launch");
    return TA_OK;
}
