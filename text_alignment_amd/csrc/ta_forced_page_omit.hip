// ta_forced_page_omit.hip -- page-scope forced alignment whose path may OMIT characters of the text at a price per
// character: ONE best path through the frames of all the lines of a page (section 14.8) on the
// lattice with the far move (section 14.9), so that a character the scribe never wrote takes no frame from its
// neighbours, on its own line or across a line break.  Integers only from the float32 probabilities on; the checker of
// record is tests/forced_page_omit_ref.py.
//
// forced_page_omit_kernel<K>, one wave per page, laid out as forced_page_kernel<K>: lane l holds the WINDOW states
// l K .. l K + K - 1 (page state minus 2 lo_k) as int64, K from the page's widest window, one launch per variant.  The
// prologue, the fill's control structure, the walk and the peaks are forced_page_common.h's, the strict page kernel's;
// the seed, the cell, the bit words, the end rule and the far move's source are forced_common.h's, the line kernel's
// (ta_forced_omit.hip).  What is this file's own:
//   head    the price's range in front of page_head, and the page's frames summed through LDS for it (kMaxFrames).
//   cell    OmitCell: omit_step with a[x] = v[x] + omit * ceil(x / 2) formed in WINDOW coordinates: a window starts at an
//           even page state, so another window's coordinates add the same omit * d to both sides of every comparison.
//   break   OmitCell::leave.  The first frame of a line k >= 1 takes its far candidates from the OLD window, the
//           2 (lo_k - lo_{k-1}) states that fall off the front included.  Before the re-basing the old registers are
//           masked to the old window and scanned in old coordinates; that scan's bits are the line's bit row of frame 0,
//           and its prefix maxima Pm go through LDS beside v (pbuf).  The first frame's state of window character i reads
//           Pm[2 i + d - 2] - omit * (i + d / 2), d = 2 (lo_k - lo_{k-1}), and a label state has no stay candidate.
//   start   every state of window 0 may start the path, the characters in front paid for (omit_seed).
//   end     omit_end over s <= 2 n of the last window.
//   walk    page_walk<K, true>.  The frames are set to -1 before the fill; the characters a far move jumps keep the -1,
//           and page_peaks<true> leaves such a row alone.
// Workspace of line k: forced_ws_rows(T_k, K) rows of 64 move words, then omit_bit_rows(T_k, K) rows of 64 bit words as
// ta_forced_omit.hip lays them out; frame 0's bits are the boundary scan's, so the first-frame bit row needs no room of its
// own.  256-byte rows, plain vector stores.
// Limits: n <= 2^20 characters and at most 2^25 frames per page, so omit * n + 2^21 * frames < 2^48 and nothing approaches
// -2^49; under the rule every page has a path (the checker's docstring), TA_FORCED_NOPATH is kept for a score below -2^49
// all the same.  A refused page gets a status and touches nothing else.
// All five variants are built; K = 32 holds its values in 256 VGPRs and 125 AGPRs and 57 KiB of LDS, without scratch.
// The kernel itself stands in forced_page_omit.h, which ta_forced_page_omit_gated.hip instantiates as well.
#include "forced_page_omit.h"

extern "C" int64_t ta_forced_page_omit_workspace_bytes(int32_t nl, const int32_t* T, int32_t K) {
    return page_workspace_bytes(nl, T, K, page_omit_rows);
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
    int variants;
    const int rc2 = forced_check_pages(T_host, line_first_host, lo_host, hi_host, lab_off_host, npages, nlines, rows, nlabels,
                                       workspace_bytes, page_omit_rows, kMaxChars, "a page's text has more than 2^20 characters",
                                       kMaxFrames, "a page has more than 2^25 frames", "ta_forced_page_omit_workspace_bytes",
                                       &variants);
    if (rc2 != TA_OK) return rc2;
    const PageArgs a{probs, row_off, T, line_first, lo, hi, labels, lab_off, ws_off, npages, nlines, no, variants, rows,
                     nlabels, static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status, omit_q};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_page_omit_kernel<decltype(kc)::value>), dim3((unsigned)a.npages), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_page_omit_kernel launch");
    return TA_OK;
}
