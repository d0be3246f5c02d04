// ta_page_windows.hip -- page scope inside the pipeline: per page whether it is eligible for
// ta_forced_align_pages_gated, and per line of an eligible page the window of transcript characters [lo, hi) the page's one
// path may put on it -- forced.page_scope_eligibility and forced.page_windows (checker tests/forced_page_ref.py's
// page_windows) on the device, from the harvest table where ta_harvest_lines left it.  Integers only.
//
// page_windows_kernel, one wave per page, one launch per chunk.  A page has no bound on its lines: they go through the wave
// in tiles of 64, a line per lane, the carries from tile to tile in registers.
//   core    a row without EMPTY / PAGE has the core [t_first, t_first + L); any other line the empty range at the end of the
//           LATEST earlier line with a core (0 in front of the first).  "Latest" is a wave max-scan over the line indices of
//           the rows with a core (carry: the latest of the tiles before); the end is then read from that row.
//   margin  lo = max(start - margin, 0), hi = min(end + margin, n), lo_0 = 0, hi_last = n, in 64 bits.
//   hi      a running maximum: wave_max_scan, carry the maximum of the tiles before.
//   lo      lo_k = min(max(lo_k, lo_{k-1}), hi_{k-1}): a composition of clamps.  It is a short SERIAL pass on lane 0 over the
//           tile's values in LDS, not a scan: the pass is 64 steps of two compares on a page that has some twenty lines,
//           behind it stands an aligner that takes milliseconds, and a clamp scan would need the pair (a, b) moved through
//           six DPP steps with a composition rule that is easy to get wrong at equal bounds.
// The lines are swept twice: the first sweep only finds the widest window and the page's frames (nothing is written, a page
// with a reason keeps every word of its lo / hi), the second writes.  Every offset the kernel reads through is checked on the
// device's own numbers first: a page whose line_first or t_off leave nlines / t_len or decrease gets TA_PAGE_WINDOWS_BOUNDS
// and nothing else of it is read or written.
// The kernel is page_windows.h's page_windows_kernel<kOmit>, which ta_page_windows_omit.hip instantiates for the lattice with
// omission; this unit holds the strict rule's instantiation alone (profiles/forced_page_omit_gated.txt).
#include "page_windows.h"

extern "C" int ta_page_windows(const int32_t* table, const int32_t* harvest_status, const int64_t* line_first,
                               const int64_t* t_off, const int32_t* t_class, const int32_t* T, const uint8_t* plain,
                               int32_t npages, int32_t nlines, int64_t t_len, int32_t margin, int32_t* lo, int32_t* hi,
                               int32_t* reason, void* stream) {
    return page_windows_launch<false>(table, harvest_status, line_first, t_off, t_class, T, plain, npages, nlines, t_len,
                                      margin, lo, hi, reason, stream);
}
