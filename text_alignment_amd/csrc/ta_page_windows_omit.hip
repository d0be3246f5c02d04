// ta_page_windows_omit.hip -- ta_page_windows for the lattice with omission: page_windows.h's
// kernel with kOmit = true, the rule forced.page_scope_eligibility(..., omit=True).  Reasons 1 - 5, their precedence, the
// windows and TA_PAGE_WINDOWS_BOUNDS are the strict entry's; TA_PAGE_SCOPE_FRAMES never occurs (every page has a path), and
// behind TA_PAGE_SCOPE_WINDOWS a page of more than 2^20 characters or 2^25 frames is TA_PAGE_SCOPE_TOO_LONG -- what
// ta_forced_align_pages_omit_gated would refuse.  A unit of its own: see page_windows.h.
#include "forced_page_common.h"
#include "page_windows.h"

static_assert(kWinMaxChars == kMaxChars && kWinMaxFrames == kMaxFrames, "the windows kernel and the aligner hold one limit");

extern "C" int ta_page_windows_omit(const int32_t* table, const int32_t* harvest_status, const int64_t* line_first,
                                    const int64_t* t_off, const int32_t* t_class, const int32_t* T, const uint8_t* plain,
                                    int32_t npages, int32_t nlines, int64_t t_len, int32_t margin, int32_t* lo, int32_t* hi,
                                    int32_t* reason, void* stream) {
    return page_windows_launch<true>(table, harvest_status, line_first, t_off, t_class, T, plain, npages, nlines, t_len,
                                     margin, lo, hi, reason, stream);
}
