/*
 * text_alignment_amd.h -- C ABI of libta_hip.so, the MI355X (gfx950) hot path of
 * DDMAL/text_alignment.
 *
 * The reference has no FFI on this path: its boundary is two Python calls and one shell
 * command.  Each entry point below names the reference interface
 * whose arithmetic it replaces; the Python mirror of that interface lives in
 * text_alignment_amd/ and binds these symbols with ctypes.
 *
 * Conventions: plain pointers and sizes only; every pointer marked [dev] is a device
 * (HBM) address owned by the caller; [host] is host memory.  `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Calls enqueue work and return without
 * synchronising.  Return value: 0 = ok, negative = TA_E*; ta_last_error() describes the
 * most recent failure on the calling thread.  The library keeps no mutable global state besides the
 * lazily loaded code object and one-time, thread-safe raises of kernels' dynamic-LDS limits.
 *
 * The Python binding is DERIVED from this file: text_alignment_amd/_abi.py parses it when the package is imported and
 * takes every ctypes signature and every TA_* constant from it, for the package and for the tests alike (hipcc holds
 * the definitions in csrc/ against it, so nothing is written down twice).  For that the file keeps to a rule: plain C
 * declarations `RET NAME(PARAMS);` over the stdint types, int, float, double, char, void and pointers to them -- no
 * typedefs, structs, function pointers or line continuations -- and constants as object-like macros
 * `#define TA_NAME <integer expression>` (literals, parentheses, unary minus, <<, other TA_ names, INT64_MIN;
 * function-like macros are for C callers only).  A declaration outside the rule is refused at import; if one is ever
 * needed, extend the parser.
 */
#ifndef TEXT_ALIGNMENT_AMD_H
#define TEXT_ALIGNMENT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TA_OK 0
#define TA_EINVAL (-1)    /* bad argument (null pointer, negative size, unsupported shape) */
#define TA_ERANGE (-2)    /* scores would overflow the integer fast path */
#define TA_EHIP (-3)      /* a HIP runtime call failed */
#define TA_ELIMIT (-4)    /* problem exceeds a kernel limit (LDS capacity) */

/* bit flags for ta_nw_batch */
#define TA_NW_FILL 1u
#define TA_NW_TRACEBACK 2u
#define TA_NW_CODES8 4u      /* caller asserts every token id < 255: 1-byte codes in LDS (ta_nw2_batch) */
#define TA_NW_WIDE 8u        /* ta_nw_batch: force one problem over several workgroups (HBM hand-off rows) */
#define TA_NW_NARROW 16u     /* ta_nw_batch: force one workgroup per problem; default: wide iff nprob < 256 */
#define TA_NW_OPENS_SAME 32u /* ta_nw2_batch hint: gap_open_x == gap_open_y in every scoring system of the batch */
/* ta_nw2_batch, score profile in LDS.  TA_NW_ALPHABET(a) with 1 <= a <= 254 makes two statements about the
 * batch, of different kinds:
 *   - a caller ASSERTION, like TA_NW_CODES8: every token id of every problem is < a.  It is not checked.  The
 *     OCR ids index the per-wave profile directly (row pitch 256 B, a + 1 rows), so an id >= a reads another
 *     wave's table or LDS beyond the profile and ids >= 256 wrap: the alignment comes out silently WRONG,
 *     not slower.  Derive `a` from the data (max id + 1), as text_alignment_amd.textSeqCompare.NWBatch does,
 *     or add TA_NW_CHECK_IDS while bringing a caller up.
 *   - HINTS that change speed only: every gap open is <= 0 and match/mismatch minus both gap extends fit a
 *     signed byte.  A problem that does not meet them (and, under TA_NW_OPENS_SAME, one whose two gap opens
 *     differ) is still aligned correctly, through the kernel's general cell.
 * Leave the field 0 (no profile: token ids are compared per cell) when the id bound is not known. */
#define TA_NW_ALPHABET_SHIFT 8
#define TA_NW_ALPHABET(a) (((uint32_t)(a) & 0xFFu) << TA_NW_ALPHABET_SHIFT)
/* ta_nw2_batch launch-shape overrides (tests, A/B timing): phase 1 without the score profile even where
 * the hints allow it; phase 1 with exactly w waves per workgroup (1, 2, 4 or 8; ignored when the tallest
 * problem has fewer strips or the LDS does not hold it; 0 = the library's own choice). */
/* ta_nw_batch launch-shape override (tests, timing): rows per lane of the one-pass fill, 1, 2 or 4 (0 = the
 * library's choice: 2 for batches too small to give every SIMD a 256-row strip, else 4; 1 -- 64-row
 * strips -- measured slower than 2 at every size tried and is never chosen).  Fill and traceback of
 * one batch must be given the same value (and the same nprob / max_n), also when issued as two calls. */
#define TA_NW_ROWS_SHIFT 20
#define TA_NW_ROWS(r) (((uint32_t)(r) & 0x7u) << TA_NW_ROWS_SHIFT)
/* ta_nw2_batch, traceback launch shape (tests, timing): waves per problem of phase 2 -- 1 (one wave walks the chunks
 * one after the other), 2 or 4 (the chunks along the path dealt to the waves of a workgroup, each re-filling the
 * chunk it expects ahead of the walk), 3 (TWO problems per wave, 32 lanes each, walking back half-strips of 128 rows:
 * large batches), 5 / 6 (both: two / four waves per pair of problems on half-strips: medium batches); 0 = the library's
 * choice by batch size.  Same results either way. */
#define TA_NW_TBWAVES_SHIFT 24
#define TA_NW_TBWAVES(w) (((uint32_t)(w) & 0x7u) << TA_NW_TBWAVES_SHIFT)
#define TA_NW_NO_PROFILE 64u
/* ta_nw2_batch, debug guard for the two caller assertions above (TA_NW_CODES8: ids < 255; TA_NW_ALPHABET(a): ids < a):
 * with this bit the call first checks every token id of the batch on the device, WAITS for the result (one synchronisation
 * of `stream` -- its scratch word is a stream-ordered allocation, so other streams of the device run on: not for timed code) and returns TA_EINVAL -- nothing else launched -- if an id breaks an assertion
 * the flags make.  Without it a violated assertion gives silently wrong alignments. */
#define TA_NW_CHECK_IDS 128u
#define TA_NW_WAVES_SHIFT 16
#define TA_NW_WAVES(w) (((uint32_t)(w) & 0xFu) << TA_NW_WAVES_SHIFT)

int ta_version(void);
const char* ta_last_error(void);
/* PCI address ("0000:c1:00.0", NUL-terminated, len >= 13) of HIP device `device` -- the key under /sys/bus/pci/devices/
 * from which a rank of the page-sharded job (the loop of alignToOCR.py:407-438, one process per GPU) reads the NUMA node
 * of its GPU to bind itself next to it.  [host] */
int ta_device_pci_bus_id(int32_t device, char* out, int32_t len);
/* n host arrays into one staging buffer in one call: nbytes[k] bytes from src[k] to dst + dst_off[k] (memcpy; all pointers
 * [host]).  How a chunk's text-line strips reach the page-locked buffer they cross PCIe from -- where the reference writes
 * each strip to a PNG file for the recogniser (alignToOCR.py:131-132) -- without the interpreter lock being taken per strip. */
int ta_host_copy_pieces(void* dst, const void* const* src, const int64_t* dst_off, const int64_t* nbytes, int32_t n);
/* Characters and boxes of every decoded line of a batch -- the loop of alignToOCR.py:160-182 over all lines at once, host
 * arithmetic: entry i of line b is (dec_t, dec_c)[dec_off[b] + i], i < dec_n[b]; its position x = (t - pad) * raw_w[b] /
 * (T[b] - 2 pad) goes through the `.llocs` text's one decimal ("%.1f") and int(np.round(x + x_min[b])) (half to even); a box
 * runs from the previous character's position (x_min[b] for the first) to its own, between y_min[b] and y_max[b]; classes
 * with cps[c] < 0 ('~' and '', alignToOCR.py:175) are dropped but still move the edge.  dec_len = entries in dec_t / dec_c (a
 * line whose dec_off + dec_n exceeds it is refused: TA_EINVAL).  Outputs have capacity sum(dec_n):
 * out_line, out_cp, out_boxes [k][4] = ulx, uly, lrx, lry; *out_count = characters kept.  All pointers [host]. */
/* Union of the OCR character boxes under every syllable of a batch of pages (alignToOCR.py:285-324 after the alignment;
 * host arithmetic).  ops: uint8 alignment columns of all pages end to end (0 pair, 1 transcript character over a gap, 2 gap
 * over an OCR character); idx[nidx]: row of boxes ([nboxes][4] = ulx, uly, lrx, lry) of the character of every OCR-carrying
 * column, in order; syllable s = transcript characters first_t[s] .. last_t[s] of the concatenated transcripts (ranges
 * disjoint, ascending).  out_low[s] = largest uly under the syllable (INT64_MIN: no OCR character under it -- the reference
 * skips it, :313-314); out_box[s][4] = union of the boxes whose uly is that value (the lower of two text lines, :318-320).
 * All pointers [host]. */
int ta_host_syllable_boxes(const uint8_t* ops, int64_t ncol, const int64_t* idx, int64_t nidx, const int64_t* boxes,
                           int64_t nboxes, const int64_t* first_t, const int64_t* last_t, int64_t nsyl,
                           int64_t* out_low, int64_t* out_box);
int ta_host_chars_of_batch(const int32_t* dec_t, const int32_t* dec_c, const int64_t* dec_n, const int64_t* dec_off,
                           const int64_t* T, const int64_t* raw_w, const int64_t* x_min, const int64_t* y_min,
                           const int64_t* y_max, const int64_t* cps, int32_t ncps, int32_t pad, int32_t nlines,
                           int64_t dec_len, int64_t* out_line, int64_t* out_cp, int64_t* out_boxes, int64_t* out_count);

/*
 * Affine-gap Needleman-Wunsch, replaces textSeqCompare.perform_alignment
 * (reference textSeqCompare.py:13-177; called from alignToOCR.py:273).
 *
 * ta_nw_workspace_bytes: bytes of pointer-matrix workspace one n x m problem needs
 * (1 byte per DP cell plus the skew padding of the strip layout -- 63 columns per strip, sized for the
 * finest strips TA_NW_ROWS can ask for -- plus one 8(m+2)-byte hand-off row per four strips for the wide
 * launch; multiple of 1024).
 */
int64_t ta_nw_workspace_bytes(int32_t n, int32_t m);

/* largest m (OCR-side length) the LDS-resident hand-off row supports */
int32_t ta_nw_max_m(void);

/*
 * ta_nw_batch: fill (textSeqCompare.py:53-88) and/or traceback (textSeqCompare.py:96-170)
 * of `nprob` independent problems.
 *
 *   t_codes, o_codes [dev]  concatenated int32 token ids of all transcripts / OCR strings;
 *                           equal ids <=> equal tokens (textSeqCompare.py:32); ids < 65536
 *   t_off, o_off     [dev]  int64[nprob+1] prefix offsets into the code arrays
 *   params           [dev]  int32 scoring systems, 6 per system: match, mismatch,
 *                           gap_open_x, gap_open_y, gap_extend_x, gap_extend_y
 *                           (textSeqCompare.py:30-34); params_stride = 0 -> one shared
 *                           system, 6 -> one per problem (the parameter grid of
 *                           evaluate_text_alignment.py:181-198)
 *   ws               [dev]  pointer-matrix workspace; ws_off [dev] int64[nprob] byte offset of
 *                           each problem's region (16-byte aligned, ta_nw_workspace_bytes long)
 *   ops_out          [dev]  alignment columns; problem p owns ops_off[p] .. ops_off[p] + n_p + m_p
 *                           and its alignment is RIGHT-aligned in that region: the last
 *                           ops_len[p] bytes, forward order, 0 = (t,o) pair, 1 = (t,'_'),
 *                           2 = ('_',o)  (textSeqCompare.py:115-164 after the reversal at :167)
 *   ops_off          [dev]  int64[nprob]
 *   ops_len          [dev]  int32[nprob] alignment lengths (written by the traceback; ta_nw2_batch sets them to -1
 *                           first, and a problem whose length is still negative afterwards was not walked)
 *   max_n, max_m            host-side maxima of the problem sizes (sizes LDS and the grid)
 *   score_bound             host-side bound on (max_n + max_m + 2) * max|param| used for the
 *                           overflow check (TA_ERANGE if it does not fit 2^23)
 *   flags                   TA_NW_FILL | TA_NW_TRACEBACK
 */
int ta_nw_batch(const int32_t* t_codes, const int64_t* t_off,
                const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                const int32_t* params, int32_t params_stride,
                uint8_t* ws, const int64_t* ws_off,
                uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                int32_t max_n, int32_t max_m, int64_t score_bound,
                uint32_t flags, void* stream);

/*
 * ta_nw2_batch: the same aligner in two phases -- a score-only wavefront fill that leaves
 * checkpoints, then a traceback that re-derives pointers only in windows around the path
 * (csrc/ta_nw2.hip).  Arguments and results exactly as ta_nw_batch, except that `ws` regions are
 * ta_nw2_workspace_bytes(n, m) long (lane-state checkpoints every 16 groups + the bottom rows of every
 * half-strip of 128 rows: ~0.3 B per cell instead of the 1 B/cell pointer matrix).  TA_NW_FILL = phase 1,
 * TA_NW_TRACEBACK = phase 2.
 */
int64_t ta_nw2_workspace_bytes(int32_t n, int32_t m);
/* widest OCR string ta_nw2_batch takes (its LDS holds the OCR codes only; the hand-off rows between
 * strips live in the workspace) */
int32_t ta_nw2_max_m(void);
int ta_nw2_batch(const int32_t* t_codes, const int64_t* t_off,
                 const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                 const int32_t* params, int32_t params_stride,
                 uint8_t* ws, const int64_t* ws_off,
                 uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                 int32_t max_n, int32_t max_m, int64_t score_bound,
                 uint32_t flags, void* stream);

/*
 * Banded phase 1 (csrc/ta_nw2.hip).  ta_nw2_batch_band is ta_nw2_batch with a band of half-width
 * band_w around the diagonal: the fill runs only the groups of every strip that hold cells with
 * min(0, m - n) - band_w <= j - i <= max(0, m - n) + band_w (plus a margin for the traceback's chunks), compares the
 * banded score of the walk's start with band_u[p] -- ta_nw2_band_bound(n_p, m_p, system of p, band_w), above which no
 * alignment that leaves the band can score -- and fills every problem that does not clear it again in full, in the same
 * call, before the traceback: results are ta_nw2_batch's, bit for bit.  band_w = 0: ta_nw2_batch itself (band_u, band_ok
 * unused); otherwise band_w >= 2, as ta_nw2_band_plan gave it for this batch and these flags.
 *   band_u  [dev]  int32[nprob]      the bounds (ta_nw2_band_plan's u_out)
 *   band_ok [dev]  int32[nprob]      written by the fill: 1 = the problem's band was certified, 0 = it was filled again in
 *                                    full (fail-closed: the fill zeroes the words, and only a passed comparison sets one)
 */
int ta_nw2_batch_band(const int32_t* t_codes, const int64_t* t_off,
                      const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                      const int32_t* params, int32_t params_stride,
                      uint8_t* ws, const int64_t* ws_off,
                      uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                      int32_t max_n, int32_t max_m, int64_t score_bound,
                      uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok, void* stream);
/*
 * The funnel (csrc/nw_band.h).  ta_nw2_batch_funnel is ta_nw2_batch_band with a region that narrows towards the table's
 * last cell inside the band of half-width band_w, certified at its own border: the fill leaves three words per problem
 * -- v0, the banded score of the walk's start; the exit maximum, above which no alignment that leaves the region can
 * score (banded value of the cell it leaves from + a static bound on the rest); the strips that contributed -- and a
 * small kernel between the fill and the fallback launch sets band_ok[p] iff the count is complete, v0 > band_u[p] and
 * v0 > the exit maximum.  Results are ta_nw2_batch's, bit for bit.
 *   band_x0   [dev]  int32[nprob]      host part of the exit maxima (ta_nw2_funnel_plan's x0_out)
 *   band_cert [dev]  int32[4 nprob]    per problem: v0, exit maximum, strips counted (written by the fill), and 1 if the
 *                                      funnel's own ranges ran, 0 if the band's (set before the fill)
 * Both NULL: ta_nw2_batch_band itself.
 */
int ta_nw2_batch_funnel(const int32_t* t_codes, const int64_t* t_off,
                        const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                        const int32_t* params, int32_t params_stride,
                        uint8_t* ws, const int64_t* ws_off,
                        uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                        int32_t max_n, int32_t max_m, int64_t score_bound,
                        uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok,
                        const int32_t* band_x0, int32_t* band_cert, void* stream);
/* The funnel inside the band of half-width w >= 2 for every problem of a batch (all pointers [host], any may be NULL
 * but the sizes and params): x0_out[nprob] = band_x0; for problem `big`, ranges_out[2 * strips] (ranges_cap = its
 * length) = first group and end group of every strip, out[0] = 1 if the funnel's own ranges run (0: declined for this
 * shape and system -- the band's ranges run, under the same certificate), out[1] = groups run, in 1/1000 of all. */
int ta_nw2_funnel_plan(const int32_t* n_arr, const int32_t* m_arr, int32_t nprob, const int32_t* params,
                       int32_t params_stride, int32_t w, int32_t big, int32_t* x0_out, int32_t* ranges_out,
                       int32_t ranges_cap, int32_t* out);
/*
 * The LCS-bounded funnel (csrc/nw_band.h).  ta_nw2_batch_funnel_lcs is ta_nw2_batch_funnel with the remainder of an
 * alignment that leaves the region bounded by the suffix LCS of the two strings, which a kernel of its own works out
 * before the fill (nw_lcs_suffix_kernel), and with the funnel's widths narrowed accordingly
 * (ta_nw2_funnel_lcs_scale_pm, per mille of the static funnel's).  It covers the problems of a batch that carries the
 * TA_NW_ALPHABET hint (alphabet <= 64), have at most ta_nw2_funnel_lcs_max_m() columns and match > mismatch; every
 * other problem of the batch runs ta_nw2_batch_funnel's region and bound in the same call.
 *   lcs [dev] int32[ta_nw2_funnel_lcs_words(nprob, max_n)]   the kernel's table (scratch); NULL: ta_nw2_batch_funnel
 * band_cert's fourth word is 2 for the problems covered.  band_x0 as for ta_nw2_batch_funnel (the covered problems'
 * boundary part is worked out on the device).
 */
int ta_nw2_batch_funnel_lcs(const int32_t* t_codes, const int64_t* t_off,
                            const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                            const int32_t* params, int32_t params_stride,
                            uint8_t* ws, const int64_t* ws_off,
                            uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                            int32_t max_n, int32_t max_m, int64_t score_bound,
                            uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok,
                            const int32_t* band_x0, int32_t* band_cert, int32_t* lcs, void* stream);
int64_t ta_nw2_funnel_lcs_words(int32_t nprob, int32_t max_n);
int32_t ta_nw2_funnel_lcs_scale_pm(void);
int32_t ta_nw2_funnel_lcs_max_m(void);
/* The ranges of problem (n, m) under params[6] inside the band of half-width w with the funnel's widths at scale_pm
 * per mille (1000: ta_nw2_funnel_plan's; otherwise ta_nw2_funnel_lcs_scale_pm()): ranges_out[2 * strips], out[0] = 1 if the funnel's own ranges run at this
 * scale, out[1] = groups run in 1/1000 of all.  Pure host function. */
int ta_nw2_funnel_ranges(int32_t n, int32_t m, const int32_t* params, int32_t w, int32_t scale_pm,
                         int32_t* ranges_out, int32_t ranges_cap, int32_t* out);
/* Suf bounded by the suffix LCS: the remainder with at most l matches among its diagonal steps (funnel_suf_lcs of
 * csrc/nw_band.h; never above ta_nw2_funnel_suf).  Pure host function. */
int32_t ta_nw2_funnel_suf_lcs(int32_t rn, int32_t rm, int32_t l, const int32_t* params);
/* The funnel's static bound on what is left of an alignment with rn rows and rm columns to go, in any state (Suf of
 * csrc/nw_band.h); ap_out (or NULL) = the best score of a single step.  Pure host function. */
int32_t ta_nw2_funnel_suf(int32_t rn, int32_t rm, const int32_t* params, int32_t* ap_out);
/* U(w): no alignment of an n x m problem under params[6] that visits a cell outside the band of half-width w scores
 * more than this.  Pure host function. */
int32_t ta_nw2_band_bound(int32_t n, int32_t m, const int32_t* params, int32_t w);
/* The band of a batch, from its sizes and scoring systems alone (all pointers [host]; params as ta_nw_batch's, on the
 * host).  band: 0 = the library's rule (smallest w with U(w) < 1/2 max(match, mismatch) min(n, m), the widest over the
 * batch; declined -- today's full fill -- when no w qualifies, the tallest problem has fewer than 1024 rows, the band
 * would run 0.8 or more of the groups of the largest problem (by cells: the one that weighs most in the batch's time), or phase 1 would not run the score profile with 4 or 8 waves),
 * 1 = off, otherwise the width itself (tests, tuning).  out[0] = band_w for ta_nw2_batch_band (0: no band), out[1] = the
 * rule's width (-1: none), out[2] = groups the band runs of the largest problem, in 1/1000 of all, out[3] = strips of
 * that problem, out[4] = its index, out[5] = 1 if the band runs as a funnel (band = 0 only: ta_nw2_batch_funnel with
 * ta_nw2_funnel_plan's x0_out for out[0]; out[2] and ranges_out are then the funnel's); u_out[nprob] (or NULL) = band_u; ranges_out[2 * out[3]] (or NULL; ranges_cap =
 * its length) = first group and end group of every strip of the largest problem. */
int ta_nw2_band_plan(const int32_t* n_arr, const int32_t* m_arr, int32_t nprob, const int32_t* params,
                     int32_t params_stride, uint32_t flags, int32_t band, int32_t* out, int32_t* u_out,
                     int32_t* ranges_out, int32_t ranges_cap);

/* What phase 2 (the traceback) of ta_nw2_batch launches for a batch of nprob problems: 1, 2 or 4 = waves per problem
 * (nw_trace2_kernel / nw_trace2w_kernel), 3 = two problems per wave on half-strips (nw_trace2h_kernel: batches that
 * fill the chip and share one scoring system), 5 / 6 = two / four waves per pair of problems on half-strips
 * (nw_trace2hw_kernel: medium batches under one scoring system).  Pure host function. */
int32_t ta_nw2_traceback_plan(int32_t nprob, int32_t params_stride, uint32_t flags);
/* What phase 1 of ta_nw2_batch would launch for a batch whose tallest / widest problem is
 * max_n x max_m under `flags` (the hints above): out[0] = 1 compare-select cell, 2 score profile
 * in LDS; out[1] = waves per workgroup; out[2] = dynamic LDS bytes per workgroup; out[3] = 1 if the
 * single-gap-open form of the cell is used.  For a batch large enough to fill the chip (the launch
 * also weighs the number of problems when it picks out[1]).  Pure host function (no GPU call). */
int ta_nw2_phase1_plan(int32_t max_n, int32_t max_m, uint32_t flags, int32_t* out);
/* the same for a batch of nprob problems: exactly what ta_nw2_batch will launch */
int ta_nw2_phase1_plan_batch(int32_t max_n, int32_t max_m, int32_t nprob, uint32_t flags, int32_t* out);

/*
 * ta_nw_general: the same aligner for scoring systems the integer kernel does not take --
 * a caller-supplied scoring function (textSeqCompare.py:27-29; the host tabulates it over
 * the distinct tokens into `table`, row-major [t id][o id], row length tm) or non-integral
 * numbers.  IEEE float64 throughout, bit-identical to the reference.  One problem per call.
 *
 *   t, o      [dev]  int32 token ids, n and m of them
 *   params    [dev]  6 doubles: match, mismatch, gap_open_x, gap_open_y, gap_extend_x, gap_extend_y
 *   table     [dev]  optional (NULL = use match/mismatch)
 *   score_ws  [dev]  ta_nw_general_score_bytes(n) bytes
 *   ptr_ws    [dev]  ta_nw_general_ptr_bytes(n, m) bytes
 *   ops_out   [dev]  n + m bytes, alignment right-aligned as in ta_nw_batch; ops_len [dev] int32
 */
int64_t ta_nw_general_score_bytes(int32_t n);
int64_t ta_nw_general_ptr_bytes(int32_t n, int32_t m);
int ta_nw_general(const int32_t* t, int32_t n, const int32_t* o, int32_t m,
                  const double* params, const double* table, int32_t tm,
                  double* score_ws, uint8_t* ptr_ws,
                  uint8_t* ops_out, int32_t* ops_len, void* stream);
/* The same for many problems in one launch (one workgroup each), match/mismatch scoring only:
 * concatenated codes with offsets as in ta_nw_batch; params = double[nprob or 1][6] with
 * params_stride 6 or 0; score_off (in doubles) / ptr_off / ops_off (in bytes) = per-problem offsets
 * into the workspaces (sizes as above) and into ops_out (capacity n + m, right-aligned). */
int ta_nw_general_batch(const int32_t* t_codes, const int64_t* t_off,
                        const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                        const double* params, int32_t params_stride,
                        double* score_ws, const int64_t* score_off,
                        uint8_t* ptr_ws, const int64_t* ptr_off,
                        uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len, void* stream);

/*
 * ta_nw_span_batch: WHERE in a longer transcript a page's text lies, before it is aligned (csrc/ta_nw_span.hip; DESIGN.md
 * section 4.6, the definition of record; checker tests/span_ref.py).  The reference's aligner is global -- "a transcript
 * of text that lies entirely within that manuscript" (textSeqCompare.py:13-20) -- so a transcript that runs over the page's
 * ends is smeared over the page.  This call fills the same affine-gap table (interior recurrence textSeqCompare.py:62-88,
 * row-0 boundary :57-60) with a FREE column 0 (M = Y = 0 there, where the reference has -i), carries with every value the
 * row at which it left column 0, and returns per problem int32 out[p][3] = (i0, i1, score): score = the maximum of the
 * last column, i1 = the smallest row that has it, i0 = the origin of that value (at equal score the larger origin, i.e.
 * the shorter span).  transcript[i0:i1] is then what ta_nw_batch / ta_nw2_batch is given.  Score only, no pointers.
 *
 *   t_codes          [dev]  int32 token ids; problem p's transcript is t_codes[t_start[p] .. t_start[p] + t_len[p]) --
 *                           NOT prefix offsets: many problems (the pages of a book) may name the same range
 *   t_start, t_len   [dev]  int64[nprob], int32[nprob]
 *   o_codes, o_off   [dev]  concatenated OCR ids and int64[nprob+1] prefix offsets, as in ta_nw_batch; ids < 65535
 *   params, params_stride   as in ta_nw_batch; gap opens of either sign
 *   out              [dev]  int32[nprob][3]; m = 0 gives (0, 0, 0), n = 0 gives (0, 0, -m)
 *   max_n, max_m            host-side maxima of t_len and of the OCR lengths
 *   score_bound             as in ta_nw_batch (TA_ERANGE if it does not fit 2^23: scores travel in a 24-bit field)
 *   max_param               host-side max |parameter| (TA_ERANGE above 2^19); a problem whose device parameters break
 *                           it anyway is refused by the kernel: out = (-1, -1, INT32_MIN)
 *   workspace               ta_nw_span_workspace_bytes(nprob, max_n, max_m) bytes [dev] -- 0 today (the rows handed from
 *                           strip to strip live in LDS; NULL is fine), TA_EINVAL for sizes the call would refuse
 * Limits, all TA_EINVAL before anything is launched: max_m <= ta_nw_span_max_m() (the LDS hand-off row, 16 bytes per OCR
 * token), max_n < 2^28 (the origin field).  One launch, one workgroup per problem; nothing waits.
 */
int32_t ta_nw_span_max_m(void);
int64_t ta_nw_span_workspace_bytes(int32_t nprob, int32_t max_n, int32_t max_m);
int ta_nw_span_batch(const int32_t* t_codes, const int64_t* t_start, const int32_t* t_len,
                     const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                     const int32_t* params, int32_t params_stride, int32_t* out,
                     int32_t max_n, int32_t max_m, int64_t score_bound, int32_t max_param,
                     void* workspace, int64_t workspace_bytes, void* stream);

/*
 * ta_nw_span_chain: the pages of a book IN READING ORDER in one transcript (csrc/ta_nw_span.hip; DESIGN.md section 4.6.1,
 * the definition of record; checker tests/span_chain_ref.py).  ta_nw_span_batch searches every page on its own, so a
 * passage the book repeats goes to its first copy; here chain c is one transcript and its pages
 * page_first[c] .. page_first[c+1], and page p's fill is ta_nw_span_batch's with a carry G'_{p-1}(i) where that has
 * the free 0 on column 0 and on row 0 (G'(0) - j).  F_p(i) = the last column's value of row i, G'_p(i) =
 * max(max_{j<=i} F_p(j) - max F_p, -floor), G'_{-1} = 0.  The walk back from limit = n, last page first: i1 = the smallest
 * row <= limit with the largest F_p up to limit, i0 = its origin, score = F_p(i1) - G'_{p-1}(i0), limit = i0.  Per page
 * int32 out[page][3] = (i0, i1, score) with i1 of a page <= i0 of the next; per chain int64 total = the sum of its scores.
 *
 *   t_codes, t_start, t_len [dev]  as in ta_nw_span_batch, one transcript per CHAIN: [nchains]
 *   o_codes, o_off          [dev]  the pages' OCR ids, concatenated, and int64[npages+1] prefix offsets; ids < 65535
 *   page_first              [dev]  int32[nchains+1], page_first[0] = 0, page_first[nchains] = npages
 *   host_pages              [HOST] int32[nchains], the chains' page counts: what the launches are sized with
 *   params, params_stride          as in ta_nw_batch, one row per CHAIN (or one for all); gap opens of either sign
 *   floor                          > 0: the clamp of the carry (it belongs to the rule; callers pass score_bound)
 *   out, total              [dev]  int32[npages][3], int64[nchains]
 *   max_n, max_m, score_bound, max_param   as in ta_nw_span_batch; TA_ERANGE unless score_bound + floor < 2^23
 *   workspace               [dev]  ta_nw_span_chain_workspace_bytes(nchains, npages, max_n) bytes, 16-byte aligned: per
 *                                  page the last column, its origins and the carry (12 bytes per transcript token)
 * Limits and refusals are ta_nw_span_batch's (TA_EINVAL / TA_ERANGE before anything is launched, nothing touched), and
 * TA_EINVAL for floor <= 0, a workspace too small and host_pages that do not add up to npages.  A chain whose device-side
 * sizes or parameters break the limits is refused as a whole by the kernels: (-1, -1, INT32_MIN) on each of its pages and
 * total = INT64_MIN.  Launches: one that ranks the chains by page count, then per step s the fill and the carry of page s
 * of every chain that has one, then one walk back -- all on `stream`, whose order is the only dependency; nothing
 * waits on the host or between workgroups, nothing is allocated.
 */
int64_t ta_nw_span_chain_workspace_bytes(int32_t nchains, int32_t npages, int32_t max_n);
int ta_nw_span_chain(const int32_t* t_codes, const int64_t* t_start, const int32_t* t_len,
                     const int32_t* o_codes, const int64_t* o_off, const int32_t* page_first,
                     int32_t nchains, int32_t npages, const int32_t* host_pages,
                     const int32_t* params, int32_t params_stride, int32_t floor,
                     int32_t* out, int64_t* total,
                     int32_t max_n, int32_t max_m, int64_t score_bound, int32_t max_param,
                     void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Line recogniser: replaces the `ocropus-rpred` subprocess of
 * alignToOCR.perform_ocr_with_ocropus (reference alignToOCR.py:142-147; arithmetic of the
 * third-party ocropy 1.3.3).  All pointers [dev].
 *
 * Lines are concatenated row-wise: line b owns rows row_off[b] .. row_off[b] + T[b] of
 *   x     [rows][48]   prepared line (ink = 1, 16 zero columns of padding each side)
 *   hout  [rows][200]  BiLSTM outputs [forward 100 | reversed LSTM flipped back 100]
 *   probs [rows][no]   softmax outputs;  logits [rows][no] optional (NULL to skip)
 *
 * ta_lstm_forward: group_lines = int32[ngroups][16] line ids (-1 = empty slot; [ngroups][4] in mode 2); one
 *   workgroup runs the lines of a group in lockstep, so groups should hold lines of similar length.
 *   mode 0: exact f32 MFMA chain.  wp = ta_lstm_packed_weight_floats(0) floats: B fragments
 *          [dir 2][wave 7][gate GI,GF,GO,CI][k-step 38][lane 64] =
 *          W_gate[unit 16*wave + lane%16][kp 4*kstep + lane/16], kp: 0 bias, 1..48 x,
 *          49..51 zero, 52..151 h; units >= 100 zero.
 *   mode 1: 16-bit matrix cores on split operands, f32 accumulation: W = W_hi (bf16) + W_r (fp16 of
 *          W - W_hi), activations three bf16 terms + one fp16; W.a ~ W_hi.(a_lo + a_mid + a_hi) + W_r.a16.
 *          wp = ta_lstm_packed_weight_floats(1) 4-byte units holding 16-bit patterns
 *          [dir 2][wave 7][plane hi,r][gate 4][k-step 5][lane 64][8] =
 *          plane of W_gate[unit 16*wave + lane%16][kp 32*kstep + 8*(lane/16) + j], kp as above
 *          padded with zeros to 160.
 *   mode 2: mode 0's arithmetic, bit for bit, on groups of FOUR lines (group_lines = int32[ngroups][4]):
 *          v_mfma_f32_4x4x1_16B_f32, one k per instruction -- a step costs a quarter of mode 0's, for the
 *          batches (a page, a few hundred lines) whose time is their longest line's.  wp =
 *          ta_lstm_packed_weight_floats(2) floats [dir 2][wave 7][k 152][lane 64] =
 *          W_gate(lane % 4)[unit 16*wave + lane/4][kp k], kp and padding as in mode 0.
 *   peep = float[2][3][112]: WIP, WFP, WOP per direction, units >= 100 zero.
 *   h0, c0, tstart (all NULL for fresh lines, or all given): a "line" may be the continuation of a
 *          sequence run elsewhere -- float h0[lines][2][100] / c0[lines][2][100] are the LSTM output
 *          and cell state before its first step, per direction (index 1 = the reversed LSTM, whose
 *          first step is the line's LAST row), and int32 tstart[lines][2] the number of steps of the
 *          sequence already done (> 0: the peepholes that ocropy skips at t = 0 apply from the start).
 * ta_lstm_output: w2p = float[201][16*ceil(no/16)] (classes beyond `no` zero): row 0 = bias
 *   column W2[:, 0]; row 1 + 4*kk + kq = W2[:, 1 + 50*kq + kk] (kk < 50, kq < 4) -- the k order
 *   in which the kernel consumes a row of hout.  no <= 128.  probs / logits / summary are each
 *   optional (at least one of probs, summary): summary = float[rows][4] =
 *   {P(class 0), best P, best class (integer bits), 0}, all the decoder needs.
 * ta_lstm_output_split: the same layer on the 16-bit matrix cores with split operands (the output
 *   stage of mode 1 above; products exact to ~2^-19 relative): w2s = ta_lstm_output_split_weight_bytes(no)
 *   bytes of 16-bit patterns [plane hi,r][class tile ceil(no/16)][k-step 7][lane 64][8] =
 *   plane of W2[16*tile + lane%16][1 + 32*kstep + 4*(lane/16) + 16*(j/4) + j%4] (inputs >= 200 and classes >= no
 *   zero), W2 = bf16 hi + fp16 rest as for the recurrence; bias = float[16*ceil(no/16)] = W2[:, 0].
 * ta_decode / ta_decode_summary: translate_back(outputs, threshold) per line, from the full
 *   probabilities or from the summaries; line b writes dec_n[b] (t, class) pairs at
 *   dec_t/dec_c + dec_off[b] (capacity (T[b] + 1) / 2 entries).
 */
int32_t ta_lstm_packed_weight_floats(int32_t mode);
int ta_lstm_forward(const float* x, const int64_t* row_off, const int32_t* T,
                    const int32_t* group_lines, int32_t ngroups,
                    const float* wp, const float* peep, float* hout, int32_t mode,
                    const float* h0, const float* c0, const int32_t* tstart, void* stream);
/*
 * The recurrence in FLOAT64 (csrc/ta_lstm_f64.hip) -- the arithmetic type of the reference's recogniser (ocropy
 * computes in float64 numpy; call site alignToOCR.py:142-147).  Two calls per run of groups:
 *
 * ta_lstm_xproj_f64: the input projection of every row at once, gx[dir][r][16 (unit / 4) + 8 (gate / 2) + 2 (unit % 4) + gate % 2] =
 *   W_gate[unit][0 .. 48] . [1; x[r]] in float64 for the `rows` rows at x; gx = ta_lstm_f64_gx_bytes(rows) bytes
 *   ([2][rows][400] doubles; the buffer is private to the pair of calls, its layout is the recurrence kernel's).  wx = ta_lstm_f64_weight_doubles(1) doubles [dir 2][tile 25][slot 13][lane 64]:
 *   slots 0..11 = W_gate(2 (i / 8) + i % 2)[unit 4 tile + (i % 8) / 2][1 + 4 slot + lane / 16], i = lane % 16 (the weights of
 *   x[4 slot + lane / 16]: B fragments of v_mfma_f64_16x16x4_f64, column i of a tile = its position in a row of gx);
 *   slot 12 = the column's bias W_gate(..)[unit ..][0] in every lane of the column (what the accumulators start from).
 * ta_lstm_forward_f64: the recurrence over `ngroups` groups of 16 lines (group_lines = int32[ngroups][16], -1 =
 *   empty slot) whose rows lie in [gx_row0, gx_row0 + gx_rows) -- row_off / hout use ABSOLUTE rows, gx holds the
 *   projection of rows gx_row0 .. only.  wh = ta_lstm_f64_weight_doubles(0) doubles
 *   [dir 2][wave 4][slot 7][k-step 25][lane 64] = W_gate(i / 4)[unit 4 tile + i % 4][49 + 4 kstep + lane / 16],
 *   tile = 6 wave + slot for slots 0..5 and 24 for slot 6 (the tile the waves split along k); peep = double[2][3][100]: WIP, WFP, WOP per direction.
 *   hout [rows][200] float (the float64 outputs rounded once).  h0 / c0 (double[lines][2][100]) / tstart as in
 *   ta_lstm_forward.  status (optional, [dev] one int32 the caller zeroes): the kernel ORs TA_LSTM_F64_PARTS_LATE into
 *   it if a workgroup's bounded wait for the partial sums of the tile its waves share ever runs out (the outputs of
 *   that group are NaN from there on); the launch itself still returns TA_OK -- read the word back with the results.
 * ta_lstm_forward_f64_g4: the same recurrence, bit for bit the same outputs, over groups of FOUR lines (group_lines =
 *   int32[ngroups][4]) on v_mfma_f64_4x4x4_4b_f64: a quarter of the cost per step, for batches whose 16-line groups
 *   would not fill the GPU or would wait for their longest line.  wh4 = ta_lstm_f64_weight_doubles(3) doubles
 *   [dir 2][tile 25][k-step 25][lane 64] = W_gate(lane % 4)[unit 4 tile + (lane / 4) % 4][49 + 4 kstep + lane / 16];
 *   every other argument as in ta_lstm_forward_f64.
 */
#define TA_LSTM_F64_PARTS_LATE 1
int64_t ta_lstm_f64_weight_doubles(int32_t which);
int64_t ta_lstm_f64_gx_bytes(int64_t rows);
int ta_lstm_xproj_f64(const float* x, int64_t rows, const double* wx, double* gx, void* stream);
int ta_lstm_forward_f64(const double* gx, int64_t gx_row0, int64_t gx_rows, const int64_t* row_off,
                        const int32_t* T, const int32_t* group_lines, int32_t ngroups, const double* wh,
                        const double* peep, float* hout, const double* h0, const double* c0,
                        const int32_t* tstart, int32_t* status, void* stream);
int ta_lstm_forward_f64_g4(const double* gx, int64_t gx_row0, int64_t gx_rows, const int64_t* row_off,
                           const int32_t* T, const int32_t* group_lines, int32_t ngroups, const double* wh4,
                           const double* peep, float* hout, const double* h0, const double* c0,
                           const int32_t* tstart, int32_t* status, void* stream);
int ta_lstm_output(const float* y, int64_t rows, const float* w2p, int32_t no,
                   float* probs, float* logits, float* summary, void* stream);
int64_t ta_lstm_output_split_weight_bytes(int32_t no);
int ta_lstm_output_split(const float* y, int64_t rows, const void* w2s, const float* bias, int32_t no,
                         float* probs, float* logits, float* summary, void* stream);
int ta_decode_summary(const float* summary, const int64_t* row_off, const int32_t* T,
                      int32_t nlines, float threshold,
                      int32_t* dec_t, int32_t* dec_c, int32_t* dec_n, const int64_t* dec_off,
                      void* stream);
int ta_decode(const float* probs, const int64_t* row_off, const int32_t* T,
              int32_t nlines, int32_t no, float threshold,
              int32_t* dec_t, int32_t* dec_c, int32_t* dec_n, const int64_t* dec_off,
              void* stream);

/*
 * ta_rows_gather: prepared rows that already lie in device memory into the recogniser's row layout -- line b's T[b]
 *   rows of 48 floats are copied from the device ADDRESS src[b] (16-byte aligned; any allocation, e.g. the device copy
 *   of a page-locked block of rows that ONE transfer brought over as it was) to rows dst_row[b] .. of x.  max_T >= every
 *   T[b].  All pointers [dev].  It stands where the reference writes each strip to a PNG file for the recogniser
 *   (alignToOCR.py:131-132): the hand-over of a batch's line images, without a host-side copy per line.
 */
int ta_rows_gather(const int64_t* src, const int64_t* dst_row, const int32_t* T, int32_t nlines,
                   int32_t max_T, float* x, void* stream);

/*
 * Line normaliser: what `ocropus-rpred` does to each PNG strip of alignToOCR.py:131-147 before the
 * network sees it -- ocropy 1.3.3 CenterNormalizer.measure / dewarp / normalize and prepare_line
 * (third-party arithmetic).  All pointers [dev].
 *
 * Strips are uint8 greyscale images (white background), concatenated: strip b = pix + pix_off[b],
 * hh[b] rows of ww[b] pixels.  gw holds the gaussian kernels; gw_off[b][3] are the offsets of the
 * CENTRE taps and gr[b][3] the radii of the three kernels of strip b (sigma 0.5 h along rows,
 * 1.0 h along columns, 0.3 h for the centre line; scipy's truncate = 4 kernels, computed by the
 * caller so that they are bit-identical to the host's).  ws: 3 * hh * ww doubles per strip at
 * ws_off[b]; arg / center: ww[b] ints per strip at col_off[b]; minmax: 2 ints per strip.
 *
 * ta_linenorm_measure writes center (the smoothed, truncated centre line), r_out (half-height of
 * the band cut around it) and wout (normalised width int(48 / (2 r) * w)) -- the caller reads wout
 * back to size the outputs.  ta_linenorm_resample writes the recogniser's input rows: strip b owns
 * rows row_off[b] .. row_off[b] + wout[b] + 32 of x [rows][48] (16 zero rows of padding each
 * side); tmp: 48 * wout[b] floats per strip at tmp_off[b]; omax: one word per strip.
 */
int ta_linenorm_measure(const uint8_t* pix, const int64_t* pix_off, const int32_t* hh,
                        const int32_t* ww, int32_t nlines, const double* gw,
                        const int64_t* gw_off, const int32_t* gr, double* ws,
                        const int64_t* ws_off, int32_t* arg, int32_t* center,
                        const int64_t* col_off, int32_t* minmax, int32_t* r_out,
                        int32_t* wout, void* stream);
int ta_linenorm_resample(const uint8_t* pix, const int64_t* pix_off, const int32_t* hh,
                         const int32_t* ww, int32_t nlines, const int32_t* center,
                         const int64_t* col_off, const int32_t* minmax, const int32_t* r,
                         const int32_t* wout, float* tmp, const int64_t* tmp_off,
                         uint32_t* omax, float* x, const int64_t* row_off, void* stream);

/*
 * Page preprocessing primitives: the full-page image passes of textAlignPreprocessing.py:160-285
 * (Gamera's to_onebit, despeckle, cc_analysis, rotation_angle_projections, rotate,
 * filter_short_runs / filter_narrow_runs, projection_rows in the reference).  One page at a time;
 * images are uint8 planes [h][w] (ink = 1).  All pointers [dev].
 *
 * ta_pp_label: 8-connected components; lab[p] = linear index of the component's first pixel in
 *   raster order, -1 on background; stats = int32[5][h*w] = area, x0, y0, x1, y1, indexed by that
 *   root (only the entries of roots are written; the others keep whatever the buffer held); flag = one device int (unused since round 3: tiles are stitched by one lock-free union-find
 *   pass, nothing iterates and nothing waits for the stream).
 * ta_pp_components: up to cap records {root, area, x0, y0, x1, y1} (any order), *count = true number.
 * ta_pp_filter_components: clears components with area < min_area or more than max_height rows.
 * ta_pp_angle_histograms: hist[a][row] of the page decimated by `step` and rotated by angle a
 *   (cos_sin = {cos a0, sin a0, ...}): pixel (y, x) lands on row rint(cy + dy cos a - dx sin a).
 * ta_pp_rotate: (bilinear resample of the 0/1 plane through output -> input map
 *   in = M out + offset, mo = {m00, m01, m10, m11, off0, off1}, zeros outside) > 0.5.
 * ta_pp_open_runs: morphological opening with a line of `len` pixels along `axis`.
 */
int ta_pp_histogram(const uint8_t* img, int64_t n, uint32_t* hist256, void* stream);
int ta_pp_threshold(const uint8_t* img, int64_t n, int32_t thr, int32_t invert, uint8_t* ink, void* stream);
int ta_pp_label(const uint8_t* ink, int32_t h, int32_t w, int32_t* lab, int32_t* stats, int32_t* flag,
                void* stream);
/* ta_pp_label for nimg images with shared waits: ink / lab / stats are [host] arrays of [dev] pointers,
 * h / w [host] arrays, flags nimg [dev] ints */
int ta_pp_label_batch(int32_t nimg, const uint8_t* const* ink, const int32_t* h, const int32_t* w,
                      int32_t* const* lab, int32_t* const* stats, int32_t* flags, void* stream);
int ta_pp_components(const int32_t* lab, const int32_t* stats, int32_t h, int32_t w, int32_t* recs,
                     int32_t cap, int32_t* count, void* stream);
int ta_pp_filter_components(uint8_t* ink, const int32_t* lab, const int32_t* stats, int32_t h, int32_t w,
                            int32_t min_area, int32_t max_height, void* stream);
int ta_pp_invert(uint8_t* ink, int64_t n, void* stream);
int ta_pp_angle_histograms(const uint8_t* ink, int32_t h, int32_t w, int32_t step, const double* cos_sin,
                           int32_t nang, uint32_t* hist, void* stream);
/* The skew search from a list of the page's ink pixels, made once for every angle of both sweeps:
 * ta_pp_ink_points: points[i] = (row << 16) | column on the grid decimated by `step` (room for
 * ceil(h/step) * ceil(w/step) entries; at most 65535 rows / columns), in no particular order; *count [dev].
 * ta_pp_angle_histograms_points(points, count, hs = ceil(h/step), ws = ceil(w/step), ...): the histograms of
 * ta_pp_angle_histograms, count for count. */
int ta_pp_ink_points(const uint8_t* ink, int32_t h, int32_t w, int32_t step, uint32_t* points, uint32_t* count,
                     void* stream);
int ta_pp_angle_histograms_points(const uint32_t* points, const uint32_t* count, int32_t hs, int32_t ws,
                                  const double* cos_sin, int32_t nang, uint32_t* hist, void* stream);
int ta_pp_rotate(const uint8_t* ink, int32_t h, int32_t w, uint8_t* out, int32_t oh, int32_t ow,
                 const double* mo, void* stream);
int ta_pp_open_runs(const uint8_t* in, uint8_t* out, int32_t h, int32_t w, int32_t len, int32_t axis,
                    void* stream);
int ta_pp_row_sums(const uint8_t* ink, int32_t h, int32_t w, int32_t* sums, void* stream);
int ta_pp_clear_rows(uint8_t* ink, int32_t w, const int32_t* rows, int32_t nrows, void* stream);
/* Host arithmetic, no device work: for the candidate rows idx[0..k) (local maxima) of a row projection
 * d[0..n), the arguments of the logarithms of calculate_peak_prominence (textAlignPreprocessing.py:59-110):
 * arg[c] = d[i] where d[i] == data_max, else d[i] - min(d[lo:hi]) + 1 over the reference's slice between i
 * and the nearest strictly higher sample.  All pointers [host]. */
int ta_pp_peak_prominence_args(const double* d, int32_t n, const int32_t* idx, int32_t k, double data_max,
                               double* arg);
/* The text-line strips of a page, cut from its ink plane (h x w, non-zero = ink) into one packed buffer as
 * the greyscale images the reference writes for the recogniser (alignToOCR.py:131-132; ink 0 on 255).
 * boxes (device): nstrips x {ulx, uly, lrx, lry, byte offset of the strip in out}, inclusive corners inside
 * the plane (the caller's to guarantee); strip s is row-major (lry - uly + 1) x (lrx - ulx + 1) at out + offset. */
int ta_pp_cut_strips(const uint8_t* ink, int32_t h, int32_t w, const int64_t* boxes, int32_t nstrips,
                     uint8_t* out, void* stream);

/*
 * Whole STAGES of the page preprocessing for a batch of n pages, one call each: everything between two of the
 * pipeline's data-dependent host decisions (Otsu threshold | skew sweeps | projection peaks | component selection |
 * strips) -- reference textAlignPreprocessing.py:160-285, where every page pass is a Gamera call.  A page's stage is a
 * dozen launches; made one by one from the host language they cost more host time than the kernels take.  Arguments
 * named like arrays are [host] arrays of n [dev] pointers / sizes; everything is enqueued on `stream`, nothing is
 * waited for; per page the kernels and their order are those of the single-page entry points above.
 *
 * The two stages that need connected components (ta_pp_binarise_batch, ta_pp_line_components_batch) find them over
 * RUNS since round 6 (a text page's ~6 M pixels are a few hundred thousand horizontal runs; a wave per row finds
 * them, one union-find pass joins each with the touching runs of the row above, 8-connectivity; a component's root is
 * its raster-first run): same components, areas, boxes and root pixels as ta_pp_label gives, a fifth of the memory
 * traffic; the holes are filled from the runs of PAPER, without inverting the plane and back.  lab[i] / stats[i] are
 * then scratch for the run tables (pages under 8 columns, or flags & TA_PP_LABEL_PIXELS: the per-pixel form).
 *
 * ta_pp_histogram_batch: hist [dev] = uint32[n][256] of img[i][0..npix[i]).
 * ta_pp_binarise_batch (:167-186): ink[i] = img[i] thresholded at thr[i], despeckled (components under `despeckle`
 *   pixels; ink, then background), components taller than max_height rows dropped; points[i] / counts[i] [dev uint32[n]]
 *   = ta_pp_ink_points of the page decimated by step[i].  lab[i] / stats[i]: h*w and 5*h*w int32 of scratch.
 * ta_pp_angle_histograms_points_batch: ta_pp_angle_histograms_points per page (cos_sin[i]: 2*nang[i] doubles [dev],
 *   hist[i]: uint32[nang[i]][hs[i]] [dev]).
 * ta_pp_deskew_batch (:187-195, :212-215): out[i] (oh[i] x ow[i]) = ink[i] rotated through mo[i] (ta_pp_rotate;
 *   mo[i] NULL: a copy, sizes equal); eroded[i] = out[i] opened with runs of runs_len pixels along the rows, then the
 *   columns, `rounds` times (runs_len <= 1: a copy; tmp[i]: oh*ow bytes of scratch); sums[i][r] = ink of eroded row r.
 * ta_pp_line_components_batch (:216-252): work[i] = eroded[i] with rows[i][0..nrows[i]) cleared, labelled (scratch as
 *   above); page i's component table (ta_pp_components) at recs [dev] + i*cap*6, its true count in counts[i] [dev].
 * ta_pp_cut_strips_batch: ta_pp_cut_strips per page into ONE packed buffer (the boxes carry their offsets).
 */
int ta_pp_histogram_batch(int32_t n, const uint8_t* const* img, const int64_t* npix, uint32_t* hist, void* stream);
#define TA_PP_LABEL_PIXELS 1   /* flags of the two stages that label: a label per PIXEL (ta_pp_label_batch) instead of
                                * connected components over RUNS -- the form of rounds 3-5, kept as the cross-check */
int ta_pp_binarise_batch(int32_t n, const uint8_t* const* img, const int32_t* h, const int32_t* w, const int32_t* thr,
                         int32_t despeckle, int32_t max_height, uint8_t* const* ink, int32_t* const* lab,
                         int32_t* const* stats, const int32_t* step, uint32_t* const* points, uint32_t* counts,
                         int32_t flags, void* stream);
int ta_pp_angle_histograms_points_batch(int32_t n, const uint32_t* const* points, const uint32_t* counts,
                                        const int32_t* hs, const int32_t* ws, const double* const* cos_sin,
                                        const int32_t* nang, uint32_t* const* hist, void* stream);
int ta_pp_deskew_batch(int32_t n, const uint8_t* const* ink, const int32_t* h, const int32_t* w,
                       const double* const* mo, uint8_t* const* out, const int32_t* oh, const int32_t* ow,
                       uint8_t* const* tmp, uint8_t* const* eroded, int32_t runs_len, int32_t rounds,
                       int32_t* const* sums, void* stream);
int ta_pp_line_components_batch(int32_t n, const uint8_t* const* eroded, const int32_t* h, const int32_t* w,
                                const int32_t* const* rows, const int32_t* nrows, uint8_t* const* work,
                                int32_t* const* lab, int32_t* const* stats, int32_t* recs, int32_t cap,
                                int32_t* counts, int32_t flags, void* stream);
int ta_pp_cut_strips_batch(int32_t n, const uint8_t* const* ink, const int32_t* h, const int32_t* w,
                           const int64_t* const* boxes, const int32_t* nstrips, uint8_t* packed, void* stream);

/*
 * Host arithmetic between the preprocessing stages ([host] pointers only, no device work): the per-page numpy passes
 * of the reference's Python between two Gamera calls, as plain loops that hold no interpreter lock; each reproduces
 * the numpy expression it replaces operation by operation (tests/test_preprocessing.py fuzzes them against numpy).
 * ta_host_otsu_batch: Otsu's threshold (first maximum of the between-class variance) of n 256-bin histograms.
 * ta_host_sharpest_rows: per page k the row of its nang[k] x hs[k] int32 histograms (at hist + off[k]) with the
 *   largest np.var (numpy's pairwise summation), and whether the page has a count at all; var_out may be NULL.
 * ta_host_line_boxes: per peak location the union of the components [ulx, uly, lrx, lry] that vertically coincide
 *   with the strip of half height `half` around it (textAlignPreprocessing.py:38-56, :253-276).
 */
/* The text-line peaks of a batch of pages in two calls with ONE numpy logarithm between them (numpy's float64 log is
 * its own routine on AVX-512 hosts and differs from libm's in the last bit now and then, and the prominences are
 * compared with a tolerance after a division: the logarithm stays numpy's).
 * ta_host_peak_candidates: page k's row projection proj + off[k] (len[k] int64 sums) -> smoothed + off[k]
 *   (moving_avg_filter, textAlignPreprocessing.py:147-157), its local maxima cand_idx + off[k] (cand_n[k] of them) and
 *   the ARGUMENT of each one's logarithm cand_arg + off[k] (calculate_peak_prominence :59-110).
 * ta_host_peak_select: with cand_log = log(cand_arg): peaks + off[k] (npeaks[k] rows whose prominence / the largest
 *   exceeds tol >= 0, find_peak_locations :113-144) and the white rows between neighbouring peaks rows + 2 off[k]
 *   (nrows[k], ascending; :222-232). */
int ta_host_peak_candidates(const int64_t* proj, const int64_t* off, const int32_t* len, int32_t n, int32_t filter_size,
                            double* smoothed, int32_t* cand_idx, double* cand_arg, int32_t* cand_n);
int ta_host_peak_select(const double* smoothed, const int64_t* off, const int32_t* len, int32_t n, const int32_t* cand_idx,
                        const double* cand_log, const int32_t* cand_n, double tol, int32_t* peaks, int32_t* npeaks,
                        int32_t* rows, int32_t* nrows);
int ta_host_otsu_batch(const int32_t* hist, int32_t n, int32_t* thr);
int ta_host_sharpest_rows(const int32_t* hist, const int64_t* off, const int32_t* nang, const int32_t* hs, int32_t n,
                          int32_t* best, uint8_t* any, double* var_out);
int ta_host_line_boxes(const int64_t* comps, int64_t ncomp, const int64_t* peaks, int64_t npeaks, int64_t half,
                       int64_t* out_boxes, uint8_t* out_hit);

/*
 * Alignment evaluation for a scoring-system sweep (csrc/ta_eval.hip; reference evaluate_text_alignment.py:16-131).
 * [device] pointers unless marked [host]; every call is enqueued on `stream`.
 * ta_eval_integral: inclusive int32 summed-area tables sat[i] (h[i] x w[i]) of the uint8 planes ink[i] (nonzero = ink).
 *   ink, h, w, sat are [host] arrays of n entries; a page over 2^31 - 1 pixels is TA_EINVAL.
 * ta_eval_syllable_boxes: per NW problem p (of a ta_nw_batch / ta_nw2_batch call: ops, ops_off, ops_len, t_off, o_off as
 *   that call had them) on page prob_page[p]: the union of the OCR boxes under each syllable on its lowest text line,
 *   un-rotated onto the raw page.  Page tables: char_box [.][4] (ulx, uly, lrx, lry of the expanded OCR characters,
 *   page k's at char_off[k]); syllable s of page k covers transcript characters syl_first[s] .. syl_last[s]
 *   (s in syl_off[k] .. syl_off[k + 1]); rot[6 k ..] = sin, cos (of -angle, host libm), px, py, px - dx, py - dy.
 *   Out: out_box [nprob][max_syl][4] int32, out_present [nprob][max_syl], status [nprob] (TA_EVAL_*).  max_cols bounds
 *   n + ops_len of every problem (LDS); above TA_EVAL_MAX_COLUMNS the call is TA_ELIMIT.
 * ta_eval_score: per problem p and counted gt box r of its page (gt [.][4], page k's at rep_off[k]): the first
 *   strict maximum of the intersection over the candidates cand[cand_off[r] .. cand_off[r + 1]] (syllable indices,
 *   ascending; absent boxes skipped), then IOU and black-area IOU on the page's table sat[k] (a [device] array of
 *   pointers, with sat_h / sat_w [device]).  Output r of problem p at out_off[p] + r: iou, area (float64), status;
 *   a problem whose boxes have a non-zero status passes it on.  max_rep: the largest gt box count of a page.
 */
#define TA_EVAL_OK 0
#define TA_EVAL_UNFINISHED 1       /* the problem's traceback did not finish (ops_len < 0) */
#define TA_EVAL_MISMATCH 2         /* alignment columns disagree with the page's tables */
#define TA_EVAL_OUT_OF_RANGE 3     /* a rectangle of the black-area IOU lies outside the ink plane */
#define TA_EVAL_ZERO_AREA 4        /* black-area IOU with a zero denominator */
#define TA_EVAL_MAX_COLUMNS 40960  /* n + alignment columns of one problem: 160 KiB of LDS */
int32_t ta_eval_max_columns(void);
int ta_eval_integral(int32_t n, const uint8_t* const* ink, const int32_t* h, const int32_t* w, int32_t* const* sat,
                     void* stream);
int ta_eval_syllable_boxes(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, const int64_t* t_off,
                           const int64_t* o_off, int32_t nprob, const int32_t* prob_page, const int32_t* char_box,
                           const int64_t* char_off, const int32_t* syl_first, const int32_t* syl_last,
                           const int64_t* syl_off, const double* rot, int32_t max_syl, int32_t max_cols,
                           int32_t* out_box, uint8_t* out_present, int32_t* status, void* stream);
int ta_eval_score(int32_t nprob, const int32_t* prob_page, const int32_t* boxes, const uint8_t* present,
                  const int32_t* box_status, int32_t max_syl, const int32_t* gt, const int64_t* rep_off,
                  const int64_t* cand_off, const int32_t* cand, const int32_t* const* sat, const int32_t* sat_h,
                  const int32_t* sat_w, const int64_t* out_off, int32_t max_rep, double* iou, double* area,
                  int32_t* status, void* stream);

/*
 * Training of the line recogniser in float64 (csrc/ta_train.hip; DESIGN.md section 14: ocropy 1.3.3's
 * SeqRecognizer.trainSequence restated, parity unpinned).  [device] pointers unless marked [host]; every call is
 * enqueued on `stream` and none synchronises the device.  A batch is `nlines` lines whose rows (timesteps) lie in
 * per-row arrays of `rows` rows: line b owns rows row_off[b] .. row_off[b] + T[b]; max_T bounds every T[b] and may not
 * exceed TA_TRAIN_MAX_T.  Weights: W [dir 2][gate 4: WGI, WGF, WGO, WCI][unit 100][149], peep [dir 2][WIP, WFP, WOP][100],
 * W2 [no][201], all as in SURVEY.md Appendix B.3 / B.4 (dir 1 = the reversed LSTM, which walks a line from its last row).
 * ta_lstm_train_forward: gx [rows][dir 2][400] holds W_gate[unit][0 .. 48] . [1; x[row]] (a matrix product, the
 *   caller's); the recurrence writes states [rows][dir 2][TA_TRAIN_STATE_FIELDS][100] = gi, gf, go, ci, c and the
 *   h the step STARTED from, hout [rows][200] and the softmax outputs probs [rows][no].
 * ta_lstm_train_backward: dy [rows][200] = d(-CE)/d hout; walks every line backwards through the saved states and
 *   writes the gate errors gate_err [rows][dir 2][gate 4][100] and the peephole gradients dpeep [nlines][dir 2][3][100]
 *   (the other weight gradients are matrix products of gate_err with the steps' inputs: the caller's).
 * ta_ctc_align: per line the target codes labels[lab_off[b] .. + L[b]] (0 < code < no); T_host / L_host are [host]
 *   copies of T / L: a target whose 2 L + 1 states exceed its line's timesteps, or TA_CTC_MAX_STATES, is TA_EINVAL
 *   before anything is launched.  workspace: the sum of ta_ctc_workspace_bytes(T, L, no) over the lines (-1 for sizes
 *   the call would refuse), line b's piece at ws_off[b] DOUBLES.  Writes aligned and deltas = aligned - probs
 *   ([rows][no]) and err [nlines] = the line's sum of deltas^2 (NaN: the kernel found the line's numbers out of bounds
 *   and left its rows alone).
 */
#define TA_TRAIN_NI 48
#define TA_TRAIN_NS 100
#define TA_TRAIN_STATE_FIELDS 6
#define TA_TRAIN_MAX_T 5000
#define TA_TRAIN_MAX_CLASSES 128
#define TA_CTC_MAX_STATES 2049     /* 2 L + 1 of one target: the lattice's running row lives in LDS */
int64_t ta_ctc_workspace_bytes(int32_t T, int32_t L, int32_t no);
int ta_ctc_align(const double* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                 const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines, int32_t no,
                 int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host, double* workspace,
                 int64_t workspace_bytes, double* aligned, double* deltas, double* err, void* stream);
int ta_lstm_train_forward(const double* gx, const int64_t* row_off, const int32_t* T, int32_t nlines, int32_t max_T,
                          int64_t rows, const double* W, const double* peep, const double* W2, int32_t no,
                          double* states, double* hout, double* probs, void* stream);
int ta_lstm_train_backward(const double* dy, const double* states, const int64_t* row_off, const int32_t* T,
                           int32_t nlines, int32_t max_T, int64_t rows, const double* W, const double* peep,
                           double* gate_err, double* dpeep, void* stream);

/*
 * Random elastic distortion of text-line strips, the training augmentation (csrc/ta_distort.hip; DESIGN.md section
 * 14.4).  pix / pix_off / hh / ww [device] as for ta_linenorm_measure; hh_host / ww_host are [host] copies: a strip
 * taller than TA_DISTORT_MAX_H, or a dsigma whose radius int(4 dsigma + 0.5) exceeds TA_DISTORT_MAX_RADIUS, is
 * TA_ELIMIT, a non-positive distort or dsigma TA_EINVAL, before anything is launched.  Strip b draws its noise from
 * Philox4x32-10 with key `seed` and counter words (pixel, 0, counters[b]); gw [device]: the 2 radius + 1 weights of
 * scipy's gaussian kernel of sigma dsigma (the caller's, so that they are bit-identical to the host's).  workspace:
 * ta_line_distort_workspace_bytes(nlines, sum of hh ww) bytes (-1 for negative arguments).  out: the distorted strips,
 * laid out as pix is.  fields: optional (may be null), the two scaled displacement fields of strip b -- rows, then
 * columns, hh ww doubles each -- at 2 pix_off[b] doubles; for tests.  One launch per kernel; nothing waits.
 */
#define TA_DISTORT_MAX_H 512
#define TA_DISTORT_MAX_RADIUS 2048
int64_t ta_line_distort_workspace_bytes(int32_t nlines, int64_t total_pixels);
int ta_line_distort(const uint8_t* pix, const int64_t* pix_off, const int32_t* hh, const int32_t* ww,
                    const uint64_t* counters, int32_t nlines, const int32_t* hh_host, const int32_t* ww_host,
                    double distort, double dsigma, uint64_t seed, const double* gw, void* workspace,
                    int64_t workspace_bytes, uint8_t* out, double* fields, void* stream);

/*
 * Held-out scoring of line models (csrc/ta_errs.hip; DESIGN.md section 14.5: what ocropus-errs / ocropus-econf report,
 * parity unpinned).  Line b's decoded class codes are dec_c[dec_off[b] .. + dec_n[b]] exactly as ta_decode /
 * ta_decode_summary left them ([device]; dec_len = the elements of dec_c): the kernel reads the lengths itself, the
 * host never learns them.  It drops class 0, treats class 1 (" ") by `kind` (TA_ERRS_KIND_EXACT: runs collapse to one,
 * none at either end; TA_ERRS_KIND_NOSPACE: all dropped), and compares what is left (n codes) with the line's target
 * targets[tgt_off[b] .. + tgt_n[b]] (m codes in 1 .. nclasses - 1, nclasses = No + 1: the code No stands for a
 * character outside the codec; tgt_len = the elements of targets) by unit-cost edit distance.  ONE alignment is walked
 * back from (n, m) -- among the minima of a cell: diagonal, then insertion (a decoded code the target lacks), then
 * deletion -- and every column of it adds one to conf[x][y] ([nclasses][nclasses] int64, x the decoded code, y the
 * target's, 0 = nothing; the caller zeroes it, calls accumulate).  per_line [nlines][TA_ERRS_FIELDS] = errors, n, m,
 * substitutions, insertions, deletions.  n_bound[b] >= dec_n[b] is the bound line b's workspace was sized for
 * ((T[b] + 1) / 2 for a line of T[b] timesteps); workspace: the sum of ta_errs_workspace_bytes(n_bound[b], tgt_n[b]),
 * line b's piece at ws_off[b] BYTES (a multiple of 16).  n_bound_host / tgt_n_host are [host] copies: a negative one
 * is TA_EINVAL, one over TA_ERRS_MAX_DECODED / TA_ERRS_MAX_TARGET TA_ELIMIT (ta_errs_workspace_bytes returns the same
 * codes), before anything is launched.  The kernel re-checks every bound on the device's numbers -- dec_n[b] against
 * n_bound[b], offsets against dec_len / tgt_len / workspace_bytes, every code against nclasses -- and a line that
 * fails gets errors = -1 (the other five fields 0) and adds nothing to conf.  One launch; nothing waits or allocates.
 */
#define TA_ERRS_FIELDS 6
#define TA_ERRS_KIND_EXACT 0
#define TA_ERRS_KIND_NOSPACE 1
#define TA_ERRS_MAX_TARGET 4096
#define TA_ERRS_MAX_DECODED 2500   /* (TA_TRAIN_MAX_T + 1) / 2: two decoded characters are a timestep apart */
int64_t ta_errs_workspace_bytes(int32_t n_max, int32_t m);
int ta_edit_distance(const int32_t* dec_c, const int64_t* dec_off, const int32_t* dec_n, int64_t dec_len,
                     const int32_t* targets, const int64_t* tgt_off, const int32_t* tgt_n, int64_t tgt_len,
                     const int32_t* n_bound, const int64_t* ws_off, int32_t nlines, int32_t nclasses, int32_t kind,
                     const int32_t* n_bound_host, const int32_t* tgt_n_host, void* workspace, int64_t workspace_bytes,
                     int32_t* per_line, int64_t* conf, void* stream);

/*
 * Harvesting of line-level training texts from aligned pages (csrc/ta_harvest.hip; DESIGN.md section 14.6, the rule of
 * record; checker tests/harvest_ref.py).  [device] pointers unless marked [host]; both calls are one launch on `stream`,
 * neither waits nor allocates.
 * ta_harvest_lines: per NW problem p = page (ops, ops_off, ops_len, t_codes, t_off, o_codes, o_off as the ta_nw_batch /
 *   ta_nw2_batch call had them; ops_bytes = the bytes of ops): o_line[o_off[p] + j] is the batch-wide text line of OCR
 *   character j (never decreasing along a page, inside line_first[p] .. line_first[p + 1]), t_class[t_off[p] + i] the
 *   recogniser's class of transcript character i (1 = space, below 1 = not in the codec), T [nlines] the lines'
 *   timesteps, num / den the minimum agreement.  Out: table [nlines][TA_HARVEST_FIELDS] int32 = reason (a set of
 *   TA_HARVEST_* bits, 0 = accepted), t_first, L (the kept characters are the page's transcript[t_first .. t_first + L)),
 *   equal pairs, unequal pairs, interior op-1 columns, op-2 columns, seam; status [nprob] (TA_HARVEST_OK ...).  A page
 *   whose device numbers fail the kernel's own checks -- ops_len < 0 or above n + m, offsets outside t_len / o_len /
 *   ops_bytes, a column code above 2, columns that do not carry n transcript and m OCR characters, an o_line that
 *   decreases or leaves the page's lines -- gets TA_HARVEST_PAGE (the other seven fields 0) on all of its lines and a
 *   non-zero status; a page whose line range itself lies outside 0 .. nlines gets the status alone.
 *   t_off_host / o_off_host / line_first_host are [host] copies, nprob + 1 entries: a decreasing one, a line_first that
 *   does not run from 0 to nlines, num / den outside 0 < num <= den <= TA_HARVEST_MAX_DEN, a workspace below
 *   ta_harvest_workspace_bytes(nlines, t_off_host[nprob], o_off_host[nprob]) or not 16-byte aligned are TA_EINVAL; a
 *   page over TA_HARVEST_MAX_COLUMNS transcript or OCR characters, or more than TA_HARVEST_MAX_LINES lines, TA_ELIMIT
 *   (ta_harvest_workspace_bytes returns the same codes) -- before anything is launched.
 * ta_harvest_pack: the accepted lines (reason 0) of `table`, ascending, in the layout ta_ctc_align reads: acc_line[k],
 *   L[k], lab_off[k] (the exclusive sum of L), labels = the t_class values of each line's range (label_cap elements:
 *   the batch's transcript characters suffice), count[2] = accepted lines, labels written.  `workspace` is the one
 *   ta_harvest_lines filled (it holds the lines' offsets into t_class).  Every row is re-checked (1 <= L <=
 *   TA_HARVEST_MAX_TARGET, its range inside t_len, the labels inside label_cap); if one fails count is {-1, -1} and the
 *   other outputs are not to be used.
 */
#define TA_HARVEST_FIELDS 8
#define TA_HARVEST_EMPTY 1         /* nothing is left after trimming the spaces at both ends */
#define TA_HARVEST_LOW 2           /* equal den < num (equal + unequal + interior op-1 + op-2), or that sum is 0 */
#define TA_HARVEST_SEAM 4          /* transcript characters other than spaces between this line and a neighbour */
#define TA_HARVEST_UNANCHORED 8    /* the first or last kept character is not in a pair of equal ids */
#define TA_HARVEST_CODEC 16        /* a kept character is not in the recogniser's codec */
#define TA_HARVEST_TOO_LONG 32     /* 2 L + 1 > T[line], or L > TA_HARVEST_MAX_TARGET */
#define TA_HARVEST_PAGE 64         /* the page was refused: see status */
#define TA_HARVEST_OK 0
#define TA_HARVEST_UNFINISHED 1    /* ops_len < 0: the traceback did not finish */
#define TA_HARVEST_MISMATCH 2      /* offsets, ops_len or the columns disagree with n and m */
#define TA_HARVEST_LINES 3         /* o_line decreases or leaves the page's lines, or the line range is out of bounds */
#define TA_HARVEST_MAX_TARGET 1024 /* (TA_CTC_MAX_STATES - 1) / 2 */
#define TA_HARVEST_MAX_COLUMNS (1 << 24)
#define TA_HARVEST_MAX_LINES (1 << 24)
#define TA_HARVEST_MAX_DEN 1000000
int64_t ta_harvest_workspace_bytes(int32_t nlines, int64_t t_len, int64_t o_len);
int ta_harvest_lines(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                     const int32_t* t_codes, const int64_t* t_off, const int32_t* o_codes, const int64_t* o_off,
                     int32_t nprob, const int32_t* o_line, const int64_t* line_first, const int32_t* t_class,
                     const int32_t* T, int32_t nlines, int32_t num, int32_t den, const int64_t* t_off_host,
                     const int64_t* o_off_host, const int64_t* line_first_host, void* workspace,
                     int64_t workspace_bytes, int32_t* table, int32_t* status, void* stream);
int ta_harvest_pack(const int32_t* table, const void* workspace, int64_t workspace_bytes, const int32_t* t_class,
                    int64_t t_len, int32_t nlines, int64_t label_cap, int32_t* acc_line, int32_t* L, int64_t* lab_off,
                    int32_t* labels, int64_t* count, void* stream);

/*
 * Forced alignment of a line's known text with the recogniser's class posteriors (csrc/ta_forced.hip; DESIGN.md section
 * 14.7, the rule of record; checker tests/forced_ref.py).  [device] pointers unless marked [host]; one launch on
 * `stream`, nothing waits or allocates.  The conventions are those of ta_ctc_align: line b owns the probability rows
 * row_off[b] .. + T[b] of probs (float32 [rows][no], what ta_lstm_output writes in every precision mode) and the labels
 * labels[lab_off[b] .. + L[b]] (1 <= code < no; 0 is the blank).  Every probability becomes an integer emission score q
 * (units of 2^-16 bit, floor 2^-17, no transcendental function), and the best path through the 2 L + 1 states blank, c0,
 * blank, c1 ... blank -- stay / advance / skip a blank between different characters, ties in that order, the last blank
 * before the last character at the end -- is walked back.  Out: frames [nlabels][TA_FORCED_FIELDS] int32, row
 * lab_off[b] + i = t_first, t_last (the timesteps the path spends in character i) and t_peak (the first of them with the
 * largest q of that character); score [nlines] int64, the path's total; status [nlines].
 * T_host / L_host are [host] copies of T / L: L < 1, T < 1, 2 L + 1 > T, timesteps or labels that sum to more than rows /
 * nlabels, no outside 2 .. TA_TRAIN_MAX_CLASSES, a null pointer, a negative size, a workspace below the sum of
 * ta_forced_workspace_bytes(T, L) or not 16-byte aligned are TA_EINVAL, L > TA_FORCED_MAX_TARGET or T > TA_TRAIN_MAX_T
 * TA_ELIMIT (ta_forced_workspace_bytes returns -1 for all of these) -- before anything is launched.  Line b's piece of
 * the workspace (its moves: two bits per state and timestep) lies at ws_off[b] BYTES, a multiple of 16.  The kernel
 * re-checks every bound on the device's numbers: a line whose T, L, offsets or workspace piece fail gets
 * TA_FORCED_BOUNDS, one with a label outside 1 .. no - 1 TA_FORCED_LABEL; neither touches its frames or its score.
 * The walk stages the moves through LDS in blocks of TA_FORCED_WALK_BLOCK timesteps.
 */
#define TA_FORCED_MAX_TARGET 1023  /* L; 2 L + 1 = 2047 states, 32 per lane */
#define TA_FORCED_FIELDS 3         /* t_first, t_last, t_peak */
#define TA_FORCED_WALK_BLOCK 32
#define TA_FORCED_OK 0
#define TA_FORCED_BOUNDS 1         /* the kernel found the line's own numbers out of bounds; its outputs are left alone */
#define TA_FORCED_LABEL 2          /* a label outside 1 .. no - 1 */
int64_t ta_forced_workspace_bytes(int32_t T, int32_t L);
int ta_forced_align(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                    const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines, int32_t no,
                    int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host, void* workspace,
                    int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status, void* stream);
/*
 * ta_forced_align_lines: the same alignment (the same kernel body) for a line list that lies on the device, as
 * ta_harvest_pack leaves it -- so a caller can enqueue it behind the harvest without a look at the table.  Packed slot
 * k < count[0] aligns the chunk's line q = acc_line[k]: its rows row_off_all[q] .. + T_all[q], its workspace piece at
 * ws_off_all[q], the labels labels[lab_off[k] .. + L[k]] (label_cap elements, as ta_harvest_pack's).  Out: frames
 * [label_cap][TA_FORCED_FIELDS] rows lab_off[k] + i, score [nslots] and status [nslots] PER SLOT.  nslots <= nlines_all is
 * the number of slots the launches cover; a slot at or behind count[0], and every slot of a call whose count[0] is
 * negative, writes nothing at all.
 * [host] T_all_host and Lcap_host per chunk line: Lcap is the caller's upper bound on the text line q can receive
 * (0: none; at most TA_FORCED_MAX_TARGET and (T - 1) / 2); Lcap [device] is its copy.  From these alone the host takes
 * the refusals (as ta_forced_align's: T < 1, a cap below 0, 2 Lcap + 1 > T, timesteps above rows, a workspace below the sum
 * of ta_forced_workspace_bytes(T, Lcap) over the lines with a cap or not 16-byte aligned, nslots > nlines_all are
 * TA_EINVAL; a cap above TA_FORCED_MAX_TARGET or T above TA_TRAIN_MAX_T TA_ELIMIT), the size of line q's workspace piece,
 * ta_forced_workspace_bytes(T, Lcap) -- which never decreases with L, so it holds every text within the cap -- and the
 * variants to launch: every one up to the widest cap's, each over all slots.  The kernel holds a slot to L[k] <=
 * Lcap[q] and 0 <= q < nlines_all on top of ta_forced_align's re-checks; a slot that fails gets TA_FORCED_BOUNDS and its
 * frames and score are left alone.  One launch per variant; nothing waits or allocates.
 */
int ta_forced_align_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all, const int64_t* ws_off_all,
                          const int32_t* Lcap, const int32_t* acc_line, const int32_t* L, const int64_t* lab_off,
                          const int32_t* labels, const int64_t* count, int32_t nlines_all, int32_t nslots, int32_t no,
                          int64_t rows, int64_t label_cap, const int32_t* T_all_host, const int32_t* Lcap_host,
                          void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status,
                          void* stream);
/*
 * ta_forced_align_omit: ta_forced_align with a lattice that may OMIT characters of the text (csrc/ta_forced_omit.hip;
 * DESIGN.md section 14.9, the rule of record; checker tests/forced_omit_ref.py).  omit_q, 0 .. TA_FORCED_OMIT_MAX in the
 * units of q, is the price of a character the path does not enter.  The path may start in any state (the characters in
 * front are paid for) and end in any (likewise); on top of stay / advance / skip a state of character i >= 1 may be
 * entered from any state s' <= 2 i - 2 for omit_q times the label states strictly between, ties stay > advance > skip >
 * far and the largest s' among equal far candidates; the end is the state with the largest total after its price, the
 * largest state on a tie.  frames: as ta_forced_align's for a character the path spends a frame in, TA_FORCED_OMITTED in
 * all three fields for one it never enters; score: the total, prices included.
 * Everything else -- arguments, [host] refusals, device re-checks, statuses -- is ta_forced_align's, with
 * ta_forced_omit_workspace_bytes(T, L) for the size of a line's piece (the moves, then one more bit per state and
 * timestep; -1 outside the bounds, 256-byte rows, never decreasing with L); omit_q outside its range is TA_EINVAL.
 */
#define TA_FORCED_OMIT_MAX (1 << 26)
#define TA_FORCED_OMITTED (-1)
int64_t ta_forced_omit_workspace_bytes(int32_t T, int32_t L);
int ta_forced_align_omit(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                         const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines, int32_t no,
                         int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host, int32_t omit_q,
                         void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status,
                         void* stream);
/*
 * ta_forced_align_omit_lines: ta_forced_align_omit (the same kernel body) for a line list that lies on the device, as
 * ta_harvest_pack leaves it: it relates to ta_forced_align_omit as ta_forced_align_lines relates
 * to ta_forced_align.  The arguments are ta_forced_align_lines' and mean the same, with omit_q in front of the workspace;
 * line q's workspace piece is ta_forced_omit_workspace_bytes(T, Lcap), which never decreases with L.  [host] refusals:
 * ta_forced_align_lines' (with that size function), and omit_q outside 0 .. TA_FORCED_OMIT_MAX is TA_EINVAL.  Per slot:
 * frames, score and status as ta_forced_align_omit's -- every character's three fields TA_FORCED_OMITTED or a frame
 * triple, the score with the prices in it; a slot at or behind count[0], and every slot of a call whose count[0] is
 * negative, writes nothing at all; a slot that fails a device re-check (L[k] <= Lcap[q] and 0 <= q < nlines_all among
 * them) gets TA_FORCED_BOUNDS or TA_FORCED_LABEL and its frames and score are left alone.  One launch per variant up to the
 * widest cap's, each over all slots; nothing waits or allocates.
 */
int ta_forced_align_omit_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all,
                               const int64_t* ws_off_all, const int32_t* Lcap, const int32_t* acc_line, const int32_t* L,
                               const int64_t* lab_off, const int32_t* labels, const int64_t* count, int32_t nlines_all,
                               int32_t nslots, int32_t no, int64_t rows, int64_t label_cap, const int32_t* T_all_host,
                               const int32_t* Lcap_host, int32_t omit_q, void* workspace, int64_t workspace_bytes,
                               int32_t* frames, int64_t* score, int32_t* status, void* stream);
/*
 * ta_forced_confidence: per-character confidence of a forced alignment from max-marginals (csrc/ta_forced_conf.hip;
 * DESIGN.md section 14.10, the rule of record; checker tests/forced_conf_ref.py), on ta_forced_align's strict lattice,
 * emission score q and skip rule.  A[t][s] is the aligner's forward total (the emission at t included), B[t][s] the best
 * total of frames t + 1 .. T - 1 from state s on to an end in S - 1 or S - 2, G[t][s] = A + B where both are above
 * -2^49 and exactly -2^50 elsewhere: the total of the best path that spends frame t in state s.  t_query [nlabels] int32,
 * row lab_off[b] + i = the frame queried for character i of line b.  Out: confidence [nlabels] int64, row lab_off[b] + i =
 * G[t][2 i + 1] minus the largest G[t][s] over s != 2 i + 1 (units of 2^-16 bit; at the aligner's own t_peak it is >= 0
 * and the first term is the line's score); rival [nlabels] int32, the smallest such s that attains it; status [nlines].
 * Arguments, [host] refusals and device re-checks are ta_forced_align's, with ta_forced_confidence_workspace_bytes(T, L)
 * = 512 K L bytes (a forward row of 64 K int64 per character, K the states per lane: 2 / 4 / 8 / 16 / 32 for 2 L + 1 <=
 * 128 / 256 / 512 / 1024 / 2047; -1 outside the bounds) for the size of a line's piece.  A line whose queries leave
 * 0 .. T - 1 or decrease with i gets TA_FORCED_QUERY (equal neighbours are allowed); a refused line touches nothing but
 * its status.  One launch per variant K the lines call for on `stream`; nothing waits or allocates.
 */
#define TA_FORCED_QUERY 4          /* a query frame outside 0 .. T - 1, or queries that decrease */
int64_t ta_forced_confidence_workspace_bytes(int32_t T, int32_t L);
int ta_forced_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                         const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, const int32_t* t_query,
                         int32_t nlines, int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                         const int32_t* L_host, void* workspace, int64_t workspace_bytes, int64_t* confidence,
                         int32_t* rival, int32_t* status, void* stream);
/*
 * ta_forced_confidence_lines: the same confidence (the same kernel body) for a line list that lies on the device, as
 * ta_harvest_pack leaves it and ta_forced_align_lines aligned it -- so a caller can enqueue it behind that call without a
 * look at the harvest table or at the frames.  It relates to ta_forced_confidence as ta_forced_align_lines relates to
 * ta_forced_align.  Packed slot k < count[0] takes the chunk's line q = acc_line[k] (rows row_off_all[q] .. + T_all[q]),
 * the labels labels[lab_off[k] .. + L[k]] and, as the query of character i, frames[(lab_off[k] + i) TA_FORCED_FIELDS + 2]:
 * its own t_peak, where the aligner left it (frames [label_cap][TA_FORCED_FIELDS]).  align_status [nslots] is the status
 * ta_forced_align_lines wrote: a filled slot whose entry is not TA_FORCED_OK reads neither its frames nor its labels and
 * writes only status[k] = TA_FORCED_SKIPPED.  A slot at or behind count[0], and every slot of a call whose count[0] is
 * negative, writes nothing at all.  Out: confidence [label_cap] int64 and rival [label_cap] int32, rows lab_off[k] + i;
 * status [nslots].
 * Workspace: slot k's piece starts at byte 512 Kmax lab_off[k] and holds L[k] rows of 512 K(L[k]) bytes, Kmax the widest
 * variant the call launches (that of the largest cap).  ta_harvest_pack gives every transcript character to at most one
 * slot and makes lab_off the running sum of L, so the pieces do not overlap and the call takes no offsets;
 * ta_forced_confidence_lines_workspace_bytes(label_cap, Lcap_max) = 512 K(Lcap_max) label_cap bytes holds them all (-1
 * for a negative size or Lcap_max outside 0 .. TA_FORCED_MAX_TARGET, 0 for Lcap_max = 0).
 * [host] T_all_host and Lcap_host as ta_forced_align_lines takes them, and from these alone its refusals (with the
 * workspace rule above in place of the sum over the lines) and the variants to launch: every one up to the widest cap's,
 * each over all slots.  The kernel holds a slot to 0 <= q < nlines_all, L[k] <= Lcap[q] and its piece inside
 * workspace_bytes on top of ta_forced_confidence's re-checks (TA_FORCED_BOUNDS, TA_FORCED_LABEL, TA_FORCED_QUERY); a
 * refused slot touches nothing but its status.  One launch per variant; nothing waits or allocates.
 */
#define TA_FORCED_SKIPPED 5        /* ta_forced_confidence_lines: the aligner did not give the slot TA_FORCED_OK */
int64_t ta_forced_confidence_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max);
int ta_forced_confidence_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all, const int32_t* Lcap,
                               const int32_t* acc_line, const int32_t* L, const int64_t* lab_off, const int32_t* labels,
                               const int64_t* count, const int32_t* align_status, const int32_t* frames,
                               int32_t nlines_all, int32_t nslots, int32_t no, int64_t rows, int64_t label_cap,
                               const int32_t* T_all_host, const int32_t* Lcap_host, void* workspace,
                               int64_t workspace_bytes, int64_t* confidence, int32_t* rival, int32_t* status,
                               void* stream);
/*
 * ta_forced_omit_confidence: ta_forced_confidence's max-marginals on ta_forced_align_omit's lattice
 * (csrc/ta_forced_omit_conf.hip; DESIGN.md section 14.18, the rule of record; checker tests/forced_omit_conf_ref.py):
 * stay / advance / skip, far at omit_q per label state jumped, a path that may start and end in any state.  A[t][s] is that
 * aligner's forward total, B[T-1][s] = -omit_q (L - ceil(s / 2)) its end rule, B[t][s] the best total of frames t + 1 ..
 * T - 1 from state s on, G = A + B: the total of the best path that spends frame t in state s -- every state is reachable,
 * no value stands for "none".  A query is a pair: line b has nq[b] of them, 0 .. 2 L[b], at q_off[b] .. + nq[b] of
 * q_char / q_frame [nqueries] int32 -- a character 0 .. L - 1 and a frame 0 .. T - 1, the frames never decreasing along
 * the line (equal neighbours and several queries per character are allowed).  Out: confidence [nqueries] int64, row
 * q_off[b] + j = G[t][2 i + 1] minus the largest G[t][s] over s != 2 i + 1 for query j = (i, t), in units of 2^-16 bit;
 * rival [nqueries] int32, the smallest such s that attains it; status [nlines].
 * The other arguments, the [host] refusals and the device re-checks are ta_forced_align_omit's, with
 * ta_forced_omit_confidence_workspace_bytes(T, L, nq) = 512 K nq bytes (a forward row of 64 K int64 per query; -1 outside
 * ta_forced_align's bounds or for nq outside 0 .. 2 L) for the size of a line's piece and nq_host [nlines], the [host]
 * copy of nq: an entry outside 0 .. 2 L or a sum above nqueries is TA_EINVAL.  On the device a line whose nq leaves
 * 0 .. 2 L, whose frames leave 0 .. T - 1 or decrease, or whose characters leave 0 .. L - 1 gets TA_FORCED_QUERY; queries
 * that leave q_char / q_frame TA_FORCED_BOUNDS.  A refused line touches nothing but its status, a refused call nothing.
 * One launch per variant K the lines call for on `stream`; nothing waits or allocates.
 */
int64_t ta_forced_omit_confidence_workspace_bytes(int32_t T, int32_t L, int32_t nq);
int ta_forced_omit_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                              const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, const int32_t* q_char,
                              const int32_t* q_frame, const int64_t* q_off, const int32_t* nq, int32_t nlines, int32_t no,
                              int64_t rows, int64_t nlabels, int64_t nqueries, const int32_t* T_host,
                              const int32_t* L_host, const int32_t* nq_host, int32_t omit_q, void* workspace,
                              int64_t workspace_bytes, int64_t* confidence, int32_t* rival, int32_t* status, void* stream);
/*
 * ta_forced_posterior: sum-product posteriors of a forced alignment and the text's likelihood per line
 * (csrc/ta_forced_post.hip; DESIGN.md section 14.11, the rule of record; checker tests/forced_post_ref.py), on
 * ta_forced_align's strict lattice and skip rule.  The emission is e(p) = (double)min(max(p, 2^-17), 1), with the two
 * float32 comparisons of the aligner's score.  Every value is a non-negative real with a 53-bit significand and an
 * unbounded exponent, every + and * rounded once to nearest-even, no fused multiply-add: a[t][s] the mass of all paths
 * through frames 0 .. t that are in state s at t, b[t][s] that of all continuations through t + 1 .. T - 1 to an end in
 * S - 1 or S - 2, g[t][s] = a b, Z = a[T-1][S-1] + a[T-1][S-2] = P(text | line).  t_query as ta_forced_confidence's.
 * Out, each value as a pair (significand in [0.5, 1) as frexp gives it, int32 exponent; zero is (0.0, 0)) that equals the
 * checker's bit for bit: own_m / own_x [nlabels], row lab_off[b] + i = g[t][2 i + 1]; rival_m / rival_x the largest g[t][s]
 * over s != 2 i + 1 and rival_state the smallest such s that attains it; z_m / z_x [nlines]; status [nlines].  A caller
 * forms posterior = ldexp(own_m / z_m, own_x - z_x) and log2 P(text | line) = log2(z_m) + z_x.
 * Arguments, [host] refusals and device re-checks are ta_forced_confidence's (TA_FORCED_BOUNDS, TA_FORCED_LABEL,
 * TA_FORCED_QUERY), with ta_forced_posterior_workspace_bytes(T, L) = 768 K L bytes (per character a forward row of 64 K
 * doubles and 64 K int32 exponents, K as above; -1 outside the bounds) for the size of a line's piece.  A refused line
 * touches nothing but its status.  One launch per variant K the lines call for on `stream`; nothing waits or allocates.
 */
int64_t ta_forced_posterior_workspace_bytes(int32_t T, int32_t L);
int ta_forced_posterior(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                        const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, const int32_t* t_query,
                        int32_t nlines, int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                        const int32_t* L_host, void* workspace, int64_t workspace_bytes, double* own_m, int32_t* own_x,
                        double* rival_m, int32_t* rival_x, int32_t* rival_state, double* z_m, int32_t* z_x,
                        int32_t* status, void* stream);
/*
 * ta_forced_posterior_lines: the same posteriors (the same kernel body) for a line list that lies on the device, as
 * ta_harvest_pack leaves it and ta_forced_align_lines aligned it.  It relates to ta_forced_posterior as
 * ta_forced_confidence_lines relates to ta_forced_confidence, and its arguments up to the workspace are that entry's:
 * packed slot k < count[0] takes the chunk's line q = acc_line[k] (rows row_off_all[q] .. + T_all[q]), the labels
 * labels[lab_off[k] .. + L[k]] and, as the query of character i, frames[(lab_off[k] + i) TA_FORCED_FIELDS + 2], its own
 * t_peak where the aligner left it.  A filled slot whose align_status is not TA_FORCED_OK reads neither its frames nor its
 * labels and writes only status[k] = TA_FORCED_SKIPPED; a slot at or behind count[0], and every slot of a call whose
 * count[0] is negative, writes nothing at all.  Out: own_m / own_x / rival_m / rival_x / rival_state [label_cap], rows
 * lab_off[k] + i; z_m / z_x / status [nslots], PER SLOT; every word equals tests/forced_post_ref.py bit for bit.
 * Workspace: slot k's piece starts at byte 768 Kmax lab_off[k] and holds L[k] rows of 768 K(L[k]) bytes, Kmax the widest
 * variant the call launches (that of the largest cap); the pieces do not overlap since the slots' labels do not, and
 * ta_forced_posterior_lines_workspace_bytes(label_cap, Lcap_max) = 768 K(Lcap_max) label_cap bytes holds them all (-1 for
 * a negative size or Lcap_max outside 0 .. TA_FORCED_MAX_TARGET, 0 for Lcap_max = 0).
 * [host] T_all_host and Lcap_host as ta_forced_align_lines takes them, and from these alone the refusals (those of
 * ta_forced_confidence_lines) and the variants to launch: every one up to the widest cap's, each over all slots.  The
 * kernel holds a slot to 0 <= q < nlines_all, L[k] <= Lcap[q] and its piece inside workspace_bytes on top of
 * ta_forced_posterior's re-checks (TA_FORCED_BOUNDS, TA_FORCED_LABEL, TA_FORCED_QUERY); a refused slot touches nothing
 * but its status.  One launch per variant; nothing waits or allocates.
 */
int64_t ta_forced_posterior_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max);
int ta_forced_posterior_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all, const int32_t* Lcap,
                              const int32_t* acc_line, const int32_t* L, const int64_t* lab_off, const int32_t* labels,
                              const int64_t* count, const int32_t* align_status, const int32_t* frames,
                              int32_t nlines_all, int32_t nslots, int32_t no, int64_t rows, int64_t label_cap,
                              const int32_t* T_all_host, const int32_t* Lcap_host, void* workspace,
                              int64_t workspace_bytes, double* own_m, int32_t* own_x, double* rival_m, int32_t* rival_x,
                              int32_t* rival_state, double* z_m, int32_t* z_x, int32_t* status, void* stream);

/*
 * Page-scope forced alignment (csrc/ta_forced_page.hip; DESIGN.md section 14.8, the rule of record; checker
 * tests/forced_page_ref.py): ONE best CTC path through the frames of all the lines of a page, one wave per page.
 * [device] pointers unless marked [host]; one launch per variant on `stream`, nothing waits or allocates.
 * Page p owns the lines line_first[p] .. line_first[p + 1] (in reading order) and the labels labels[lab_off[p] ..
 * lab_off[p + 1]) (n of them, 1 <= code < no); line q owns the probability rows row_off[q] .. + T[q], the window of
 * characters [lo[q], hi[q]) of its page's text and the workspace piece at ws_off[q] BYTES (a multiple of 16).  During a
 * line's frames only the states 2 lo .. 2 hi are live.  Windows: the first starts at 0, the last ends at n, lo[q] <=
 * lo[q + 1] <= hi[q] <= hi[q + 1], 0 <= hi - lo <= TA_FORCED_MAX_TARGET.  Stay / advance / skip, ties in that order, as
 * ta_forced_align -- but a character never stays from one line's last frame into the next line's first.
 * The page's variant K (states per lane) is that of its widest window, ta_forced_page_variant(width); line q's piece
 * holds 256 * rows(T[q], K) bytes, and ta_forced_page_workspace_bytes(nl, T [host], K) is the sum over a page's lines
 * (-1 for nl < 1, a T outside 1 .. TA_TRAIN_MAX_T or a K that is no variant).
 * Out: frames [nlabels][TA_FORCED_PAGE_FIELDS] int32, row lab_off[p] + i = line (in the page), t_first, t_last, t_peak
 * of character i, the timesteps local to that line; score [npages] int64; status [npages].  A page whose best end is
 * below -2^49 has no path (fewer frames than characters, for one): TA_FORCED_NOPATH, frames and score left alone.
 * [host] copies T_host, line_first_host, lo_host, hi_host, lab_off_host: from these the refusals before anything is
 * launched -- a page without lines or text, T < 1, a window that breaks the conditions above, timesteps above rows,
 * labels above nlabels, a workspace below the pages' sum or not 16-byte aligned, a null pointer, a negative size are
 * TA_EINVAL; a window wider than TA_FORCED_MAX_TARGET or T > TA_TRAIN_MAX_T TA_ELIMIT.  The kernel re-checks every bound
 * on the device's numbers (windows, offsets against rows / nlabels / workspace_bytes, T, the variant against the call's
 * launches: TA_FORCED_BOUNDS; labels: TA_FORCED_LABEL); a refused page touches nothing but its status.
 */
#define TA_FORCED_PAGE_FIELDS 4    /* line, t_first, t_last, t_peak */
#define TA_FORCED_NOPATH 3         /* no path through the page's windows */
int64_t ta_forced_page_workspace_bytes(int32_t nl, const int32_t* T, int32_t K);
int32_t ta_forced_page_variant(int32_t width);
int ta_forced_align_pages(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                          const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                          const int64_t* ws_off, int32_t npages, int32_t nlines, int32_t no, int64_t rows, int64_t nlabels,
                          const int32_t* T_host, const int64_t* line_first_host, const int32_t* lo_host,
                          const int32_t* hi_host, const int64_t* lab_off_host, void* workspace, int64_t workspace_bytes,
                          int32_t* frames, int64_t* score, int32_t* status, void* stream);

/*
 * Page scope inside the pipeline: windows and eligibility on the device, and the page aligner
 * without host windows.  [device] pointers unless marked [host]; nothing waits or allocates.
 *
 * ta_page_windows (csrc/ta_page_windows.hip; checkers forced.page_scope_eligibility / tests/forced_page_ref.py's
 * page_windows): one launch, a wave per page, behind ta_harvest_lines on `stream`.  In, where the harvest left them: table
 * [nlines][TA_HARVEST_FIELDS] (fields 0 - 2 are read: reason, t_first, L), harvest_status [npages], line_first
 * [npages + 1], t_off [npages + 1] (page p's n transcript characters are t_class[t_off[p] .. t_off[p + 1])), t_class
 * [t_len], T [nlines], plain [npages] (a byte: the page's syllables are formed on the array path), margin (characters a
 * window reaches beyond its line's core).  Out: reason [npages] -- the first TA_PAGE_SCOPE_* that applies, in the order of
 * their numbers (WINDOWS: no lines, or a window wider than TA_FORCED_MAX_TARGET; FRAMES: n above the page's timesteps) --
 * and, for a page with reason 0 alone, lo / hi [nlines]: a line without TA_HARVEST_EMPTY / TA_HARVEST_PAGE has the core
 * [t_first, t_first + L), any other the empty range at the latest earlier core's end (0 in front of the first); lo =
 * max(start - margin, 0), hi = min(end + margin, n), lo_0 = 0, hi_last = n, hi a running maximum, lo_k = min(max(lo_k,
 * lo_{k-1}), hi_{k-1}).  A page whose line_first or t_off decrease or leave nlines / t_len gets TA_PAGE_WINDOWS_BOUNDS and
 * nothing else of it is read or written.  Null pointers (npages > 0), negative sizes and margin < 0 are TA_EINVAL.
 *
 * ta_forced_align_pages_gated (csrc/ta_forced_page.hip): ta_forced_align_pages' kernel and outputs for the pages whose
 * gate [npages] is 0; a page with gate != 0 gets status TA_FORCED_SKIPPED and nothing else of it is read or written -- it
 * may have no lines or no text.  lo / hi stay on the device (ta_page_windows wrote them); the host sizes by cap instead:
 * cap_host [host] / cap [npages], the widest window a page may have (min(n, TA_FORCED_MAX_TARGET)), and line q's
 * workspace piece holds 256 * rows(T[q], ta_forced_page_variant(cap of its page)) bytes -- rows never decreases with K, so
 * the piece holds whatever variant the device's windows call for; ta_forced_page_gated_workspace_bytes(nl, T [host],
 * cap) is the sum over a page's lines (-1 as ta_forced_page_workspace_bytes, and for a cap outside 0 ..
 * TA_FORCED_MAX_TARGET).  One launch per variant up to the widest cap's, over all pages.  On the device ta_forced_align_pages'
 * re-checks, and a page whose windows need a wider variant than its cap's is TA_FORCED_BOUNDS.  [host] refusals: those of
 * ta_forced_align_pages that need no window -- line_first or lab_off that decrease are TA_EINVAL, a page without lines or
 * without text is NOT refused (the gate decides), a cap below 0 TA_EINVAL, above TA_FORCED_MAX_TARGET TA_ELIMIT.
 */
#define TA_PAGE_SCOPE_REFINED 0
#define TA_PAGE_SCOPE_NOT_PLAIN 1  /* the page's syllables take the object path */
#define TA_PAGE_SCOPE_HARVEST 2    /* the harvest refused the page */
#define TA_PAGE_SCOPE_CLASS0 3     /* a transcript character outside the codec */
#define TA_PAGE_SCOPE_NO_TEXT 4
#define TA_PAGE_SCOPE_WINDOWS 5    /* no lines, or a window wider than TA_FORCED_MAX_TARGET */
#define TA_PAGE_SCOPE_FRAMES 6     /* fewer frames than characters */
#define TA_PAGE_SCOPE_NO_PATH 7    /* set by the host where ta_forced_align_pages_gated says TA_FORCED_NOPATH */
#define TA_PAGE_WINDOWS_BOUNDS (-1)
int ta_page_windows(const int32_t* table, const int32_t* harvest_status, const int64_t* line_first, const int64_t* t_off,
                    const int32_t* t_class, const int32_t* T, const uint8_t* plain, int32_t npages, int32_t nlines,
                    int64_t t_len, int32_t margin, int32_t* lo, int32_t* hi, int32_t* reason, void* stream);
int64_t ta_forced_page_gated_workspace_bytes(int32_t nl, const int32_t* T, int32_t cap);
int ta_forced_align_pages_gated(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                                const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                                const int64_t* ws_off, const int32_t* gate, const int32_t* cap, int32_t npages,
                                int32_t nlines, int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                                const int64_t* line_first_host, const int64_t* lab_off_host, const int32_t* cap_host,
                                void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score,
                                int32_t* status, void* stream);

/*
 * Page-scope forced alignment that may omit characters (csrc/ta_forced_page_omit.hip; DESIGN.md section 14.12, the rule
 * of record; checker tests/forced_page_omit_ref.py): ta_forced_align_pages' lattice with ta_forced_align_omit's far move.
 * The arguments are ta_forced_align_pages' and mean the same, plus omit_q, 0 .. TA_FORCED_OMIT_MAX in the units of the
 * emission score: the price of a character the path does not enter.  Every state of the first window may start the
 * path and every state of the last may end it, the characters in front and behind paid for; a far move on a line's
 * first frame may start in any state of the PREVIOUS line's window, those below the new window included; a character
 * still never stays across a line break.  Under this rule every page has a path, whatever its number of frames.
 * All five variants K are built.  Line q's piece holds its move rows as ta_forced_align_pages' and, behind them, its bit
 * rows as ta_forced_align_omit's: 256 * (rows(T[q], K) + ceil(T[q] / (32 / K))) bytes;
 * ta_forced_page_omit_workspace_bytes(nl, T [host], K) is the sum over a page's lines (-1 as
 * ta_forced_page_workspace_bytes).
 * Out: frames [nlabels][TA_FORCED_PAGE_FIELDS] as ta_forced_align_pages' for a character the path spends a frame in,
 * four TA_FORCED_OMITTED for one it never enters; score [npages]: the path's total less omit_q per omitted character.
 * Refusals: ta_forced_align_pages', and omit_q outside its range TA_EINVAL, a page of more than 2^20 characters or more
 * than 2^25 frames TA_ELIMIT (on the device, as omit_q: TA_FORCED_BOUNDS).  A refused call does not touch a word, a
 * refused page nothing but its status.
 */
#define TA_PAGE_SCOPE_TOO_LONG 8     /* with omission: more than 2^20 characters or 2^25 frames (ta_page_windows_omit) */
#define TA_PAGE_SCOPE_ALL_OMITTED 9  /* set by the host where the path of a page with omission holds no character */
int64_t ta_forced_page_omit_workspace_bytes(int32_t nl, const int32_t* T, int32_t K);
int ta_forced_align_pages_omit(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                               const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                               const int64_t* ws_off, int32_t npages, int32_t nlines, int32_t no, int64_t rows,
                               int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                               const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host, int32_t omit_q,
                               void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status,
                               void* stream);

/*
 * Page scope with omission behind the harvest, device-resident: the pair of section 14.14 for the
 * lattice with omission.  [device] pointers unless marked [host]; nothing waits or allocates.
 *
 * ta_page_windows_omit (csrc/ta_page_windows_omit.hip; checker forced.page_scope_eligibility(..., omit=True)):
 * ta_page_windows' arguments, windows, reasons 1 - 5, precedence, TA_PAGE_WINDOWS_BOUNDS and [host] refusals.
 * TA_PAGE_SCOPE_FRAMES never occurs; behind TA_PAGE_SCOPE_WINDOWS a page of more than 2^20 characters or more than 2^25
 * frames gets TA_PAGE_SCOPE_TOO_LONG.  lo / hi are written for reason 0 alone.
 *
 * ta_forced_align_pages_omit_gated (csrc/ta_forced_page_omit_gated.hip): ta_forced_align_pages_omit's kernel and outputs
 * for the pages whose gate [npages] is 0; a page with gate != 0 gets TA_FORCED_SKIPPED in front of every other check and
 * nothing else of it is read or written.  Arguments as ta_forced_align_pages_gated, plus omit_q.  Line q's piece holds
 * 256 * (rows(T[q], K) + ceil(T[q] / (32 / K))) bytes at K = ta_forced_page_variant(cap of its page) -- neither term
 * decreases with K; ta_forced_page_omit_gated_workspace_bytes(nl, T [host], cap) is the sum over a page's lines (-1 as
 * ta_forced_page_gated_workspace_bytes).  One launch per variant up to the widest cap's.  On the device: a cap outside 0 ..
 * TA_FORCED_MAX_TARGET, or windows that need a wider variant than the cap's, are TA_FORCED_BOUNDS.  [host] refusals:
 * ta_forced_align_pages_gated's, with a page of more than 2^20 characters or 2^25 frames TA_ELIMIT and omit_q outside 0 ..
 * TA_FORCED_OMIT_MAX TA_EINVAL.
 */
int ta_page_windows_omit(const int32_t* table, const int32_t* harvest_status, const int64_t* line_first,
                         const int64_t* t_off, const int32_t* t_class, const int32_t* T, const uint8_t* plain,
                         int32_t npages, int32_t nlines, int64_t t_len, int32_t margin, int32_t* lo, int32_t* hi,
                         int32_t* reason, void* stream);
int64_t ta_forced_page_omit_gated_workspace_bytes(int32_t nl, const int32_t* T, int32_t cap);
int ta_forced_align_pages_omit_gated(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                                     const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                                     const int64_t* ws_off, const int32_t* gate, const int32_t* cap, int32_t npages,
                                     int32_t nlines, int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                                     const int64_t* line_first_host, const int64_t* lab_off_host, const int32_t* cap_host,
                                     int32_t omit_q, void* workspace, int64_t workspace_bytes, int32_t* frames,
                                     int64_t* score, int32_t* status, void* stream);

/*
 * Per-character confidence at page scope from max-marginals (csrc/ta_forced_page_conf.hip; DESIGN.md section 14.13, the
 * rule of record; checker tests/forced_page_conf_ref.py), on ta_forced_align_pages' strict lattice: windows, live states,
 * emission score, skip rule, no character across a line break.  The frames of a page are ordered (line, t).  A is the
 * aligner's forward total after a frame, B the best total of all later frames from state s on to an end in 2 n or 2 n - 1,
 * G = A + B where both are above -2^49 and exactly -2^50 elsewhere: the total of the best legal path of the page that
 * spends the frame in state s.  query [nlabels][TA_FORCED_PAGE_FIELDS] int32, row lab_off[p] + i: field 0 the line (in the
 * page) and field 3 the frame (local to that line) queried for character i; fields 1 and 2 are not read, so
 * ta_forced_align_pages' frames can be handed over where they lie.  Out: confidence [nlabels] int64, row lab_off[p] + i =
 * G[2 i + 1] at the query frame minus the largest G[s] over the live states s != 2 i + 1 of the query line's window (units
 * of 2^-16 bit; at the aligner's own line and t_peak it is >= 0 and the first term is the page's score); rival [nlabels]
 * int32, the smallest such PAGE state that attains it (2 lo of the query line where no rival is reachable: the second
 * term is -2^50 then); status [npages].
 * The arguments up to lab_off are ta_forced_align_pages' and mean the same.  ws_off [npages]: page p's ONE workspace
 * piece at ws_off[p] BYTES (a multiple of 16) holds ta_forced_page_confidence_workspace_bytes(n, K) = 512 K n bytes, a
 * forward row of 64 K int64 per character, K the page's variant (-1 for n outside 1 .. 2^29 or a K that is no variant).
 * [host] refusals are ta_forced_align_pages', with the workspace rule above, and a page of more than 2^25 frames is
 * TA_ELIMIT.  The kernel re-checks every bound on the device's numbers (TA_FORCED_BOUNDS, a page of more than 2^25 frames
 * among them; TA_FORCED_LABEL) and the queries: a line outside the page, a frame outside its line, a character outside
 * its query line's window or queries that decrease in (line, frame) order are TA_FORCED_QUERY (equal neighbours are
 * allowed).  A page without a path gets TA_FORCED_NOPATH and its outputs are left alone; a refused page touches nothing
 * but its status.  One launch per variant on `stream`; nothing waits or allocates.
 */
int64_t ta_forced_page_confidence_workspace_bytes(int64_t n, int32_t K);
int ta_forced_page_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                              const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                              const int64_t* ws_off, const int32_t* query, int32_t npages, int32_t nlines, int32_t no,
                              int64_t rows, int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                              const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host, void* workspace,
                              int64_t workspace_bytes, int64_t* confidence, int32_t* rival, int32_t* status, void* stream);

/*
 * Sum-product posteriors at page scope and the page's likelihood (csrc/ta_forced_page_post.hip; DESIGN.md section 14.15,
 * the rule of record; checker tests/forced_page_post_ref.py), on ta_forced_align_pages' strict lattice -- windows, live
 * states, skip rule, no character across a line break -- with ta_forced_posterior's emission and arithmetic: e(p) =
 * min(max(p, 2^-17), 1), every value a pair (53-bit significand, unbounded exponent), every + and * rounded once.  The
 * frames of a page are ordered (line, t).  a is the mass of all legal beginnings that reach state s at a frame, b the mass
 * of all legal continuations from it to an end in 2 n or 2 n - 1, g = a b, Z = a_last[2 n] + a_last[2 n - 1] the mass of
 * all legal paths of the page: log2 P(text | page) = log2(z_m) + z_x.
 * The arguments up to query are ta_forced_page_confidence's and mean the same (query: field 0 the line, field 3 the
 * frame; ta_forced_align_pages' frames can be handed over where they lie).  ws_off [npages]: page p's ONE workspace piece
 * at ws_off[p] BYTES (a multiple of 16) holds ta_forced_page_posterior_workspace_bytes(n, K) = 768 K n bytes, per
 * character a forward row of 64 K doubles then 64 K int32 exponents, K the page's variant (-1 for n outside 1 .. 2^29 or
 * a K that is no variant).
 * Out, every pair normalised as frexp does and zero as (0.0, 0): own_m [nlabels] double / own_x [nlabels] int32, row
 * lab_off[p] + i = g[2 i + 1] at character i's query frame; rival_m / rival_x: the largest g[s] over the live states
 * s != 2 i + 1 of the query line's window, by exponent, then significand; rival_state [nlabels] int32: the smallest such
 * PAGE state that attains it (2 lo of the query line where every rival is zero); z_m [npages] double / z_x [npages]
 * int32; status [npages].  posterior = ldexp(own_m / z_m, own_x - z_x).
 * [host] refusals are ta_forced_align_pages', with the workspace rule above, and a page of more than 2^24 frames is
 * TA_ELIMIT (every exponent then stays above -17 2^24 - 2, clear of the kernel's zero).  The kernel re-checks every bound
 * on the device's numbers (TA_FORCED_BOUNDS, a page of more than 2^24 frames among them; TA_FORCED_LABEL) and the queries
 * as ta_forced_page_confidence does (TA_FORCED_QUERY).  A page without a path (Z = 0 exactly) gets TA_FORCED_NOPATH and
 * its outputs, z_m and z_x included, are left alone; a refused page touches nothing but its status; a refused call does
 * not touch a word.  One launch per variant on `stream`; nothing waits or allocates.
 */
int64_t ta_forced_page_posterior_workspace_bytes(int64_t n, int32_t K);
int ta_forced_page_posterior(const float* probs, const int64_t* row_off, const int32_t* T, const int64_t* line_first,
                             const int32_t* lo, const int32_t* hi, const int32_t* labels, const int64_t* lab_off,
                             const int64_t* ws_off, const int32_t* query, int32_t npages, int32_t nlines, int32_t no,
                             int64_t rows, int64_t nlabels, const int32_t* T_host, const int64_t* line_first_host,
                             const int32_t* lo_host, const int32_t* hi_host, const int64_t* lab_off_host, void* workspace,
                             int64_t workspace_bytes, double* own_m, int32_t* own_x, double* rival_m, int32_t* rival_x,
                             int32_t* rival_state, double* z_m, int32_t* z_x, int32_t* status, void* stream);

/*
 * The refined lines' column runs replaced on the device (csrc/ta_refine.hip; checker
 * tests/refine_ref.py): forced.refine_columns as ONE launch, a wave per page, behind ta_harvest_lines, ta_harvest_pack and
 * ta_forced_align_lines on `stream`.  [device] pointers throughout; nothing waits or allocates.
 * In: the aligner's columns (ops, ops_off, ops_len, ops_bytes: page p's ops_len[p] columns lie right-aligned in the region
 * of n + m bytes at ops_off[p]; t_off / o_off [nprob + 1] give n and m, t_len / o_len bound them), o_line and line_first as
 * ta_harvest_lines took them, idx [o_len] (per OCR character its row of the old box array, at o_off[p] + j), the harvest's
 * table and status, the packed acc_line / L / lab_off / count (nslots: the slots the arrays hold, label_cap as
 * ta_harvest_pack's), the forced alignment's status per slot, plain [nprob] (non-zero: the page's syllables are formed
 * on the array path) and box_base, the rows of the old box array.
 * A line is refined iff its reason is 0, it has a slot k < count[0] (acc_line[k] == line; acc_line ascending), the forced
 * status of k is TA_FORCED_OK, L[k] <= TA_FORCED_MAX_TARGET and its page is plain.  A count[0] below 0 fills no slot.
 * Out, buffers of their own: ops_new [ops_bytes] -- page p's new columns from ops_off[p] on, LEFT-aligned, ops_new_len[p]
 * of them (never more than ops_len[p]: a refined run loses its op-2 columns); idx_new [ops_bytes] int32 -- from ops_off[p]
 * on the box row of every OCR-carrying new column, idx_new_len[p] of them (a refined line may carry more pairs than it had
 * OCR characters, hence the columns' region): kept character i of slot k has row box_base + lab_off[k] + i, every other
 * one its old row; refined [nlines] (0 / 1), slot [nlines] (a refined line's k, else -1); status [nprob].
 * The kernel re-checks what forced.refine_columns checks, on the device's numbers: o_line never decreasing inside the
 * page's lines, the columns carrying n and m characters, every refined line with OCR characters and t_first .. + L inside
 * the transcript range of its run, its packed L equal to the table's.  A page that fails, and a page the harvest refused,
 * gets a non-zero status, its columns and idx copied through unchanged and none of its lines refined; only a page whose
 * offsets themselves are out of bounds (TA_REFINE_BOUNDS) has nothing copied, lengths of -1 and its lines left alone.
 * Negative sizes and null pointers are TA_EINVAL, box_base + label_cap beyond 32 bits TA_ELIMIT.
 */
#define TA_REFINE_OK 0
#define TA_REFINE_HARVEST 1        /* the harvest refused the page (its status is not TA_HARVEST_OK) */
#define TA_REFINE_BOUNDS 2         /* the page's offsets, ops_len or line range are out of bounds */
#define TA_REFINE_COLUMNS 3        /* o_line decreases or leaves the page's lines, or the columns disagree with n and m */
#define TA_REFINE_CONTAIN 4        /* a refined line's kept characters are not inside its run, or its slot disagrees with the table */
int ta_refine_columns(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                      const int64_t* t_off, const int64_t* o_off, int64_t t_len, int64_t o_len, int32_t nprob,
                      const int32_t* o_line, const int64_t* line_first, const int32_t* idx, const int32_t* table,
                      const int32_t* harvest_status, int32_t nlines, const int32_t* acc_line, const int32_t* L,
                      const int64_t* lab_off, const int64_t* count, int32_t nslots, int64_t label_cap,
                      const int32_t* forced_status, const uint8_t* plain, int32_t box_base, uint8_t* ops_new,
                      int32_t* ops_new_len, int32_t* idx_new, int32_t* idx_new_len, int32_t* refined, int32_t* slot,
                      int32_t* status, void* stream);
/*
 * ta_refine_columns_omit: ta_refine_columns behind ta_forced_align_omit_lines, whose path may leave characters of a line's
 * text out (the same kernel, its second instantiation; DESIGN.md section 14.16, the rule of record; checker
 * tests/refine_omit_ref.py): forced.refine_columns(..., present=...) on the device.  The arguments are ta_refine_columns'
 * plus frames [label_cap][TA_FORCED_FIELDS] as the aligner wrote them and the output omitted [nlines].
 * Character i of slot k is PRESENT iff frames[3 (lab_off[k] + i)] >= 0; any negative first field counts as omitted.
 * omitted[q] is the number of characters of line q's slot that are not present, for a line with a filled slot whose forced
 * status is TA_FORCED_OK, L[k] <= TA_FORCED_MAX_TARGET and rows lab_off[k] .. + L[k] inside label_cap (L[k] >= 1), whether
 * or not its page is plain; -1 for every other line and for every line of a page whose status is not TA_REFINE_OK.
 * A line is refined iff ta_refine_columns' predicate holds AND it has a present character; a line with none keeps its
 * run, op-2 columns included.  In a refined run the kept character i is a pair (op 0) if present and an op-1 column if
 * not; the box row of a present one is box_base + lab_off[k] + i as before, the rows of omitted ones are never referenced.
 * Statuses, containment checks (on every line of ta_refine_columns' predicate), the copy-through of a refused page and the
 * host's refusals are ta_refine_columns'.
 */
int ta_refine_columns_omit(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                           const int64_t* t_off, const int64_t* o_off, int64_t t_len, int64_t o_len, int32_t nprob,
                           const int32_t* o_line, const int64_t* line_first, const int32_t* idx, const int32_t* table,
                           const int32_t* harvest_status, int32_t nlines, const int32_t* acc_line, const int32_t* L,
                           const int64_t* lab_off, const int64_t* count, int32_t nslots, int64_t label_cap,
                           const int32_t* forced_status, const int32_t* frames, const uint8_t* plain, int32_t box_base,
                           uint8_t* ops_new, int32_t* ops_new_len, int32_t* idx_new, int32_t* idx_new_len,
                           int32_t* refined, int32_t* slot, int32_t* omitted, int32_t* status, void* stream);
/*
 * The refined lines' confidences per transcript character and per syllable, on the device (csrc/ta_refine_conf.hip;
 * DESIGN.md section 14.10; checker tests/refine_conf_ref.py): ONE launch, a wave per page, behind
 * ta_forced_confidence_lines and ta_refine_columns on `stream`.  [device] pointers throughout; nothing waits or allocates.
 * In: confidence [label_cap] and its status per slot as ta_forced_confidence_lines wrote them, the packed lab_off / L /
 * count, the harvest's table, line_first, refined and slot [nlines] as ta_refine_columns wrote them, t_off [nprob + 1]
 * (page p's transcript characters are t_off[p] .. t_off[p + 1] of t_len), and per page the syllables syl_off[p] ..
 * syl_off[p + 1] of nsyl: syl_first / syl_last, the inclusive range of a syllable's characters inside its page.
 * Out: char_conf [t_len] int64 -- TA_NO_CONFIDENCE everywhere, except that kept character i of refined line q with slot k
 * holds confidence[lab_off[k] + i] at t_off[p] + table[q][1] + i; syl_conf [nsyl] int64 -- the smallest char_conf of the
 * syllable's range among those that are not TA_NO_CONFIDENCE, else TA_NO_CONFIDENCE; status [nprob].  A page with a
 * non-zero status has nothing else written: its own offsets out of bounds (TA_CONF_PAGES_BOUNDS), a syllable's range
 * outside its characters (RANGE), a refined line whose kept characters leave the page's or whose labels leave label_cap
 * (TABLE), a refined line without a filled slot (SLOT) or whose confidence status is not TA_FORCED_OK (STATUS).
 * Negative sizes and null pointers are TA_EINVAL, nlines above TA_HARVEST_MAX_LINES TA_ELIMIT.
 */
#define TA_NO_CONFIDENCE INT64_MIN
#define TA_CONF_PAGES_OK 0
#define TA_CONF_PAGES_BOUNDS 1     /* the page's offsets or line range are out of bounds */
#define TA_CONF_PAGES_RANGE 2      /* a syllable's range leaves the page's characters */
#define TA_CONF_PAGES_TABLE 3      /* a refined line's kept characters leave the page's, or its labels label_cap */
#define TA_CONF_PAGES_SLOT 4       /* a refined line without a filled slot */
#define TA_CONF_PAGES_STATUS 5     /* a refined line whose confidence status is not TA_FORCED_OK */
int ta_confidence_pages(const int64_t* confidence, const int64_t* lab_off, const int32_t* L, const int64_t* count,
                        const int32_t* conf_status, int32_t nslots, int64_t label_cap, const int32_t* table,
                        const int64_t* line_first, const int32_t* refined, const int32_t* slot, int32_t nlines,
                        const int64_t* t_off, int64_t t_len, const int32_t* syl_first, const int32_t* syl_last,
                        const int64_t* syl_off, int64_t nsyl, int32_t nprob, int64_t* char_conf, int64_t* syl_conf,
                        int32_t* status, void* stream);
/*
 * The refined lines' posteriors per transcript character and per syllable, on the device (csrc/ta_refine_conf.hip, the
 * kernel body of ta_confidence_pages; checker tests/refine_post_ref.py): ONE launch, a wave per
 * page, behind ta_forced_posterior_lines and ta_refine_columns on `stream`.  In: own_m / own_x [label_cap] and z_m / z_x /
 * post_status [nslots] as ta_forced_posterior_lines wrote them; everything else is ta_confidence_pages'.
 * Out: char_post [t_len] float64 -- TA_NO_POSTERIOR everywhere, except that kept character i of refined line q with slot
 * k holds ldexp(own_m[lab_off[k] + i] / z_m[k], own_x[lab_off[k] + i] - z_x[k]), one IEEE double division and one ldexp
 * (a zero mass (0.0, 0) gives +0.0; a result in the subnormal range is rounded once, to nearest-even); syl_post [nsyl]
 * float64 -- the smallest char_post of the syllable's range among those that are no NaN, else TA_NO_POSTERIOR; status
 * [nprob], the TA_CONF_PAGES_* codes with ta_confidence_pages' meanings (STATUS: a refined line whose post_status is not
 * TA_FORCED_OK).  A page with a non-zero status has nothing else written.  Refusals as ta_confidence_pages'.
 */
#define TA_NO_POSTERIOR 0x7FF8000000000000LL     /* the bits of the quiet NaN that stands for "no value" */
int ta_posterior_pages(const double* own_m, const int32_t* own_x, const double* z_m, const int32_t* z_x,
                       const int64_t* lab_off, const int32_t* L, const int64_t* count, const int32_t* post_status,
                       int32_t nslots, int64_t label_cap, const int32_t* table, const int64_t* line_first,
                       const int32_t* refined, const int32_t* slot, int32_t nlines, const int64_t* t_off, int64_t t_len,
                       const int32_t* syl_first, const int32_t* syl_last, const int64_t* syl_off, int64_t nsyl,
                       int32_t nprob, double* char_post, double* syl_post, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TEXT_ALIGNMENT_AMD_H */
