// ta_forced_post.hip -- sum-product posteriors of a forced alignment and the text's likelihood per line (DESIGN.md
// section 14.11).  For a query frame t per character i of a line's text: the mass of ALL CTC paths that spend frame t in the
// character's own state 2 i + 1, the largest such mass over the other states with the state that has it, and per line the
// mass Z of all paths -- on the lattice and the skip rule of ta_forced.hip.  The checker of record is
// tests/forced_post_ref.py, and every word written here equals it bit for bit.  Two entries, one kernel body:
// ta_forced_posterior (a line list from the host, a query array) and ta_forced_posterior_lines (the packed slots
// ta_harvest_pack left on the device, the queries the t_peak ta_forced_align_lines left in its frames: kSlots).
//
// The rule's arithmetic: a value is a non-negative real with a 53-bit significand and an unbounded exponent, every + and *
// rounded once to nearest-even.  Here a value is a pair (double m, int x) = m 2^x that is NOT kept normalised:
//   times e    e in [2^-17, 1] is a clamped float32 probability: m * e, one double multiply of normal numbers, x stays;
//   plus       x = the larger exponent, both significands brought there by ldexp (exact: nothing leaves the normal range)
//              and ONE double add.  A term more than kShift binades down is shifted by kShift: the add rounds it away.
//   zero       is (0.0, kZeroX), below every exponent that occurs, so it never sets a sum's exponent.
// Once per chunk of kChunk = 8 timesteps every state is renormalised (frexp: m back in [0.5, 1)); within a chunk a
// significand moves by a factor in [2^-136, 3^8], so it stays in [2^-137, 2^13): far inside double's normal range, and
// kShift = 256 exceeds the spread of two significands (150 binades) by more than the 54 bits below which a term cannot
// change a sum.  The results therefore do not depend on where the renormalisation happens; no subnormal occurs, so not on
// the denormal mode either.  Built with -ffp-contract=off: a fused multiply-add would change the bits.
//
// forced_post_kernel<K, kSlots>, one wave per line, the layout of forced_common.h and the structure of forced_conf_kernel: lane l
// holds the K consecutive states l K .. l K + K - 1 as (double, int) registers.  ONE wave runs both fills -- the control
// structure is two_fill's and the kernel's way to its line two_fill_prologue's (forced_two_fill.h, shared with
// ta_forced_conf.hip); the arithmetic is PostCells of forced_post_cells.h, shared with ta_forced_page_post.hip:
//   forward   a[t][s]; only the left lane's last value crosses a lane boundary (from_left and one DPP move for the
//             exponent).  The row of every query frame goes to the workspace, row i for character i (queries do not
//             decrease, so one cursor meets them in order): 64 K doubles, then 64 K exponents.  At the end Z.
//   backward  b[t][s], walked from the last chunk of emissions to the first; across a lane boundary the RIGHT lane's first
//             two values are needed.  At a query frame the character's forward row comes back to the lane that stored it,
//             g = a b, every lane keeps the best of its states but the character's own, and 64 candidates meet in LDS,
//             ordered by exponent, then significand, then the smaller state.  That happens L times per line, not T times.
// No barrier and no wave-wide reduction in a fill.  Padding states (s >= S) stay zero in the backward fill, so their g is
// zero; they are no rivals.  Every bound is re-checked on the line's own device numbers before anything is read through it;
// a refused line gets a status and touches nothing else.
#include "forced_post_cells.h"

namespace {

struct PostArgs : TwoFillArgs {
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state; double* z_m; int32_t* z_x;
};

// the blocks, their lines and their statuses: two_fill_prologue.  z_m, z_x and status are per block (line or SLOT).
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_post_kernel(PostArgs a) {
    __shared__ float etab[2 * kChunk * kMaxNo];        // two chunks of emissions (8 KiB)
    __shared__ PostRed red;
    const int b = blockIdx.x, lane = threadIdx.x;
    TwoFillLine line;
    int64_t l0;
    if (!two_fill_prologue<K, kSlots, PostCells>(a, b, lane, &line, &l0)) return;
    const PostLine ln{line, a.own_m + l0, a.own_x + l0, a.rival_m + l0, a.rival_x + l0, a.rival_state + l0, a.z_m + b, a.z_x + b};
    two_fill<K, kSlots ? TA_FORCED_FIELDS : 1, PostCells>(ln, lane, etab, &red);
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

template <bool kSlots>
hipError_t launch_variants(const PostArgs& a, void* stream) {
    return forced_launch_variants(a.variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_post_kernel<decltype(kc)::value, kSlots>), dim3((unsigned)a.nlines), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
}

}  // namespace

extern "C" int64_t ta_forced_posterior_workspace_bytes(int32_t T, int32_t L) {
    return forced_ws_guard(T, L) ? two_fill_ws_bytes<PostCells>(L) : -1;
}

extern "C" int ta_forced_posterior(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                                   const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, const int32_t* t_query,
                                   int32_t nlines, int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host,
                                   const int32_t* L_host, void* workspace, int64_t workspace_bytes, double* own_m,
                                   int32_t* own_x, double* rival_m, int32_t* rival_x, int32_t* rival_state, double* z_m,
                                   int32_t* z_x, int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr, nlines == 0,
                             !probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !t_query || !T_host ||
                                 !L_host || !workspace || !own_m || !own_x || !rival_m || !rival_x || !rival_state || !z_m ||
                                 !z_x || !status,
                             workspace, &go);
    if (!go) return rc;
    int variants;
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, [](int, int l) { return two_fill_ws_bytes<PostCells>(l); },
                            "ta_forced_posterior_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const PostArgs a{{probs, row_off, T, labels, lab_off, L, ws_off, t_query, nlines, no, variants, rows, nlabels,
                      static_cast<unsigned char*>(workspace), workspace_bytes, status, nullptr, nullptr, nullptr, nullptr,
                      nullptr, 0, 0}, own_m, own_x, rival_m, rival_x, rival_state, z_m, z_x};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_post_kernel launch");
    return TA_OK;
}

extern "C" int64_t ta_forced_posterior_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max) {
    return two_fill_slots_ws_bytes<PostCells>(label_cap, Lcap_max);
}

extern "C" int ta_forced_posterior_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all,
                                         const int32_t* Lcap, const int32_t* acc_line, const int32_t* L,
                                         const int64_t* lab_off, const int32_t* labels, const int64_t* count,
                                         const int32_t* align_status, const int32_t* frames, int32_t nlines_all,
                                         int32_t nslots, int32_t no, int64_t rows, int64_t label_cap,
                                         const int32_t* T_all_host, const int32_t* Lcap_host, void* workspace,
                                         int64_t workspace_bytes, double* own_m, int32_t* own_x, double* rival_m,
                                         int32_t* rival_x, int32_t* rival_state, double* z_m, int32_t* z_x, int32_t* status,
                                         void* stream) {
    bool go;
    int rc = forced_preamble(nlines_all < 0 || nslots < 0 || rows < 0 || label_cap < 0 || workspace_bytes < 0, no,
                             nslots > nlines_all ? "more slots than lines" : nullptr, nlines_all == 0 || nslots == 0,
                             !probs || !row_off_all || !T_all || !Lcap || !acc_line || !L || !lab_off || !labels || !count ||
                                 !align_status || !frames || !T_all_host || !Lcap_host || !workspace || !own_m || !own_x ||
                                 !rival_m || !rival_x || !rival_state || !z_m || !z_x || !status,
                             workspace, &go);
    if (!go) return rc;
    int kmax;
    rc = forced_check_slots(T_all_host, Lcap_host, nlines_all, rows, label_cap, workspace_bytes,
                            ta_forced_posterior_lines_workspace_bytes, "ta_forced_posterior_lines_workspace_bytes", &kmax);
    if (rc != TA_OK || kmax == 0) return rc;           // (kmax 0: no line can take a slot)
    const int variants = variants_up_to(kmax);
    const PostArgs a{{probs, row_off_all, T_all, labels, lab_off, L, nullptr, nullptr, nslots, no, variants, rows, label_cap,
                      static_cast<unsigned char*>(workspace), workspace_bytes, status, acc_line, count, Lcap, align_status,
                      frames, nlines_all, kmax}, own_m, own_x, rival_m, rival_x, rival_state, z_m, z_x};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_post_kernel launch (slots)");
    return TA_OK;
}
