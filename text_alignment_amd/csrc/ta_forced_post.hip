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
// holds the K consecutive states l K .. l K + K - 1 as (double, int) registers.  ONE wave runs both fills:
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
#include "forced_common.h"

namespace {

constexpr int kZeroX = -(1 << 29);                     // zero's exponent: two of them still add inside an int
constexpr int kShift = 256;
constexpr int kKeyNone = INT32_MIN;                    // a lane without a candidate
constexpr int kKeyZero = INT32_MIN + 1;                // a candidate whose g is zero: below every real exponent

struct PostArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off; const int32_t* t_query;
    int32_t nlines, no, variants; int64_t rows, nlabels;     // variants: a bit per K that this call launches
    unsigned char* ws; int64_t ws_bytes;
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state;
    double* z_m; int32_t* z_x; int32_t* status;
    // ta_forced_posterior_lines alone: block k is a packed slot, its line acc_line[k] of the chunk's nlines_all lines
    // (row_off, T and Lcap per CHUNK line; labels, lab_off, L per slot), count[0] the slots that are filled, align_status
    // what ta_forced_align_lines gave the slot, frames where it left the slot's t_peak; kmax the widest variant launched
    const int32_t* acc_line; const int64_t* count; const int32_t* Lcap; const int32_t* align_status; const int32_t* frames;
    int32_t nlines_all, kmax;
};

// the piece of the workspace for a line of L characters: per character a forward row of 64 K doubles and 64 K exponents
__host__ __device__ inline int64_t post_ws_bytes(int L) { return 768 * (int64_t)forced_k(2 * L + 1) * L; }

struct Val { double m; int x; };                       // m 2^x, m >= 0

__device__ __forceinline__ Val add(Val a, Val b) {
    const int x = a.x > b.x ? a.x : b.x;
    const int da = a.x - x > -kShift ? a.x - x : -kShift, db = b.x - x > -kShift ? b.x - x : -kShift;
    return Val{ldexp(a.m, da) + ldexp(b.m, db), x};
}
__device__ __forceinline__ Val normal(Val a) {         // m in [0.5, 1); zero keeps kZeroX (frexp gives it exponent 0)
    int e;
    const double m = frexp(a.m, &e);
    return Val{m, a.x + e};
}
__device__ __forceinline__ long long bits_of(double d) { long long u; __builtin_memcpy(&u, &d, 8); return u; }
__device__ __forceinline__ double double_of(long long u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
__device__ __forceinline__ Val left_of(Val v) {        // lane l takes lane l - 1's, lane 0 zero
    return Val{double_of(from_left(bits_of(v.m), 0)), __builtin_amdgcn_update_dpp(kZeroX, v.x, 0x138, 0xf, 0xf, false)};
}
__device__ __forceinline__ Val right_of(Val v) {       // lane l takes lane l + 1's, lane 63 zero
    return Val{double_of(from_right(bits_of(v.m), 0)), __builtin_amdgcn_update_dpp(kZeroX, v.x, 0x130, 0xf, 0xf, false)};
}
__device__ __forceinline__ float emission_f(float p) {
    const float a = p > 0x1p-17f ? p : 0x1p-17f;       // emission_q's two comparisons: NaN, 0 and negatives give the floor
    return a < 1.0f ? a : 1.0f;
}

struct PostLine {
    const float* P;            // the line's first probability row
    const int32_t* cs;         // its labels
    const int32_t* tq;         // its query frames, kStride words apart
    unsigned char* fwd;        // its piece of the workspace: row i = a[tq[i]]
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state;     // its rows of the outputs
    double* z_m; int32_t* z_x; // its entry of the two per line
    int T, L, no;
};

// the LDS of a combine: 64 lanes' candidates, 8 partial bests, the own state's value ([72]); Z's two terms pass through too
struct PostRed { double m[73]; int x[73]; int s[73]; };

__device__ __forceinline__ bool better(int x, double m, int s, int bx, double bm, int bs) {
    return x > bx || (x == bx && (m > bm || (m == bm && s < bs)));
}

template <int K, int kStride>
__device__ __forceinline__ void post_line(const PostLine& ln, int lane, float* etab, PostRed& red) {
    constexpr int H = K / 2;                           // labels per lane
    const int T = ln.T, L = ln.L, no = ln.no, S = 2 * L + 1;
    int lab[H];
    unsigned skipf;
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab, &skipf);
    const Val zero{0.0, kZeroX};
    Val v[K];
    Feed<float> feed(etab, no, lane);                  // the emissions stay float32
    const int nchunks = (T + kChunk - 1) / kChunk;
    auto renormalise = [&]() {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = normal(v[k]);
    };
    auto row_m = [&](int i) { return reinterpret_cast<double*>(ln.fwd + (int64_t)i * (768 * K)); };
    auto row_x = [&](int i) { return reinterpret_cast<int*>(ln.fwd + (int64_t)i * (768 * K) + 512 * K); };

    // ---- forward fill; the row of every query frame is kept -------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = zero;
    auto query = [&](int i) { return i >= 0 && i < L ? __builtin_amdgcn_readfirstlane(ln.tq[(int64_t)i * kStride]) : -1; };
    int cur = 0, want = query(0);                      // wave-uniform: the next character whose query is still ahead
    feed.prefetch(ln.P, T, 0);
    for (int c = 0; c < nchunks; ++c) {
        const float* ebuf = feed.publish(c, emission_f);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        renormalise();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const float* e = ebuf + (t - t0) * no;
            const double eb = (double)e[0];
            if (t == 0) {
                if (lane == 0) { v[0] = Val{eb, 0}; v[1] = Val{(double)e[lab[0]], 0}; }
            } else {
                const Val left = left_of(v[K - 1]);
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {     // downwards: v[k - 1] and v[k - 2] are still the old row's
                    Val y = add(v[k], k >= 1 ? v[k - 1] : left);
                    if (k & 1) {
                        const Val sk = k >= 2 ? v[k - 2] : left;
                        y = add(y, ((skip >> (k >> 1)) & 1u) ? sk : zero);
                        v[k] = Val{y.m * (double)e[lab[k >> 1]], y.x};
                    } else {
                        v[k] = Val{y.m * eb, y.x};
                    }
                }
            }
            while (want == t) {
                double* rm = row_m(cur);
                int* rx = row_x(cur);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    rm[k * 64 + lane] = v[k].m;
                    rx[k * 64 + lane] = v[k].x;
                }
                ++cur;
                want = query(cur);
            }
        }
    }
    // Z = a[S - 1] + a[S - 2]
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = lane * K + k;
        if (s == S - 1) { red.m[0] = v[k].m; red.x[0] = v[k].x; }
        if (s == S - 2) { red.m[1] = v[k].m; red.x[1] = v[k].x; }
    }
    wave_lds_sync();
    if (lane == 0) {
        const Val z = normal(add(Val{red.m[0], red.x[0]}, Val{red.m[1], red.x[1]}));
        *ln.z_m = z.m;
        *ln.z_x = z.m == 0.0 ? 0 : z.x;
    }
    wave_lds_sync();                                   // red is free again

    // ---- backward fill, and the combine at every query frame -----------------------------------------------------------
    cur = L - 1;
    want = query(cur);
    auto combine = [&]() {                             // character `cur` at the frame v holds b of
        const double* rm = row_m(cur);
        const int* rx = row_x(cur);
        const int own = 2 * cur + 1;
        int bx = kKeyNone, bs = 0;
        double bm = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane * K + k;
            // what this very lane stored in the forward fill
            const Val g = normal(Val{rm[k * 64 + lane] * v[k].m, rx[k * 64 + lane] + v[k].x});
            const int gx = g.m == 0.0 ? kKeyZero : g.x;
            if (s == own) { red.m[72] = g.m; red.x[72] = gx; }
            else if (s < S && better(gx, g.m, s, bx, bm, bs)) { bx = gx; bm = g.m; bs = s; }
        }
        red.m[lane] = bm; red.x[lane] = bx; red.s[lane] = bs;
        wave_lds_sync();
        if (lane < 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int at = 8 * lane + j;
                if (j == 0 || better(red.x[at], red.m[at], red.s[at], bx, bm, bs)) { bx = red.x[at]; bm = red.m[at]; bs = red.s[at]; }
            }
            red.m[64 + lane] = bm; red.x[64 + lane] = bx; red.s[64 + lane] = bs;
        }
        wave_lds_sync();
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int at = 64 + j;
                if (j == 0 || better(red.x[at], red.m[at], red.s[at], bx, bm, bs)) { bx = red.x[at]; bm = red.m[at]; bs = red.s[at]; }
            }
            ln.own_m[cur] = red.m[72];
            ln.own_x[cur] = red.x[72] == kKeyZero ? 0 : red.x[72];
            ln.rival_m[cur] = bm;
            ln.rival_x[cur] = bx == kKeyZero ? 0 : bx;
            ln.rival_state[cur] = bs;
        }
        wave_lds_sync();                               // red is free again
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = lane * K + k;
        v[k] = s == S - 1 || s == S - 2 ? Val{1.0, 0} : zero;
    }
    while (want == T - 1) {
        combine();
        --cur;
        want = query(cur);
    }
    feed.prefetch(ln.P, T, nchunks - 1);
    for (int c = nchunks - 1; c >= 0; --c) {
        const float* ebuf = feed.publish(c, emission_f);
        feed.prefetch(ln.P, T, c - 1);
        wave_lds_sync();
        renormalise();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t1 - 1; t >= t0 && t >= 1; --t) {  // the emission of frame t takes b[t] to b[t - 1]
            const float* e = ebuf + (t - t0) * no;
            const double eb = (double)e[0];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k].m *= (k & 1) ? (double)e[lab[k >> 1]] : eb;
            const Val r0 = right_of(v[0]), r1 = right_of(v[1]);
#pragma unroll
            for (int k = 0; k < K; ++k) {              // upwards: v[k + 1] and v[k + 2] still carry frame t
                Val y = add(v[k], k + 1 < K ? v[(k + 1) % K] : r0);
                if (k & 1) {
                    const Val sk = k + 2 < K ? v[(k + 2) % K] : r1;
                    y = add(y, ((skipf >> (k >> 1)) & 1u) ? sk : zero);
                }
                v[k] = y;
            }
            while (want == t - 1) {
                combine();
                --cur;
                want = query(cur);
            }
        }
    }
}

// One launch per variant the host's copies call for, each over all lines, as forced_conf_kernel: a line belongs to the
// launch of ITS K (from the device's L) and the others leave at once; a line that fails the checks, or whose K no launch
// of this call covers, is refused by every launch alike.
// kSlots (ta_forced_posterior_lines): the blocks are the packed slots ta_harvest_pack left on the device, behind
// ta_forced_align_lines, exactly as forced_conf_kernel takes them.  A slot behind count[0] -- or any slot of a call whose
// count[0] is negative -- leaves before it has read or written anything else; a filled slot the aligner did not give
// TA_FORCED_OK gets TA_FORCED_SKIPPED and nothing of it is read; any other finds its line through acc_line, is held to
// that line's cap on top of the checks below, takes its queries from its own rows of frames (t_peak, TA_FORCED_FIELDS
// words apart) and its piece of the workspace from lab_off: 768 kmax lab_off[k] bytes in, which no other slot's piece
// reaches since the slots' labels do not overlap.  z_m, z_x and status are per SLOT.  All of this is over before
// post_line's registers are live.
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_post_kernel(PostArgs a) {
    constexpr int kStride = kSlots ? TA_FORCED_FIELDS : 1;
    __shared__ float etab[2 * kChunk * kMaxNo];        // two chunks of emissions (8 KiB)
    __shared__ PostRed red;
    const int b = blockIdx.x, lane = threadIdx.x;
    int q = b;                                         // the line whose rows and timesteps block b takes
    if (kSlots) {
        if (!slot_filled(a.count, b)) return;
        if (__builtin_amdgcn_readfirstlane(a.align_status[b]) != TA_FORCED_OK) {
            if (lane == 0) a.status[b] = TA_FORCED_SKIPPED;
            return;
        }
        q = slot_line(a.acc_line, a.nlines_all, b);
        if (q < 0) {
            if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
            return;
        }
    }
    const int T = __builtin_amdgcn_readfirstlane(a.T[q]), L = __builtin_amdgcn_readfirstlane(a.L[b]);
    const int64_t r0 = a.row_off[q], l0 = a.lab_off[b];
    if (kSlots && L > __builtin_amdgcn_readfirstlane(a.Lcap[q])) {     // beyond what the host chose the variants for
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    // (slots: the product stays far inside 64 bits once l0 is known to lie inside the labels)
    const int64_t w0 = !kSlots ? a.ws_off[b] : l0 >= 0 && l0 <= a.nlabels ? 768 * (int64_t)a.kmax * l0 : -1;
    if (!line_ok(a, T, L, r0, l0, w0, [&] { return post_ws_bytes(L); })) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (forced_k(2 * L + 1) != K) return;              // wave-uniform
    const int32_t* cs = a.labels + l0;
    const int32_t* tq = kSlots ? a.frames + TA_FORCED_FIELDS * l0 + 2 : a.t_query + l0;
    if (!labels_ok(cs, L, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    if (!queries_ok<kStride>(tq, L, T, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_QUERY;
        return;
    }
    const PostLine ln{a.probs + r0 * a.no, cs, tq, a.ws + w0, a.own_m + l0, a.own_x + l0, a.rival_m + l0, a.rival_x + l0,
                      a.rival_state + l0, a.z_m + b, a.z_x + b, T, L, a.no};
    post_line<K, kStride>(ln, lane, etab, red);
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
    return forced_ws_guard(T, L) ? post_ws_bytes(L) : -1;
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
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, [](int, int l) { return post_ws_bytes(l); },
                            "ta_forced_posterior_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const PostArgs a{probs, row_off, T, labels, lab_off, L, ws_off, t_query, nlines, no, variants, rows, nlabels,
                     static_cast<unsigned char*>(workspace), workspace_bytes, own_m, own_x, rival_m, rival_x, rival_state,
                     z_m, z_x, status, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_post_kernel launch");
    return TA_OK;
}

extern "C" int64_t ta_forced_posterior_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max) {
    if (label_cap < 0 || label_cap > INT64_MAX / (768 * 32) || Lcap_max < 0 || Lcap_max > TA_FORCED_MAX_TARGET) return -1;
    if (Lcap_max == 0) return 0;
    return 768 * (int64_t)forced_k(2 * Lcap_max + 1) * label_cap;
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
    const PostArgs a{probs, row_off_all, T_all, labels, lab_off, L, nullptr, nullptr, nslots, no, variants, rows, label_cap,
                     static_cast<unsigned char*>(workspace), workspace_bytes, own_m, own_x, rival_m, rival_x, rival_state,
                     z_m, z_x, status, acc_line, count, Lcap, align_status, frames, nlines_all, kmax};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_post_kernel launch (slots)");
    return TA_OK;
}
