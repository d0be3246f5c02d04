// ta_forced_conf.hip -- per-character confidence of a forced alignment from max-marginals.
// For a query frame t per character i of a line's text: the total of the best CTC path that spends frame t in the
// character's own state 2 i + 1, minus the total of the best path that spends it in any other state, and that state.
// Integers only, on the lattice, the emission score and the skip rule of DESIGN.md section 14.7; the checker of record is
// tests/forced_conf_ref.py.  Two entries, one kernel body: ta_forced_confidence (a line list from the host, a query array)
// and ta_forced_confidence_lines (the packed slots ta_harvest_pack left on the device, the queries the t_peak
// ta_forced_align_lines left in its frames: kSlots).
//
// forced_conf_kernel<K, kSlots>, one wave per line, the layout of forced_common.h: lane l holds the K consecutive states
// l K .. l K + K - 1 as int64 registers.  ONE wave runs both fills, one after the other:
//   forward   A[t][s], the aligner's fill without its moves (forced_step, spelled out here without them): only the left
//             lane's last value crosses a lane boundary (from_left, wave_shr:1).
//             The row of every query frame goes to the workspace, row i for character i (queries do not decrease, so
//             one cursor meets them in order), K coalesced 8-byte stores per lane.
//   backward  B[t][s] = max over the successors s, s + 1, s + 2 (the skip rule read from the other side) of B[t + 1] plus
//             the emission at t + 1: a pure max, walked from the last chunk of emission scores to the first.  Across a lane
//             boundary the RIGHT lane's first two values are needed (wave_shl:1).  At a query frame the character's
//             forward row comes back, G = A + B where both are reachable (else exactly -2^50), every lane keeps the best
//             of its states but the character's own, and 64 candidates meet in LDS: value and state packed into one
//             int64 so that the largest key is the largest value at the smallest state.  That happens L times per line,
//             not T times.
// Neither fill stores moves, and there is no barrier in a fill (wave_lds_sync).  Padding states (s >= S) and unreachable
// ones start at -2^50 and only ever go down, so they never reach a reachable state's max and read as unreachable.
// Every bound is re-checked on the line's own device numbers before anything is read through it; a refused line gets a
// status and touches nothing else.
#include "forced_common.h"

namespace {

constexpr long long kReach = -(1ll << 49);

struct ConfArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off; const int32_t* t_query;
    int32_t nlines, no, variants; int64_t rows, nlabels;     // variants: a bit per K that this call launches
    unsigned char* ws; int64_t ws_bytes;
    int64_t* confidence; int32_t* rival; int32_t* status;
    // ta_forced_confidence_lines alone: block k is a packed slot, its line acc_line[k] of the chunk's nlines_all lines
    // (row_off, T and Lcap per CHUNK line; labels, lab_off, L per slot), count[0] the slots that are filled, align_status
    // what ta_forced_align_lines gave the slot, frames where it left the slot's t_peak; kmax the widest variant launched
    const int32_t* acc_line; const int64_t* count; const int32_t* Lcap; const int32_t* align_status; const int32_t* frames;
    int32_t nlines_all, kmax;
};

// the piece of the workspace for a line of L characters: a forward row of 64 K int64 per character
__host__ __device__ inline int64_t conf_ws_bytes(int L) { return 512 * (int64_t)forced_k(2 * L + 1) * L; }

struct ConfLine {
    const float* P;            // the line's first probability row
    const int32_t* cs;         // its labels
    const int32_t* tq;         // its query frames, kStride words apart
    long long* fwd;            // its piece of the workspace: row i = A[tq[i]]
    int64_t* confidence;       // its rows of the two outputs
    int32_t* rival;
    int T, L, no;
};

template <int K, int kStride>
__device__ __forceinline__ void conf_line(const ConfLine& ln, int lane, int* qtab, long long* red) {
    constexpr int H = K / 2;                           // labels per lane
    const int T = ln.T, L = ln.L, no = ln.no, S = 2 * L + 1;
    int lab[H];
    unsigned skipf;
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab, &skipf);
    long long v[K];
    Feed<int> feed(qtab, no, lane);
    const int nchunks = (T + kChunk - 1) / kChunk;

    // ---- forward fill: the aligner's, without moves; the row of every query frame is kept ------------------------------
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;
    auto query = [&](int i) { return i >= 0 && i < L ? __builtin_amdgcn_readfirstlane(ln.tq[(int64_t)i * kStride]) : -1; };
    int cur = 0, want = query(0);                      // wave-uniform: the next character whose query is still ahead
    feed.prefetch(ln.P, T, 0);
    for (int c = 0; c < nchunks; ++c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
            if (t == 0) {
                if (lane == 0) { v[0] = qb; v[1] = q[lab[0]]; }
            } else {
                const long long left = from_left(v[K - 1], kNeg);
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {     // forced_step<K, false> without its moves, spelled out: as a call
                    long long best = v[k];             // K = 8 loses a wave of occupancy
                    const long long adv = k >= 1 ? v[k - 1] : left;
                    if (adv > best) best = adv;
                    if (k & 1) {
                        const long long sk = k >= 2 ? v[k - 2] : left;
                        if (((skip >> (k >> 1)) & 1u) && sk > best) best = sk;
                        v[k] = best + q[lab[k >> 1]];
                    } else {
                        v[k] = best + qb;
                    }
                }
            }
            while (want == t) {
                long long* row = ln.fwd + (int64_t)cur * (64 * K);
#pragma unroll
                for (int k = 0; k < K; ++k) row[k * 64 + lane] = v[k];
                ++cur;
                want = query(cur);
            }
        }
    }

    // ---- backward fill, and the combine at every query frame -----------------------------------------------------------
    cur = L - 1;
    want = query(cur);
    auto combine = [&]() {                             // character `cur` at the frame v holds B of
        const long long* row = ln.fwd + (int64_t)cur * (64 * K);
        const int own = 2 * cur + 1;
        long long key = kNeg * 2048;                   // below every candidate's
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane * K + k;
            const long long a = row[k * 64 + lane];                // what this very lane stored in the forward fill
            const long long g = a > kReach && v[k] > kReach ? a + v[k] : kNeg;
            const long long cand = g * 2048 + (2047 - s);          // the larger value first, then the smaller state
            if (s == own) red[72] = g;
            else if (s < S && cand > key) key = cand;
        }
        red[lane] = key;
        wave_lds_sync();
        if (lane < 8) {
            long long m = red[8 * lane];
#pragma unroll
            for (int j = 1; j < 8; ++j) m = red[8 * lane + j] > m ? red[8 * lane + j] : m;
            red[64 + lane] = m;
        }
        wave_lds_sync();
        if (lane == 0) {
            long long m = red[64];
#pragma unroll
            for (int j = 1; j < 8; ++j) m = red[64 + j] > m ? red[64 + j] : m;
            ln.confidence[cur] = red[72] - (m >> 11);
            ln.rival[cur] = 2047 - (int)(m & 2047);
        }
        wave_lds_sync();                               // red is free again
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = lane * K + k;
        v[k] = s == S - 1 || s == S - 2 ? 0 : kNeg;
    }
    while (want == T - 1) {
        combine();
        --cur;
        want = query(cur);
    }
    feed.prefetch(ln.P, T, nchunks - 1);
    for (int c = nchunks - 1; c >= 0; --c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c - 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t1 - 1; t >= t0 && t >= 1; --t) {  // the emission of frame t takes B[t] to B[t - 1]
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] += (k & 1) ? q[lab[k >> 1]] : qb;
            const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
            for (int k = 0; k < K; ++k) {              // upwards: v[k + 1] and v[k + 2] still carry frame t
                long long best = v[k];
                const long long adv = k + 1 < K ? v[(k + 1) % K] : r0;
                if (adv > best) best = adv;
                if (k & 1) {
                    const long long sk = k + 2 < K ? v[(k + 2) % K] : r1;
                    if (((skipf >> (k >> 1)) & 1u) && sk > best) best = sk;
                }
                v[k] = best;
            }
            while (want == t - 1) {
                combine();
                --cur;
                want = query(cur);
            }
        }
    }
}

// One launch per variant the host's copies call for, each over all lines, as forced_align_kernel: a line belongs to the
// launch of ITS K (from the device's L) and the others leave at once; a line that fails the checks, or whose K no launch
// of this call covers, is refused by every launch alike.
// kSlots (ta_forced_confidence_lines): the blocks are the packed slots ta_harvest_pack left on the device, behind
// ta_forced_align_lines.  A slot behind count[0] -- or any slot of a call whose count[0] is negative -- leaves before it has
// read or written anything else; a filled slot the aligner did not give TA_FORCED_OK gets TA_FORCED_SKIPPED and nothing of
// it is read; any other finds its line through acc_line, is held to that line's cap on top of the checks below, takes
// its queries from its own rows of frames (t_peak, TA_FORCED_FIELDS words apart) and its piece of the workspace from
// lab_off: 512 kmax lab_off[k] bytes in, which no other slot's piece reaches since the slots' labels do not overlap.
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_conf_kernel(ConfArgs a) {
    constexpr int kStride = kSlots ? TA_FORCED_FIELDS : 1;
    __shared__ int qtab[2 * kChunk * kMaxNo];          // two chunks of emission scores (8 KiB)
    __shared__ long long red[73];                      // 64 lanes' candidates, 8 partial maxima, the own state's value
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
    const int64_t w0 = !kSlots ? a.ws_off[b] : l0 >= 0 && l0 <= a.nlabels ? 512 * (int64_t)a.kmax * l0 : -1;
    if (!line_ok(a, T, L, r0, l0, w0, [&] { return conf_ws_bytes(L); })) {
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
    const ConfLine ln{a.probs + r0 * a.no, cs, tq, reinterpret_cast<long long*>(a.ws + w0), a.confidence + l0, a.rival + l0,
                      T, L, a.no};
    conf_line<K, kStride>(ln, lane, qtab, red);
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

template <bool kSlots>
hipError_t launch_variants(const ConfArgs& a, void* stream) {
    return forced_launch_variants(a.variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_conf_kernel<decltype(kc)::value, kSlots>), dim3((unsigned)a.nlines), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
}

}  // namespace

extern "C" int64_t ta_forced_confidence_workspace_bytes(int32_t T, int32_t L) {
    return forced_ws_guard(T, L) ? conf_ws_bytes(L) : -1;
}

extern "C" int ta_forced_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                                    const int64_t* lab_off, const int32_t* L, const int64_t* ws_off,
                                    const int32_t* t_query, int32_t nlines, int32_t no, int64_t rows, int64_t nlabels,
                                    const int32_t* T_host, const int32_t* L_host, void* workspace, int64_t workspace_bytes,
                                    int64_t* confidence, int32_t* rival, int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr, nlines == 0,
                             !probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !t_query || !T_host ||
                                 !L_host || !workspace || !confidence || !rival || !status,
                             workspace, &go);
    if (!go) return rc;
    int variants;
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, [](int, int l) { return conf_ws_bytes(l); },
                            "ta_forced_confidence_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const ConfArgs a{probs, row_off, T, labels, lab_off, L, ws_off, t_query, nlines, no, variants, rows, nlabels,
                     static_cast<unsigned char*>(workspace), workspace_bytes, confidence, rival, status,
                     nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_conf_kernel launch");
    return TA_OK;
}

extern "C" int64_t ta_forced_confidence_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max) {
    if (label_cap < 0 || label_cap > INT64_MAX / (512 * 32) || Lcap_max < 0 || Lcap_max > TA_FORCED_MAX_TARGET) return -1;
    if (Lcap_max == 0) return 0;
    return 512 * (int64_t)forced_k(2 * Lcap_max + 1) * label_cap;
}

extern "C" int ta_forced_confidence_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all,
                                          const int32_t* Lcap, const int32_t* acc_line, const int32_t* L,
                                          const int64_t* lab_off, const int32_t* labels, const int64_t* count,
                                          const int32_t* align_status, const int32_t* frames, int32_t nlines_all,
                                          int32_t nslots, int32_t no, int64_t rows, int64_t label_cap,
                                          const int32_t* T_all_host, const int32_t* Lcap_host, void* workspace,
                                          int64_t workspace_bytes, int64_t* confidence, int32_t* rival, int32_t* status,
                                          void* stream) {
    bool go;
    int rc = forced_preamble(nlines_all < 0 || nslots < 0 || rows < 0 || label_cap < 0 || workspace_bytes < 0, no,
                             nslots > nlines_all ? "more slots than lines" : nullptr, nlines_all == 0 || nslots == 0,
                             !probs || !row_off_all || !T_all || !Lcap || !acc_line || !L || !lab_off || !labels || !count ||
                                 !align_status || !frames || !T_all_host || !Lcap_host || !workspace || !confidence ||
                                 !rival || !status,
                             workspace, &go);
    if (!go) return rc;
    int kmax;
    rc = forced_check_slots(T_all_host, Lcap_host, nlines_all, rows, label_cap, workspace_bytes,
                            ta_forced_confidence_lines_workspace_bytes, "ta_forced_confidence_lines_workspace_bytes", &kmax);
    if (rc != TA_OK || kmax == 0) return rc;           // (kmax 0: no line can take a slot)
    const int variants = variants_up_to(kmax);
    const ConfArgs a{probs, row_off_all, T_all, labels, lab_off, L, nullptr, nullptr, nslots, no, variants, rows, label_cap,
                     static_cast<unsigned char*>(workspace), workspace_bytes, confidence, rival, status,
                     acc_line, count, Lcap, align_status, frames, nlines_all, kmax};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_conf_kernel launch (slots)");
    return TA_OK;
}
