// ta_forced_conf.hip -- per-character confidence of a forced alignment from max-marginals.
// For a query frame t per character i of a line's text: the total of the best CTC path that spends frame t in the
// character's own state 2 i + 1, minus the total of the best path that spends it in any other state, and that state.
// Integers only, on the lattice, the emission score and the skip rule of DESIGN.md section 14.7; the checker of record is
// tests/forced_conf_ref.py.  Two entries, one kernel body: ta_forced_confidence (a line list from the host, a query array)
// and ta_forced_confidence_lines (the packed slots ta_harvest_pack left on the device, the queries the t_peak
// ta_forced_align_lines left in its frames: kSlots).
//
// forced_conf_kernel<K, kSlots>, one wave per line, the layout of forced_common.h: lane l holds the K consecutive states
// l K .. l K + K - 1 as int64 registers.  ONE wave runs both fills, one after the other -- the control structure is
// two_fill's and the kernel's way to its line two_fill_prologue's (forced_two_fill.h, shared with ta_forced_post.hip); the
// arithmetic is ConfCells below:
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
#include "forced_two_fill.h"

namespace {

constexpr long long kReach = -(1ll << 49);

struct ConfArgs : TwoFillArgs { int64_t* confidence; int32_t* rival; };

struct ConfLine : TwoFillLine {
    int64_t* confidence;       // the line's rows of the two outputs
    int32_t* rival;
};

// two_fill's arithmetic: max-plus on int64 scores; a forward row is 64 K int64 per character
struct ConfCells {
    using V = long long;
    using E = int;
    using Line = ConfLine;
    using Red = long long;     // [73]: 64 lanes' candidates, 8 partial maxima, the own state's value
    using Cand = long long;    // value and state packed: the largest key is the largest value at the smallest state
    __device__ static __forceinline__ void put(Red* red, int i, Cand c) { red[i] = c; }
    __device__ static __forceinline__ Cand get(const Red* red, int i) { return red[i]; }
    __device__ static __forceinline__ bool better(Cand a, Cand b) { return a > b; }
    static constexpr int64_t kRowBytes = 512;
    __device__ static __forceinline__ V zero() { return kNeg; }
    __device__ static __forceinline__ V one() { return 0; }
    __device__ static __forceinline__ E emit(float p) { return emission_q(p); }
    __device__ static __forceinline__ V first(E q) { return q; }
    __device__ static __forceinline__ V left(V v) { return from_left(v, kNeg); }
    template <int K> __device__ static __forceinline__ void chunk_begin(V (&)[K]) {}
    template <int K> __device__ static __forceinline__ void forward_done(const Line&, int, int, const V (&)[K], Red*) {}

    template <int K>
    __device__ static __forceinline__ void forward(V (&v)[K], V left, unsigned skip, const int (&lab)[K / 2], const E* q) {
        const int qb = q[0];
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {             // forced_step<K, false> without its moves, spelled out: as a call
            long long best = v[k];                     // K = 8 loses a wave of occupancy
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

    template <int K>
    __device__ static __forceinline__ void backward(V (&v)[K], unsigned skipf, const int (&lab)[K / 2], const E* q) {
        const int qb = q[0];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += (k & 1) ? q[lab[k >> 1]] : qb;
        const long long r0 = from_right(v[0], kNeg), r1 = from_right(v[1], kNeg);
#pragma unroll
        for (int k = 0; k < K; ++k) {                  // upwards: v[k + 1] and v[k + 2] still carry frame t
            long long best = v[k];
            const long long adv = k + 1 < K ? v[(k + 1) % K] : r0;
            if (adv > best) best = adv;
            if (k & 1) {
                const long long sk = k + 2 < K ? v[(k + 2) % K] : r1;
                if (((skipf >> (k >> 1)) & 1u) && sk > best) best = sk;
            }
            v[k] = best;
        }
    }

    template <int K>
    __device__ static __forceinline__ void store_row(const Line& ln, int cur, int lane, const V (&v)[K]) {
        long long* row = reinterpret_cast<long long*>(ln.fwd) + (int64_t)cur * (64 * K);
#pragma unroll
        for (int k = 0; k < K; ++k) row[k * 64 + lane] = v[k];
    }

    // character `cur` at the frame v holds B of
    template <int K>
    __device__ static __forceinline__ void combine(const Line& ln, int cur, int lane, int S, const V (&v)[K], Red* red) {
        const long long* row = reinterpret_cast<const long long*>(ln.fwd) + (int64_t)cur * (64 * K);
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
        const long long m = two_fill_best<ConfCells>(red, lane, key);
        if (lane == 0) {
            ln.confidence[cur] = red[72] - (m >> 11);
            ln.rival[cur] = 2047 - (int)(m & 2047);
        }
        wave_lds_sync();                               // red is free again
    }
};

// the blocks, their lines and their statuses: two_fill_prologue
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_conf_kernel(ConfArgs a) {
    __shared__ int qtab[2 * kChunk * kMaxNo];          // two chunks of emission scores (8 KiB)
    __shared__ long long red[73];
    const int b = blockIdx.x, lane = threadIdx.x;
    TwoFillLine line;
    int64_t l0;
    if (!two_fill_prologue<K, kSlots, ConfCells>(a, b, lane, &line, &l0)) return;
    const ConfLine ln{line, a.confidence + l0, a.rival + l0};
    two_fill<K, kSlots ? TA_FORCED_FIELDS : 1, ConfCells>(ln, lane, qtab, red);
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
    return forced_ws_guard(T, L) ? two_fill_ws_bytes<ConfCells>(L) : -1;
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
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, [](int, int l) { return two_fill_ws_bytes<ConfCells>(l); },
                            "ta_forced_confidence_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const ConfArgs a{{probs, row_off, T, labels, lab_off, L, ws_off, t_query, nlines, no, variants, rows, nlabels,
                      static_cast<unsigned char*>(workspace), workspace_bytes, status, nullptr, nullptr, nullptr, nullptr,
                      nullptr, 0, 0}, confidence, rival};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_conf_kernel launch");
    return TA_OK;
}

extern "C" int64_t ta_forced_confidence_lines_workspace_bytes(int64_t label_cap, int32_t Lcap_max) {
    return two_fill_slots_ws_bytes<ConfCells>(label_cap, Lcap_max);
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
    const ConfArgs a{{probs, row_off_all, T_all, labels, lab_off, L, nullptr, nullptr, nslots, no, variants, rows, label_cap,
                      static_cast<unsigned char*>(workspace), workspace_bytes, status, acc_line, count, Lcap, align_status,
                      frames, nlines_all, kmax}, confidence, rival};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_conf_kernel launch (slots)");
    return TA_OK;
}
