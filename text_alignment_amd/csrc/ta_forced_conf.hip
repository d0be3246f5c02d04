// ta_forced_conf.hip -- per-character confidence of a forced alignment from max-marginals.
// For a query frame t per character i of a line's text: the total of the best CTC path that spends frame t in the
// character's own state 2 i + 1, minus the total of the best path that spends it in any other state, and that state.
// Integers only, on the lattice, the emission score and the skip rule of ta_forced.hip; the checker of record is
// tests/forced_conf_ref.py.  Two entries, one kernel body: ta_forced_confidence (a line list from the host, a query array)
// and ta_forced_confidence_lines (the packed slots ta_harvest_pack left on the device, the queries the t_peak
// ta_forced_align_lines left in its frames: kSlots).
//
// forced_conf_kernel<K, kSlots>, one wave per line, the layout of forced_common.h: lane l holds the K consecutive states
// l K .. l K + K - 1 as int64 registers.  ONE wave runs both fills, one after the other:
//   forward   A[t][s], the aligner's fill without its moves (the step is spelled out here once more: the aligner's packs
//             its moves inside the same loop): only the left lane's last value crosses a lane boundary (wave_shr:1).
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
    unsigned skip = 0;                                 // bit j: label j may be reached over the blank in front of it
    unsigned skipf = 0;                                // bit j: from label j the blank behind it may be skipped
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const int i = lane * H + j;
        lab[j] = i < L ? ln.cs[i] : 0;
        if (i >= 1 && i < L && ln.cs[i] != ln.cs[i - 1]) skip |= 1u << j;
        if (i + 1 < L && ln.cs[i + 1] != ln.cs[i]) skipf |= 1u << j;
    }
    long long v[K];
    float pf[kPf];
    const int nchunks = (T + kChunk - 1) / kChunk;
    auto prefetch = [&](int c) {                       // chunk c's probabilities; zeros for a chunk that does not exist
        const int t0 = c * kChunk;
        const int cnt = c < 0 ? 0 : (T - t0 < kChunk ? T - t0 : kChunk) * no;
        const float* src = ln.P + (int64_t)t0 * no;
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            const int idx = j * 64 + lane;
            pf[j] = idx < cnt ? src[idx] : 0.0f;
        }
    };
    auto publish = [&](int c) {                        // pf -> chunk c's buffer of emission scores
        int* qbuf = qtab + (c & 1) * (kChunk * kMaxNo);
#pragma unroll
        for (int j = 0; j < kPf; ++j) qbuf[j * 64 + lane] = emission_q(pf[j]);
        return qbuf;
    };

    // ---- forward fill: the aligner's, without moves; the row of every query frame is kept ------------------------------
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;
    auto query = [&](int i) { return i >= 0 && i < L ? __builtin_amdgcn_readfirstlane(ln.tq[(int64_t)i * kStride]) : -1; };
    int cur = 0, want = query(0);                      // wave-uniform: the next character whose query is still ahead
    prefetch(0);
    for (int c = 0; c < nchunks; ++c) {
        const int* qbuf = publish(c);
        prefetch(c + 1);
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
                for (int k = K - 1; k >= 0; --k) {     // downwards: v[k - 1] and v[k - 2] are still the old row's
                    long long best = v[k];
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
    prefetch(nchunks - 1);
    for (int c = nchunks - 1; c >= 0; --c) {
        const int* qbuf = publish(c);
        prefetch(c - 1);
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
        const int64_t filled = a.count[0];
        if (filled < 0 || b >= filled) return;
        if (__builtin_amdgcn_readfirstlane(a.align_status[b]) != TA_FORCED_OK) {
            if (lane == 0) a.status[b] = TA_FORCED_SKIPPED;
            return;
        }
        q = __builtin_amdgcn_readfirstlane(a.acc_line[b]);
        if (q < 0 || q >= a.nlines_all) {
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
    const bool ok = a.no >= 2 && a.no <= kMaxNo && T >= 1 && T <= TA_TRAIN_MAX_T && L >= 1 && L <= TA_FORCED_MAX_TARGET &&
                    2 * L + 1 <= T && r0 >= 0 && r0 + T <= a.rows && l0 >= 0 && l0 + L <= a.nlabels && w0 >= 0 &&
                    (w0 & 15) == 0 && w0 + conf_ws_bytes(L) <= a.ws_bytes &&
                    (a.variants & variant_bit(forced_k(2 * L + 1))) != 0;
    if (!ok) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (forced_k(2 * L + 1) != K) return;              // wave-uniform
    const int32_t* cs = a.labels + l0;
    const int32_t* tq = kSlots ? a.frames + TA_FORCED_FIELDS * l0 + 2 : a.t_query + l0;
    bool bad = false;
    for (int i = lane; i < L; i += 64) bad |= cs[i] < 1 || cs[i] >= a.no;
    if (__any(bad)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    for (int i = lane; i < L; i += 64) {
        const int t = tq[(int64_t)i * kStride];
        bad |= t < 0 || t >= T || (i >= 1 && t < tq[(int64_t)(i - 1) * kStride]);
    }
    if (__any(bad)) {
        if (lane == 0) a.status[b] = TA_FORCED_QUERY;
        return;
    }
    const ConfLine ln{a.probs + r0 * a.no, cs, tq, reinterpret_cast<long long*>(a.ws + w0), a.confidence + l0, a.rival + l0,
                      T, L, a.no};
    conf_line<K, kStride>(ln, lane, qtab, red);
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

template <int K, bool kSlots>
hipError_t launch(const ConfArgs& a, void* stream) {
    if (!(a.variants & variant_bit(K))) return hipSuccess;
    hipLaunchKernelGGL((forced_conf_kernel<K, kSlots>), dim3((unsigned)a.nlines), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

template <bool kSlots>
hipError_t launch_variants(const ConfArgs& a, void* stream) {
    hipError_t e = launch<2, kSlots>(a, stream);
    if (e == hipSuccess) e = launch<4, kSlots>(a, stream);
    if (e == hipSuccess) e = launch<8, kSlots>(a, stream);
    if (e == hipSuccess) e = launch<16, kSlots>(a, stream);
    if (e == hipSuccess) e = launch<32, kSlots>(a, stream);
    return e;
}

}  // namespace

extern "C" int64_t ta_forced_confidence_workspace_bytes(int32_t T, int32_t L) {
    if (T < 1 || T > TA_TRAIN_MAX_T || L < 1 || L > TA_FORCED_MAX_TARGET || 2 * (int64_t)L + 1 > T) return -1;
    return conf_ws_bytes(L);
}

extern "C" int ta_forced_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                                    const int64_t* lab_off, const int32_t* L, const int64_t* ws_off,
                                    const int32_t* t_query, int32_t nlines, int32_t no, int64_t rows, int64_t nlabels,
                                    const int32_t* T_host, const int32_t* L_host, void* workspace, int64_t workspace_bytes,
                                    int64_t* confidence, int32_t* rival, int32_t* status, void* stream) {
    if (nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative size");
    if (no < 2 || no > kMaxNo) return ta_fail(TA_EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES");
    if (nlines == 0) return TA_OK;
    if (!probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !t_query || !T_host || !L_host || !workspace ||
        !confidence || !rival || !status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return ta_fail(TA_EINVAL, "workspace not 16-byte aligned");
    int64_t need = 0, sum_t = 0, sum_l = 0;
    int variants = 0;
    for (int b = 0; b < nlines; ++b) {
        const int t = T_host[b], l = L_host[b];
        if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
        if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
        if (l < 1) return ta_fail(TA_EINVAL, "a line without text");
        if (l > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a text has more than TA_FORCED_MAX_TARGET characters");
        if (2 * (int64_t)l + 1 > t) return ta_fail(TA_EINVAL, "a text's 2 L + 1 states exceed its line's timesteps");
        need += conf_ws_bytes(l);
        variants |= variant_bit(forced_k(2 * l + 1));
        sum_t += t;
        sum_l += l;
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    if (sum_l > nlabels) return ta_fail(TA_EINVAL, "the lines' texts exceed nlabels");
    if (workspace_bytes < need)
        return ta_fail(TA_EINVAL, "workspace smaller than the lines' ta_forced_confidence_workspace_bytes");
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
    if (nlines_all < 0 || nslots < 0 || rows < 0 || label_cap < 0 || workspace_bytes < 0)
        return ta_fail(TA_EINVAL, "negative size");
    if (no < 2 || no > kMaxNo) return ta_fail(TA_EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES");
    if (nslots > nlines_all) return ta_fail(TA_EINVAL, "more slots than lines");
    if (nlines_all == 0 || nslots == 0) return TA_OK;
    if (!probs || !row_off_all || !T_all || !Lcap || !acc_line || !L || !lab_off || !labels || !count || !align_status ||
        !frames || !T_all_host || !Lcap_host || !workspace || !confidence || !rival || !status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return ta_fail(TA_EINVAL, "workspace not 16-byte aligned");
    int64_t sum_t = 0;
    int capmax = 0;
    for (int q = 0; q < nlines_all; ++q) {
        const int t = T_all_host[q], cap = Lcap_host[q];
        if (t < 1) return ta_fail(TA_EINVAL, "a line without timesteps");
        if (t > TA_TRAIN_MAX_T) return ta_fail(TA_ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps");
        if (cap < 0) return ta_fail(TA_EINVAL, "a negative cap");
        if (cap > TA_FORCED_MAX_TARGET) return ta_fail(TA_ELIMIT, "a cap above TA_FORCED_MAX_TARGET characters");
        sum_t += t;
        if (cap == 0) continue;                        // a line that can receive no text: no variant
        if (2 * (int64_t)cap + 1 > t) return ta_fail(TA_EINVAL, "a cap's 2 L + 1 states exceed its line's timesteps");
        capmax = cap > capmax ? cap : capmax;
    }
    if (sum_t > rows) return ta_fail(TA_EINVAL, "the lines' timesteps exceed rows");
    const int64_t need = ta_forced_confidence_lines_workspace_bytes(label_cap, capmax);
    if (need < 0) return ta_fail(TA_ELIMIT, "label_cap beyond what a workspace can be sized for");
    if (workspace_bytes < need)
        return ta_fail(TA_EINVAL, "workspace smaller than ta_forced_confidence_lines_workspace_bytes");
    if (capmax == 0) return TA_OK;                     // no line can take a slot
    const int kmax = forced_k(2 * capmax + 1);
    int variants = 0;                                  // a text within its cap may need any variant up to the cap's
    for (int k = 2; k <= kmax; k *= 2) variants |= variant_bit(k);
    const ConfArgs a{probs, row_off_all, T_all, labels, lab_off, L, nullptr, nullptr, nslots, no, variants, rows, label_cap,
                     static_cast<unsigned char*>(workspace), workspace_bytes, confidence, rival, status,
                     acc_line, count, Lcap, align_status, frames, nlines_all, kmax};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_conf_kernel launch (slots)");
    return TA_OK;
}
