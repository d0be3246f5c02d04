// ta_forced_omit_conf.hip -- per-character confidence on the lattice that may OMIT characters:
// max-marginals as ta_forced_conf.hip's, on ta_forced_omit.hip's lattice -- stay / advance / skip, far at `omit` per label
// state jumped, a path that may start and end in any state.  Integers only; the checker of record is
// tests/forced_omit_conf_ref.py.  A query is a (character, frame) pair: the total of the best path that spends the frame
// in the character's own state 2 i + 1, minus the total of the best path that spends it in any other state, and that state.
//
// forced_omit_conf_kernel<K>, one wave per line, the layout of forced_common.h: lane l holds the K consecutive states
// l K .. l K + K - 1 as int64 registers.  ONE wave runs both fills, one after the other, as forced_conf_kernel does; the
// loop is written out here (the queries are pairs, frame 0 seeds every lane, the end rule starts the backward fill), the
// reduction of a combine is two_fill_best's.
//   forward   A[t][s]: omit_seed / omit_step of forced_common.h without their moves and bit rows, spelled out (as in
//             ta_forced_omit.hip).  The far candidate comes from ONE wave-wide inclusive PREFIX max-scan per frame
//             (wave_max_scan).  Row j of the line's workspace piece takes A at q_frame[j] (frames do not decrease, so one
//             cursor meets them in order), K coalesced 8-byte stores per lane.
//   backward  B[T-1][s] = -omit (L - ceil(s / 2)), the end rule.  Per frame: w = B + the emission; c[x] = w[x] - omit
//             floor(x / 2); the lanes' maxima of c[] go through ONE wave-wide inclusive SUFFIX max-scan (wave_max_suffix_scan:
//             row_shl 1 / 2 / 4 / 8 inside a row of 16, the rows above joined by lane reads); shifted by a lane (from_right)
//             it is Sm at the right lane's state 0, and a second shift brings Sm at the right lane's state 2.  The states
//             are updated downwards carrying the in-lane suffix maximum: the far candidate of the states 2 j - 1 and 2 j of
//             a lane is Sm[2 j + 2] + omit ceil(s / 2).  At a query frame the forward row comes back, G = A + B (every state
//             is reachable: no test), every lane keeps the best of its states but the character's own, and 64 candidates
//             meet in LDS, value and state packed as ta_forced_conf.hip packs them.
// Padding states (s >= S) start the backward fill at -2^50 and read only states to their right, so they stay there; the
// forward fill's padding is never read by a state of the line, and a combine leaves it out.
// Every bound is re-checked on the line's own device numbers before anything is read through it; a refused line gets a
// status and touches nothing else.
#include "forced_two_fill.h"

namespace {

struct OmitConfArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off; const int32_t* q_char; const int32_t* q_frame; const int64_t* q_off;
    const int32_t* nq;
    int32_t nlines, no, variants, omit; int64_t rows, nlabels, nqueries;
    unsigned char* ws; int64_t ws_bytes;
    int64_t* confidence; int32_t* rival; int32_t* status;
};

struct OmitConfLine {
    const float* P; const int32_t* cs;
    const int32_t* qc; const int32_t* qf;      // the line's queries: character and frame
    unsigned char* fwd;                        // its piece of the workspace: row j = the forward fill at qf[j]
    int64_t* confidence; int32_t* rival;       // the line's rows of the two outputs, one per query
    int T, L, no, nq, omit;
};

// a forward row of 64 K int64 per query
__host__ __device__ inline int64_t omit_conf_ws_bytes(int L, int64_t nq) { return 512 * (int64_t)forced_k(2 * L + 1) * nq; }

// two_fill_best's reduction: ta_forced_conf.hip's packing, the largest key is the largest value at the smallest state
struct OmitConfCells {
    using Red = long long;     // [73]: 64 lanes' candidates, 8 partial maxima, the own state's value
    using Cand = long long;
    __device__ static __forceinline__ void put(Red* red, int i, Cand c) { red[i] = c; }
    __device__ static __forceinline__ Cand get(const Red* red, int i) { return red[i]; }
    __device__ static __forceinline__ bool better(Cand a, Cand b) { return a > b; }
};

// lane `from`'s value, the same in every lane
__device__ __forceinline__ long long lane_value(long long v, int from) {
    const int lo = __builtin_amdgcn_readlane((int)v, from);
    const int hi = __builtin_amdgcn_readlane((int)(v >> 32), from);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// inclusive max-scan over the 64 lanes from the RIGHT: lane l gets the maximum of the lanes l .. 63.  Hillis-Steele inside a
// row of 16, wave_max_scan's row steps mirrored; there is no row_bcast towards lower lanes, so the first lanes of the rows
// 1 .. 3 (each its row's maximum) are read as wave-uniform values and a row takes those of the rows above it
__device__ __forceinline__ long long wave_max_suffix_scan(long long v, int lane) {
    v = max64(v, dpp_or_self<0x101, 0xf>(v));          // row_shl:1
    v = max64(v, dpp_or_self<0x102, 0xf>(v));          // row_shl:2
    v = max64(v, dpp_or_self<0x104, 0xf>(v));          // row_shl:4
    v = max64(v, dpp_or_self<0x108, 0xf>(v));          // row_shl:8
    const long long m3 = lane_value(v, 48), m2 = max64(lane_value(v, 32), m3), m1 = max64(lane_value(v, 16), m2);
    const int row = lane >> 4;
    return max64(v, row == 0 ? m1 : row == 1 ? m2 : row == 2 ? m3 : kNeg);
}

template <int K>
__device__ __forceinline__ void omit_conf_line(const OmitConfLine& ln, int lane, int* qtab, long long* red) {
    constexpr int H = K / 2;                           // labels per lane
    const int T = ln.T, L = ln.L, no = ln.no, nq = ln.nq, S = 2 * L + 1;
    const long long omit = ln.omit;
    const long long pen0 = omit * (long long)(lane * H);           // omit * (the lane's first character)
    int lab[H];
    unsigned skipf;
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab, &skipf);
    long long v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;
    Feed<int> feed(qtab, no, lane);
    const int nchunks = (T + kChunk - 1) / kChunk;
    auto frame_of = [&](int j) { return j >= 0 && j < nq ? __builtin_amdgcn_readfirstlane(ln.qf[j]) : -1; };

    // ---- forward fill; the row of every query frame is kept -------------------------------------------------------------
    int cur = 0, want = frame_of(0);                   // wave-uniform: the next query whose frame is still ahead
    feed.prefetch(ln.P, T, 0);
    for (int c = 0; c < nchunks; ++c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
            if (t == 0) {                              // omit_seed<K>, spelled out
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] = (long long)((k & 1) ? q[lab[k >> 1]] : qb) - (pen0 + omit * (k >> 1));
            } else {                                   // omit_step<K, false> without its moves and bits, spelled out
                long long but_last = kNeg;
#pragma unroll
                for (int k = 0; k < K - 1; ++k) but_last = max64(but_last, v[k] + pen0 + omit * ((k + 1) >> 1));
                const long long total = max64(but_last, v[K - 1] + pen0 + omit * (K >> 1));
                const long long inc = from_left(wave_max_scan(total), kNeg);       // Pm of the state in front of the lane
                long long pm_even = from_left(max64(inc, but_last), kNeg);         // Pm[2 i - 2] of the lane's first character
                long long run = inc, o1 = from_left(v[K - 1], kNeg), o2 = kNeg, far = kNeg;
#pragma unroll
                for (int k = 0; k < K; ++k) {          // upwards: o1 and o2 carry the old row's v[k - 1] and v[k - 2]
                    const long long old = v[k];
                    run = max64(run, old + pen0 + omit * ((k + 1) >> 1));
                    if (!(k & 1)) {
                        far = pm_even - (pen0 + omit * (k >> 1));                  // lane 0's first character: kNeg, never taken
                        pm_even = run;
                    }
                    long long best = max64(old, o1);
                    if ((k & 1) && ((skip >> (k >> 1)) & 1u)) best = max64(best, o2);
                    best = max64(best, far);
                    v[k] = best + ((k & 1) ? q[lab[k >> 1]] : qb);
                    o2 = o1;
                    o1 = old;
                }
            }
            while (want == t) {
                long long* row = reinterpret_cast<long long*>(ln.fwd) + (int64_t)cur * (64 * K);
#pragma unroll
                for (int k = 0; k < K; ++k) row[k * 64 + lane] = v[k];
                ++cur;
                want = frame_of(cur);
            }
        }
    }

    // ---- backward fill, and the combine at every query frame -----------------------------------------------------------
    cur = nq - 1;
    want = frame_of(cur);
    auto combine_at = [&](int frame) {                 // the queries at `frame`, the one v holds B of
        while (want == frame) {
            const long long* row = reinterpret_cast<const long long*>(ln.fwd) + (int64_t)cur * (64 * K);
            const int own = 2 * __builtin_amdgcn_readfirstlane(ln.qc[cur]) + 1;
            long long key = kNeg * 2048;               // below every candidate's
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int s = lane * K + k;
                const long long g = row[k * 64 + lane] + v[k];             // what this very lane stored in the forward fill
                const long long cand = g * 2048 + (2047 - s);              // the larger value first, then the smaller state
                if (s == own) red[72] = g;
                else if (s < S && cand > key) key = cand;
            }
            const long long m = two_fill_best<OmitConfCells>(red, lane, key);
            if (lane == 0) {
                ln.confidence[cur] = red[72] - (m >> 11);
                ln.rival[cur] = 2047 - (int)(m & 2047);
            }
            wave_lds_sync();                           // red is free again
            --cur;
            want = frame_of(cur);
        }
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {                      // the end rule, for every state of the line
        const int s = lane * K + k;
        v[k] = s < S ? -(omit * (long long)(L - (lane * H + ((k + 1) >> 1)))) : kNeg;
    }
    combine_at(T - 1);
    feed.prefetch(ln.P, T, nchunks - 1);
    for (int c = nchunks - 1; c >= 0; --c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c - 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t1 - 1; t >= t0 && t >= 1; --t) {  // the emission of frame t takes the fill from t to t - 1
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
            long long total = kNeg, tail2 = kNeg;      // the lane's maximum of c[], and that of all but its first two states
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                v[k] += (k & 1) ? q[lab[k >> 1]] : qb;                     // w
                if (k == 1) tail2 = total;
                total = max64(total, v[k] - (pen0 + omit * (k >> 1)));
            }
            const long long right = from_right(wave_max_suffix_scan(total, lane), kNeg);    // Sm at the right lane's state 0
            long long sm_even = from_right(max64(right, tail2), kNeg);                     // Sm at the right lane's state 2
            long long run = right, o1 = from_right(v[0], kNeg), o2 = from_right(v[1], kNeg);
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {         // downwards: o1 and o2 carry w[k + 1] and w[k + 2], run Sm[k + 1]
                const long long old = v[k];
                const long long far = sm_even + (pen0 + omit * ((k + 1) >> 1));    // Sm[2 up + 2]: k + 3 (odd k), k + 2 (even k)
                if (k & 1) sm_even = run;              // Sm[k + 1], for the two states below
                run = max64(run, old - (pen0 + omit * (k >> 1)));
                long long best = max64(old, o1);
                if ((k & 1) && ((skipf >> (k >> 1)) & 1u)) best = max64(best, o2);
                v[k] = max64(best, far);
                o2 = o1;
                o1 = old;
            }
            combine_at(t - 1);
        }
    }
}

// One launch per variant the host's copies call for, each over all lines, as forced_conf_kernel: a line belongs to the
// launch of ITS K (from the device's L) and the others leave at once; a line that fails the checks, or whose K no launch of
// this call covers, is refused by every launch alike.
template <int K>
__global__ __launch_bounds__(64) void forced_omit_conf_kernel(OmitConfArgs a) {
    __shared__ int qtab[2 * kChunk * kMaxNo];          // two chunks of emission scores (8 KiB)
    __shared__ long long red[73];
    const int b = blockIdx.x, lane = threadIdx.x;
    auto refuse = [&](int status) {
        if (lane == 0) a.status[b] = status;
    };
    const int T = __builtin_amdgcn_readfirstlane(a.T[b]), L = __builtin_amdgcn_readfirstlane(a.L[b]);
    const int nq = __builtin_amdgcn_readfirstlane(a.nq[b]);
    const int64_t r0 = a.row_off[b], l0 = a.lab_off[b], w0 = a.ws_off[b], q0 = a.q_off[b];
    const bool nq_ok = nq >= 0 && nq <= 2 * (int64_t)L;
    if (a.omit < 0 || a.omit > TA_FORCED_OMIT_MAX || a.nqueries < 0 ||
        !line_ok(a, T, L, r0, l0, w0, [&] { return nq_ok ? omit_conf_ws_bytes(L, nq) : 0; }))
        return refuse(TA_FORCED_BOUNDS);
    if (!nq_ok) return refuse(TA_FORCED_QUERY);
    if (q0 < 0 || q0 > a.nqueries || nq > a.nqueries - q0) return refuse(TA_FORCED_BOUNDS);
    if (forced_k(2 * L + 1) != K) return;              // wave-uniform
    const int32_t* cs = a.labels + l0;
    if (!labels_ok(cs, L, a.no, lane)) return refuse(TA_FORCED_LABEL);
    const int32_t* qc = a.q_char + q0;
    const int32_t* qf = a.q_frame + q0;
    bool bad = false;                                  // a frame of the line, none before the one in front; a character of the text
    for (int j = lane; j < nq; j += 64) {
        const int t = qf[j], i = qc[j];
        bad |= t < 0 || t >= T || (j >= 1 && t < qf[j - 1]) || i < 0 || i >= L;
    }
    if (__any(bad)) return refuse(TA_FORCED_QUERY);
    const OmitConfLine ln{a.probs + r0 * a.no, cs, qc, qf, a.ws + w0, a.confidence + q0, a.rival + q0, T, L, a.no, nq, a.omit};
    omit_conf_line<K>(ln, lane, qtab, red);
    if (lane == 0) a.status[b] = TA_FORCED_OK;
}

}  // namespace

extern "C" int64_t ta_forced_omit_confidence_workspace_bytes(int32_t T, int32_t L, int32_t nq) {
    return forced_ws_guard(T, L) && nq >= 0 && nq <= 2 * L ? omit_conf_ws_bytes(L, nq) : -1;
}

extern "C" int ta_forced_omit_confidence(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                                         const int64_t* lab_off, const int32_t* L, const int64_t* ws_off,
                                         const int32_t* q_char, const int32_t* q_frame, const int64_t* q_off,
                                         const int32_t* nq, int32_t nlines, int32_t no, int64_t rows, int64_t nlabels,
                                         int64_t nqueries, const int32_t* T_host, const int32_t* L_host,
                                         const int32_t* nq_host, int32_t omit_q, void* workspace, int64_t workspace_bytes,
                                         int64_t* confidence, int32_t* rival, int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines < 0 || rows < 0 || nlabels < 0 || nqueries < 0 || workspace_bytes < 0, no,
                             omit_q < 0 || omit_q > TA_FORCED_OMIT_MAX ? "omit_q outside 0 .. TA_FORCED_OMIT_MAX" : nullptr,
                             nlines == 0,
                             !probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !q_char || !q_frame ||
                                 !q_off || !nq || !T_host || !L_host || !nq_host || !workspace || !confidence || !rival ||
                                 !status,
                             workspace, &go);
    if (!go) return rc;
    int variants;                                      // the lines' own sizes first; their pieces depend on the queries
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, [](int, int) { return 0; },
                            "ta_forced_omit_confidence_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    int64_t need = 0, sum_q = 0;
    for (int b = 0; b < nlines; ++b) {
        const int n = nq_host[b];
        if (n < 0 || n > 2 * L_host[b]) return ta_fail(TA_EINVAL, "a line's queries outside 0 .. 2 L");
        need += omit_conf_ws_bytes(L_host[b], n);
        sum_q += n;
    }
    if (sum_q > nqueries) return ta_fail(TA_EINVAL, "the lines' queries exceed nqueries");
    if (workspace_bytes < need) return forced_ws_small("lines", "ta_forced_omit_confidence_workspace_bytes");
    const OmitConfArgs a{probs, row_off, T, labels, lab_off, L, ws_off, q_char, q_frame, q_off, nq, nlines, no, variants,
                         omit_q, rows, nlabels, nqueries, static_cast<unsigned char*>(workspace), workspace_bytes,
                         confidence, rival, status};
    const hipError_t e = forced_launch_variants(variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_omit_conf_kernel<decltype(kc)::value>), dim3((unsigned)nlines), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
    if (e != hipSuccess) return ta_fail_hip(e, "forced_omit_conf_kernel launch");
    return TA_OK;
}
