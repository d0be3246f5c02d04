// ta_forced.hip -- forced alignment of a text line's known text with the recogniser's class posteriors (DESIGN.md
// section 14.7): the best CTC path through exactly that text, and where every character of it sits.  Integers only from
// the float32 probabilities on; the checker of record is tests/forced_ref.py.
//
// forced_align_kernel<K>, one wave per line.  The lattice has S = 2 L + 1 states (blank, c0, blank, c1, ... blank); lane l
// holds the K consecutive states l K .. l K + K - 1 as int64 registers, K = 2 / 4 / 8 / 16 / 32 chosen from S
// (forced_k), so a lane's even registers are blanks and its odd ones the K / 2 labels it keeps in registers.
//   fill   timestep after timestep.  A state takes the best of stay / advance / skip (ties in that order) and adds its
//          emission score.  K is even, so across a lane boundary only the left lane's LAST value is ever needed (the
//          advance into a lane's first blank, the skip into its first label): one int64 = two wave_shr:1 DPP moves.
//          Emission scores: the probability rows of kChunk timesteps are loaded a chunk ahead into registers, turned
//          into the integer score q once per (timestep, class) and published in LDS (two buffers, one hand-over per
//          chunk, no barrier anywhere in the fill); a step reads q[blank] and q[label] of its K / 2 labels.  Two move
//          bits per state go to the workspace as plain vector stores, 16 / K steps packed per 32-bit word and lane
//          (K = 32: two words per step), rows of 64 words.
//   walk   back from the better of the last two states.  The moves come back through LDS in blocks of kWalk timesteps,
//          loaded coalesced by the whole wave; inside a block the walk reads LDS only.  t_first / t_last of a character
//          are written when the path leaves its state.
//   peak   a lane per character scans its few frames for the first largest q.
// Every bound is re-checked on the line's own device numbers before anything is read through it; a refused line gets a
// status and touches nothing else.
#include "forced_common.h"

namespace {

struct ForcedArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off;
    int32_t nlines, no, variants; int64_t rows, nlabels;     // variants: a bit per K that this call launches
    unsigned char* ws; int64_t ws_bytes;
    int32_t* frames; int64_t* score; int32_t* status;
    // ta_forced_align_lines alone: block k is a packed slot, its line acc_line[k] of the chunk's nlines_all lines
    // (row_off, T, ws_off and Lcap per CHUNK line; labels, lab_off, L per slot), count[0] the slots that are filled
    const int32_t* acc_line; const int64_t* count; const int32_t* Lcap; int32_t nlines_all;
};

// the piece of the workspace for a line of T timesteps and L characters
__host__ __device__ inline int64_t forced_ws_bytes(int T, int L) { return 256 * forced_ws_rows(T, forced_k(2 * L + 1)); }

struct Line {
    const float* P;            // the line's first probability row
    const int32_t* cs;         // its labels
    uint32_t* moves;           // its piece of the workspace
    int32_t* frames;           // its rows of frames
    int T, L, no;
};

template <int K>
__device__ __forceinline__ long long forced_line(const Line& ln, int lane, int* qtab, uint32_t* stage, long long* vend) {
    constexpr int H = K / 2;                           // labels per lane
    const int T = ln.T, L = ln.L, no = ln.no, S = 2 * L + 1;
    int lab[H];
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab);
    long long v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;

    // ---- fill -----------------------------------------------------------------------------------------------------
    Feed<int> feed(qtab, no, lane);
    const int nchunks = (T + kChunk - 1) / kChunk;
    feed.prefetch(ln.P, T, 0);
    uint32_t acc = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
            unsigned long long mv = 0;
            if (t == 0) {
                if (lane == 0) { v[0] = qb; v[1] = q[lab[0]]; }
            } else {
                const long long left = from_left(v[K - 1], kNeg);
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {     // forced_step<K, false>, spelled out: as a call K = 32 goes to AGPRs
                    long long best = v[k];
                    unsigned m = 0;
                    const long long adv = k >= 1 ? v[k - 1] : left;
                    if (adv > best) { best = adv; m = 1; }
                    if (k & 1) {
                        const long long sk = k >= 2 ? v[k - 2] : left;
                        if (((skip >> (k >> 1)) & 1u) && sk > best) { best = sk; m = 2; }
                        v[k] = best + q[lab[k >> 1]];
                    } else {
                        v[k] = best + qb;
                    }
                    mv |= (unsigned long long)m << (2 * k);
                }
            }
            store_moves<K>(ln.moves, t, T, lane, mv, acc);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = lane * K + k;
        if (s == S - 1) vend[0] = v[k];
        if (s == S - 2) vend[1] = v[k];
    }
    __threadfence();                                   // the moves are read back below, by other lanes
    __syncthreads();
    const long long e0 = vend[0], e1 = vend[1];
    int s = e1 > e0 ? S - 2 : S - 1;                   // on a tie the last blank

    // ---- walk: wave-uniform, the moves of kWalk timesteps at a time through LDS ----------------------------------------
    const int64_t nrows = forced_ws_rows(T, K);
    int last = 0, base = -1;
    bool inside = false;                               // the step behind (t + 1) was spent in the same state
    for (int t = T - 1; t >= 0 && s >= 0; --t) {
        if ((t & ~(kWalk - 1)) != base) {
            base = t & ~(kWalk - 1);
            __syncthreads();
            stage_moves<K>(stage, ln.moves, base, nrows, lane);
            __syncthreads();
        }
        unsigned m = staged_move<K>(stage, t - base, s / K, s % K);
        if (t == 0) m = 1;                             // the path starts here: whatever state this is, it is left
        if ((s & 1) && !inside) last = t;
        if ((s & 1) && m != 0 && lane == 0) {
            ln.frames[3 * (s >> 1)] = t;
            ln.frames[3 * (s >> 1) + 1] = last;
        }
        inside = m == 0;
        s -= (int)m;
    }
    __threadfence();
    __syncthreads();

    // ---- peak: a lane per character ------------------------------------------------------------------------------------
    for (int i = lane; i < L; i += 64) {
        const int tf = ln.frames[3 * i], tl = ln.frames[3 * i + 1], c = ln.cs[i];
        ln.frames[3 * i + 2] = tf >= 0 && tl < T ? peak_frame(ln.P, no, c, tf, tl) : tf;
    }
    return e1 > e0 ? e1 : e0;
}

// One launch per variant the host's copies call for, each over all lines: a line belongs to the launch of ITS K (from the
// device's L) and the others leave at once.  A line that fails the checks, or whose K no launch of this call covers
// (`variants`: the device's L disagrees with the host's copy), is refused by every launch alike.
// kSlots (ta_forced_align_lines): the blocks are the packed slots ta_harvest_pack left on the device.  A slot behind
// count[0] -- or any slot of a call whose count[0] is negative -- leaves before it has read or written anything else; a
// filled slot finds its line through acc_line and is held to that line's cap on top of the checks below.
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_align_kernel(ForcedArgs a) {
    constexpr int kWords = walk_rows(K) * 64 > 2 * kChunk * kMaxNo ? walk_rows(K) * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long vend[2];
    int* qtab = reinterpret_cast<int*>(stage);
    const int b = blockIdx.x, lane = threadIdx.x;
    int q = b;                                         // the line whose rows, timesteps and workspace piece block b takes
    if (kSlots) {
        if (!slot_filled(a.count, b)) return;
        q = slot_line(a.acc_line, a.nlines_all, b);
        if (q < 0) {
            if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
            return;
        }
    }
    const int T = __builtin_amdgcn_readfirstlane(a.T[q]), L = __builtin_amdgcn_readfirstlane(a.L[b]);
    const int64_t r0 = a.row_off[q], l0 = a.lab_off[b], w0 = a.ws_off[q];
    if (kSlots && L > __builtin_amdgcn_readfirstlane(a.Lcap[q])) {     // beyond what the host sized the line's piece for
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (!line_ok(a, T, L, r0, l0, w0, [&] { return forced_ws_bytes(T, L); })) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (forced_k(2 * L + 1) != K) return;              // wave-uniform
    const int32_t* cs = a.labels + l0;
    if (!labels_ok(cs, L, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    const Line ln{a.probs + r0 * a.no, cs, reinterpret_cast<uint32_t*>(a.ws + w0), a.frames + 3 * l0, T, L, a.no};
    const long long best = forced_line<K>(ln, lane, qtab, stage, vend);
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

template <bool kSlots>
hipError_t launch_variants(const ForcedArgs& a, void* stream) {
    return forced_launch_variants(a.variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_align_kernel<decltype(kc)::value, kSlots>), dim3((unsigned)a.nlines), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
}

}  // namespace

extern "C" int64_t ta_forced_workspace_bytes(int32_t T, int32_t L) {
    return forced_ws_guard(T, L) ? forced_ws_bytes(T, L) : -1;
}

extern "C" int ta_forced_align(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                               const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines, int32_t no,
                               int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host, void* workspace,
                               int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no, nullptr, nlines == 0,
                             !probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !T_host || !L_host ||
                                 !workspace || !frames || !score || !status,
                             workspace, &go);
    if (!go) return rc;
    int variants;
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, forced_ws_bytes,
                            "ta_forced_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const ForcedArgs a{probs, row_off, T, labels, lab_off, L, ws_off, nlines, no, variants, rows, nlabels,
                       static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status,
                       nullptr, nullptr, nullptr, 0};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_align_kernel launch");
    return TA_OK;
}

extern "C" int ta_forced_align_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all,
                                     const int64_t* ws_off_all, const int32_t* Lcap, const int32_t* acc_line,
                                     const int32_t* L, const int64_t* lab_off, const int32_t* labels,
                                     const int64_t* count, int32_t nlines_all, int32_t nslots, int32_t no, int64_t rows,
                                     int64_t label_cap, const int32_t* T_all_host, const int32_t* Lcap_host,
                                     void* workspace, int64_t workspace_bytes, int32_t* frames, int64_t* score,
                                     int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines_all < 0 || nslots < 0 || rows < 0 || label_cap < 0 || workspace_bytes < 0, no,
                             nslots > nlines_all ? "more slots than lines" : nullptr, nlines_all == 0 || nslots == 0,
                             !probs || !row_off_all || !T_all || !ws_off_all || !Lcap || !acc_line || !L || !lab_off ||
                                 !labels || !count || !T_all_host || !Lcap_host || !workspace || !frames || !score || !status,
                             workspace, &go);
    if (!go) return rc;
    int64_t need;                                      // a cap's piece is never below that of a shorter text
    int capmax;                                        // (forced_ws_rows grows with K)
    rc = forced_check_chunk(T_all_host, Lcap_host, nlines_all, rows, forced_ws_bytes, &need, &capmax);
    if (rc != TA_OK) return rc;
    if (workspace_bytes < need) return forced_ws_small("lines", "ta_forced_workspace_bytes");
    if (capmax == 0) return TA_OK;                     // no line can take a slot
    const int variants = variants_up_to(forced_k(2 * capmax + 1));
    const ForcedArgs a{probs, row_off_all, T_all, labels, lab_off, L, ws_off_all, nslots, no, variants, rows, label_cap,
                       static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status,
                       acc_line, count, Lcap, nlines_all};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_align_kernel launch (slots)");
    return TA_OK;
}
