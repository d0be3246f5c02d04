// ta_forced_omit.hip -- forced alignment whose path may OMIT characters of the text at a price per character (DESIGN.md
// section 14.9): the page abbreviates, spells differently and drops words, and a character the scribe never wrote must
// not take a frame from its neighbours.  Integers only from the float32 probabilities on; the checker of record is
// tests/forced_omit_ref.py.
//
// forced_omit_kernel<K>, one wave per line, on forced_common.h: the lanes' K states and labels (lane_labels), the chunked
// LDS table of emission scores (Feed), the hand-over from the left lane (from_left), the moves (store_moves) and the
// walk's LDS blocks (stage_moves, staged_move), and the omission pieces it shares with ta_forced_page_omit.hip: the
// wave-wide max-scan (wave_max_scan), the bit words (store_bits), the end rule (omit_end) and the far move's source
// (far_source).  The seed and the cell are omit_seed<K> and omit_step<K, false>, spelled out in the fill: as calls K = 16
// and K = 32 spill scalars and K = 32 works out of twice the AGPRs (profiles/forced_page_shared.txt).  It runs upwards.  The
// far move, per timestep:
//   far    a state s of character i = s / 2 >= 1 may be entered from ANY s' <= 2 i - 2 for omit * (the label states
//          strictly between).  With a[x] = v[x] + omit * ceil(x / 2) and Pm[x] = max(a[0 .. x]) the far candidate of the
//          blank 2 i and of the label 2 i + 1 alike is Pm[2 i - 2] - omit * i.  A lane forms the maximum of its K a's,
//          ONE wave-wide inclusive max-scan of that int64 (DPP row_shr 1 / 2 / 4 / 8, row_bcast 15 and 31: no LDS, no
//          barrier) shifted by a lane gives the maximum of everything to its left, and a second shift Pm[2 i - 2] of the
//          lane's first character (the state before last of the left lane).  Tie order stay > advance > skip > far;
//          move code 3 = far.
//   bits   "a[x] >= Pm[x - 1]", one per state and timestep: the far move's s' is the first set bit at or below
//          2 i - 2 (the largest s' among equal candidates).  Bit 0 is always set.
// Workspace of a line (T, K): forced_ws_rows(T, K) rows of 64 move words as store_moves lays them out, then
// ceil(T / (32 / K)) rows of 64 bit words: lane l's word of row r holds, for the timesteps t = r (32 / K) + j, the K bits
// of its states at bit K j + k.  256-byte rows, plain vector stores.
//   end    fin[s] = v[s] - omit * (L - ceil(s / 2)); the largest, the largest s on a tie: every lane's best goes through
//          LDS and every lane reads all 64.
//   walk   wave-uniform.  The frames of the line are set to -1 before the fill; a far move reads the bit row of its
//          timestep from the walk's LDS block (a ballot finds the lane, its word the state), and the characters it jumps
//          over keep the -1.
// Every bound is re-checked on the line's own device numbers before anything is read through it; a refused line gets a
// status and touches nothing else.
#include "forced_common.h"

namespace {

struct OmitArgs {
    const float* probs; const int64_t* row_off; const int32_t* T; const int32_t* labels; const int64_t* lab_off;
    const int32_t* L; const int64_t* ws_off;
    int32_t nlines, no, variants, omit; int64_t rows, nlabels;
    unsigned char* ws; int64_t ws_bytes;
    int32_t* frames; int64_t* score; int32_t* status;
    // ta_forced_align_omit_lines alone: block k is a packed slot, its line acc_line[k] of the chunk's nlines_all lines
    // (row_off, T, ws_off and Lcap per CHUNK line; labels, lab_off, L per slot), count[0] the slots that are filled
    const int32_t* acc_line; const int64_t* count; const int32_t* Lcap; int32_t nlines_all;
};

__host__ __device__ inline int64_t omit_ws_bytes(int T, int L) {
    const int K = forced_k(2 * L + 1);
    return 256 * (forced_ws_rows(T, K) + omit_bit_rows(T, K));
}

struct OmitLine {
    const float* P; const int32_t* cs; uint32_t* moves; int32_t* frames;
    int T, L, no, omit;
};

template <int K>
__device__ __forceinline__ long long omit_line(const OmitLine& ln, int lane, int* qtab, uint32_t* stage, long long* fin_v,
                                               int* fin_s) {
    constexpr int H = K / 2;                           // labels per lane
    constexpr int SPB = 32 / K;                        // steps per bit word
    const int T = ln.T, L = ln.L, no = ln.no;
    const long long omit = ln.omit;
    const long long pen0 = omit * (long long)(lane * H);           // omit * (the lane's first character)
    int lab[H];
    const unsigned skip = lane_labels(ln.cs, 0, L, lane, lab);
    for (int i = lane; i < 3 * L; i += 64) ln.frames[i] = TA_FORCED_OMITTED;
    long long v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = kNeg;

    // ---- fill -----------------------------------------------------------------------------------------------------
    uint32_t* bitrows = ln.moves + forced_ws_rows(T, K) * 64;
    Feed<int> feed(qtab, no, lane);
    const int nchunks = (T + kChunk - 1) / kChunk;
    feed.prefetch(ln.P, T, 0);
    uint32_t acc = 0, accb = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int* qbuf = feed.publish(c, emission_q);
        feed.prefetch(ln.P, T, c + 1);
        wave_lds_sync();
        const int t0 = c * kChunk, t1 = t0 + kChunk < T ? t0 + kChunk : T;
        for (int t = t0; t < t1; ++t) {
            const int* q = qbuf + (t - t0) * no;
            const int qb = q[0];
            unsigned long long mv = 0;
            uint32_t bits = 0;
            if (t == 0) {                              // omit_seed<K>, spelled out: as a call K = 32 takes 51 AGPRs for 28
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] = (long long)((k & 1) ? q[lab[k >> 1]] : qb) - (pen0 + omit * (k >> 1));
            } else {
                // omit_step<K, false>, spelled out: as a call K = 16 and K = 32 spill scalars, K = 32 doubles its AGPRs
                // the lane's maximum of a[], and that of all but its last state
                long long but_last = kNeg;
#pragma unroll
                for (int k = 0; k < K - 1; ++k) but_last = max64(but_last, v[k] + pen0 + omit * ((k + 1) >> 1));
                const long long total = max64(but_last, v[K - 1] + pen0 + omit * (K >> 1));
                const long long inc = from_left(wave_max_scan(total), kNeg);       // Pm of the state in front of the lane
                long long pm_even = from_left(max64(inc, but_last), kNeg);         // Pm[2 i - 2] of the lane's first character
                const long long left = from_left(v[K - 1], kNeg);
                long long run = inc, o1 = left, o2 = kNeg, far = kNeg;
#pragma unroll
                for (int k = 0; k < K; ++k) {          // upwards: o1 and o2 carry the old row's v[k - 1] and v[k - 2]
                    const long long old = v[k];
                    const long long ak = old + pen0 + omit * ((k + 1) >> 1);
                    if (ak >= run) bits |= 1u << k;
                    run = max64(run, ak);
                    if (!(k & 1)) {
                        far = pm_even - (pen0 + omit * (k >> 1));                  // lane 0's first character: kNeg, never taken
                        pm_even = run;
                    }
                    long long best = old;
                    unsigned m = 0;
                    if (o1 > best) { best = o1; m = 1; }
                    if ((k & 1) && ((skip >> (k >> 1)) & 1u) && o2 > best) { best = o2; m = 2; }
                    if (far > best) { best = far; m = 3; }
                    v[k] = best + ((k & 1) ? q[lab[k >> 1]] : qb);
                    mv |= (unsigned long long)m << (2 * k);
                    o2 = o1;
                    o1 = old;
                }
            }
            store_moves<K>(ln.moves, t, T, lane, mv, acc);
            store_bits<K>(bitrows, t, T, lane, bits, accb);
        }
    }

    // ---- end: the largest fin, the largest s on a tie ------------------------------------------------------------------
    long long best;
    int s = omit_end<K>(v, omit, 0, L, lane, fin_v, fin_s, &best);             // the moves and the -1 frames: fenced there

    // ---- walk: wave-uniform, the moves and bits of kWalk timesteps at a time through LDS -------------------------------
    constexpr int RPB = walk_rows(K);                                  // move rows per block
    constexpr int BPB = kWalk / SPB;                                   // bit rows per block
    const int64_t nrows = forced_ws_rows(T, K), nbrows = omit_bit_rows(T, K);
    int last = 0, base = -1;
    bool inside = false;                               // the step behind (t + 1) was spent in the same state
    for (int t = T - 1; t >= 0 && s >= 0; --t) {
        if ((t & ~(kWalk - 1)) != base) {
            base = t & ~(kWalk - 1);
            __syncthreads();
            const int64_t b0 = base / SPB;
            stage_moves<K>(stage, ln.moves, base, nrows, lane);
            for (int r = 0; r < BPB && b0 + r < nbrows; ++r) stage[(RPB + r) * 64 + lane] = bitrows[(b0 + r) * 64 + lane];
            __syncthreads();
        }
        const int tt = t - base;
        unsigned m = staged_move<K>(stage, tt, s / K, s % K);
        if (t == 0) m = 1;                             // the path starts here: whatever state this is, it is left
        if ((s & 1) && !inside) last = t;
        if ((s & 1) && m != 0 && lane == 0) {
            ln.frames[3 * (s >> 1)] = t;
            ln.frames[3 * (s >> 1) + 1] = last;
        }
        inside = m == 0;
        if (m == 3) {                                  // far: down the bit row from 2 i - 2 to the first set bit
            s = far_source<K>(stage + RPB * 64, tt, 2 * (s >> 1) - 2, lane);           // -1: bit 0 of every row is set
        } else {
            s -= (int)m;
        }
    }
    __threadfence();
    __syncthreads();

    // ---- peak: a lane per character; one the path never entered keeps its -1 -------------------------------------------
    for (int i = lane; i < L; i += 64) {
        const int tf = ln.frames[3 * i], tl = ln.frames[3 * i + 1], c = ln.cs[i];
        if (tf < 0 || tl < tf || tl >= T) continue;
        ln.frames[3 * i + 2] = peak_frame(ln.P, no, c, tf, tl);
    }
    return best;
}

// One launch per variant the host's copies call for, each over all lines, as forced_align_kernel: a line belongs to the
// launch of ITS K (from the device's L) and the others leave at once; a line that fails the checks, or whose K no launch
// of this call covers, is refused by every launch alike.
// kSlots (ta_forced_align_omit_lines): the blocks are the packed slots ta_harvest_pack left on the device, as in
// forced_align_kernel.  A slot behind count[0] -- or any slot of a call whose count[0] is negative -- leaves before it has
// read or written anything else; a filled slot finds its line through acc_line and is held to that line's cap on top of
// the checks below.
template <int K, bool kSlots>
__global__ __launch_bounds__(64) void forced_omit_kernel(OmitArgs a) {
    constexpr int kRows = walk_rows(K) + kWalk * K / 32;               // move and bit rows of a walk block
    constexpr int kWords = kRows * 64 > 2 * kChunk * kMaxNo ? kRows * 64 : 2 * kChunk * kMaxNo;
    __shared__ uint32_t stage[kWords];                 // two chunks of emission scores (8 KiB), then the walk's blocks
    __shared__ long long fin_v[64];
    __shared__ int fin_s[64];
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
    if (a.omit < 0 || a.omit > TA_FORCED_OMIT_MAX || !line_ok(a, T, L, r0, l0, w0, [&] { return omit_ws_bytes(T, L); })) {
        if (lane == 0) a.status[b] = TA_FORCED_BOUNDS;
        return;
    }
    if (forced_k(2 * L + 1) != K) return;              // wave-uniform
    const int32_t* cs = a.labels + l0;
    if (!labels_ok(cs, L, a.no, lane)) {
        if (lane == 0) a.status[b] = TA_FORCED_LABEL;
        return;
    }
    const OmitLine ln{a.probs + r0 * a.no, cs, reinterpret_cast<uint32_t*>(a.ws + w0), a.frames + 3 * l0, T, L, a.no, a.omit};
    const long long best = omit_line<K>(ln, lane, qtab, stage, fin_v, fin_s);
    if (lane == 0) {
        a.score[b] = best;
        a.status[b] = TA_FORCED_OK;
    }
}

template <bool kSlots>
hipError_t launch_variants(const OmitArgs& a, void* stream) {
    return forced_launch_variants(a.variants, [&](auto kc) {
        hipLaunchKernelGGL((forced_omit_kernel<decltype(kc)::value, kSlots>), dim3((unsigned)a.nlines), dim3(64), 0,
                           reinterpret_cast<hipStream_t>(stream), a);
    });
}

}  // namespace

extern "C" int64_t ta_forced_omit_workspace_bytes(int32_t T, int32_t L) {
    return forced_ws_guard(T, L) ? omit_ws_bytes(T, L) : -1;
}

extern "C" int ta_forced_align_omit(const float* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                                    const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines,
                                    int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host,
                                    int32_t omit_q, void* workspace, int64_t workspace_bytes, int32_t* frames,
                                    int64_t* score, int32_t* status, void* stream) {
    bool go;
    int rc = forced_preamble(nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0, no,
                             omit_q < 0 || omit_q > TA_FORCED_OMIT_MAX ? "omit_q outside 0 .. TA_FORCED_OMIT_MAX" : nullptr,
                             nlines == 0,
                             !probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !T_host || !L_host ||
                                 !workspace || !frames || !score || !status,
                             workspace, &go);
    if (!go) return rc;
    int variants;
    rc = forced_check_lines(T_host, L_host, nlines, rows, nlabels, workspace_bytes, omit_ws_bytes,
                            "ta_forced_omit_workspace_bytes", &variants);
    if (rc != TA_OK) return rc;
    const OmitArgs a{probs, row_off, T, labels, lab_off, L, ws_off, nlines, no, variants, omit_q, rows, nlabels,
                     static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status,
                     nullptr, nullptr, nullptr, 0};
    const hipError_t e = launch_variants<false>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_omit_kernel launch");
    return TA_OK;
}

extern "C" int ta_forced_align_omit_lines(const float* probs, const int64_t* row_off_all, const int32_t* T_all,
                                          const int64_t* ws_off_all, const int32_t* Lcap, const int32_t* acc_line,
                                          const int32_t* L, const int64_t* lab_off, const int32_t* labels,
                                          const int64_t* count, int32_t nlines_all, int32_t nslots, int32_t no,
                                          int64_t rows, int64_t label_cap, const int32_t* T_all_host,
                                          const int32_t* Lcap_host, int32_t omit_q, void* workspace,
                                          int64_t workspace_bytes, int32_t* frames, int64_t* score, int32_t* status,
                                          void* stream) {
    bool go;
    int rc = forced_preamble(nlines_all < 0 || nslots < 0 || rows < 0 || label_cap < 0 || workspace_bytes < 0, no,
                             nslots > nlines_all                        ? "more slots than lines"
                             : omit_q < 0 || omit_q > TA_FORCED_OMIT_MAX ? "omit_q outside 0 .. TA_FORCED_OMIT_MAX"
                                                                         : nullptr,
                             nlines_all == 0 || nslots == 0,
                             !probs || !row_off_all || !T_all || !ws_off_all || !Lcap || !acc_line || !L || !lab_off ||
                                 !labels || !count || !T_all_host || !Lcap_host || !workspace || !frames || !score || !status,
                             workspace, &go);
    if (!go) return rc;
    int64_t need;                                      // a cap's piece is never below that of a shorter text
    int capmax;                                        // (ta_forced_omit_workspace_bytes never decreases with L)
    rc = forced_check_chunk(T_all_host, Lcap_host, nlines_all, rows, omit_ws_bytes, &need, &capmax);
    if (rc != TA_OK) return rc;
    if (workspace_bytes < need) return forced_ws_small("lines", "ta_forced_omit_workspace_bytes");
    if (capmax == 0) return TA_OK;                     // no line can take a slot
    const int variants = variants_up_to(forced_k(2 * capmax + 1));
    const OmitArgs a{probs, row_off_all, T_all, labels, lab_off, L, ws_off_all, nslots, no, variants, omit_q, rows, label_cap,
                     static_cast<unsigned char*>(workspace), workspace_bytes, frames, score, status,
                     acc_line, count, Lcap, nlines_all};
    const hipError_t e = launch_variants<true>(a, stream);
    if (e != hipSuccess) return ta_fail_hip(e, "forced_omit_kernel launch (slots)");
    return TA_OK;
}
