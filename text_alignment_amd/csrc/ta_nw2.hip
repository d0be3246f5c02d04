// ta_nw2.hip -- two-phase form of the affine-gap aligner (same results as ta_nw.hip, bit for bit).
//
// The single-pass fill kernel (ta_nw.hip) is bound by VALU issue, and 40 % of its instructions only
// serve the pointer byte (tag clean-up, two v_bfi, byte packing).  The reference needs pointers
// only along the traceback path (textSeqCompare.py:96-164), so:
//
//  phase 1  nw_score_kernel   the same strip / lane / skew wavefront on RAW integer scores: per cell
//           v_cmp + v_cndmask, 3 v_add, 3 v_max3_i32 and nothing else; no pointer byte is formed
//           or stored.  It leaves checkpoints in HBM (0.07 B per cell): every kCkGroups groups the
//           wave's whole lane state, and per strip its bottom row (XG, D) -- which is also what the
//           next strip starts from.
//  phase 2  nw_trace2_kernel  one wave per problem walks back strip by strip and, inside a strip,
//           checkpoint interval by checkpoint interval: it re-runs the TAGGED cell over the
//           interval the walk is in, restarted from that interval's state checkpoint (two halo
//           steps make the missing winner tags of the restart state irrelevant), keeps the
//           interval's pointer bytes in LDS and walks them.  The bottom rows carry no tags either:
//           a step that leaves a strip upwards gets its next state from the tagged outputs of the
//           cell it lands on, once the strip above is re-filled.  About 10 % of the cells are
//           recomputed.
//
// Data flow and the halo argument are replayed on the CPU by tests/native/sim_nw.cpp (run2).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <atomic>
#include <map>
#include <type_traits>
#include <vector>

#include "nw_band.h"
#include "nw_cell.h"
#include "nw_hw.h"
#include "ta_common.h"

namespace ta {

#ifndef TA_CK_GROUPS
#define TA_CK_GROUPS 16
#endif
// State checkpoint every kCkGroups groups (a multiple of 4: the steady loop runs in blocks of 4 groups).
// The interval is also phase 2's chunk, whose pointer bytes (1 KiB per group) are what limits the
// number of traceback waves on a CU (measured by padding its LDS: 8 waves per CU 3.5 ms, 6: 4.8,
// 5: 5.6, 2: 10.7).  12 groups (10 waves per CU) were tried: 4.1 ms -- 28 % more chunks to set up and
// walk into, and 16 problems per CU do not divide into rounds of ten any better than into two of eight.
constexpr int kCkGroups = TA_CK_GROUPS;
static_assert(kCkGroups % 4 == 0 && kCkGroups >= 4, "whole blocks of four groups");
constexpr int kStateInts = 10;                // D[4], H[4], V[3], dsave
constexpr int kWsRange = 0x7ffff000;          // record count of a workspace buffer descriptor: every real offset is below

// Bottom rows kept per strip: not only the strip's last row (lane 63's, what the next strip starts from) but also
// lane 31's, so that phase 2 can restart HALF-strips of 128 rows (32 lanes) and carry two problems' half-strips in one
// wave (nw_trace2h_kernel).  The same two store instructions per group write both rows (each storing lane has its
// own offset); measured on phase 1 at 4096 x 4096^2: 11.30 ms with the strip rows only, 11.39 with lanes 31 and 63,
// 11.70 with lanes 15 / 31 / 47 / 63 (quarter-strips would save phase 2 no more than they cost here).
#ifndef TA_SUBROWS
#define TA_SUBROWS 2
#endif
constexpr int kSubRows = TA_SUBROWS;
constexpr int kSubLanes = 64 / kSubRows;
// per-problem layout of the phase-1/2 workspace (all offsets in bytes, 16-byte aligned)
struct Ws2 {
    int nstrips, ngroups, nck;
    int64_t rows, row_pitch, stck, total;
    __host__ __device__ Ws2(int n, int m) {
        using L = PtrLayout<4>;
        nstrips = L::nstrips(n);
        ngroups = L::ngroups(m);
        nck = ngroups / kCkGroups + 1;
        // bottom rows: row 0 is the table's boundary row, row 1 + kSubRows s + q the last row of lanes 16 q .. 16 q + 15
        // of strip s -- (XG or V~, D) per column, what the lane below consumes; top(s) = row kSubRows s is the row above
        // strip s.  Entry j sits at index j + 1, so that the four entries a group reads start on a 16-byte boundary.
        // Phase 1 hands a strip's results to the next strip through them (they are in L2 when the next wave, ~25
        // groups behind, reads them) and phase 2 restarts from them.  A lane that has passed its last column goes on
        // over pad columns (phase 1's steady loop): lane 15 writes entries up to column m + 51, hence the pitch.
        rows = 0;
        row_pitch = ((int64_t)(m + 72) * 8 + 15) & ~(int64_t)15;
        stck = rows + (int64_t)(nstrips * kSubRows + 1) * row_pitch;
        total = stck + (int64_t)nstrips * nck * kStateInts * 64 * 4;
    }
    __host__ __device__ int64_t row(int r) const { return rows + (int64_t)r * row_pitch; }
    __host__ __device__ int64_t top(int s) const { return row(s * kSubRows); }          // the row above strip s
    __host__ __device__ int64_t state(int s, int ck) const {
        return stck + ((int64_t)(s * nck + ck) * kStateInts * 64) * 4;
    }
};

struct RawRegs { int cmis, cmat, gox, goy; };

__device__ __forceinline__ void cell_raw_hw(const RawRegs& k, int d_ul, int v_u, int h_l, int t, int o,
                                            int& d, int& v, int& h) {
    const int cs = v_score(t, o, k.cmis, k.cmat);
    const int mr = d_ul + cs;
    const int xg = v_u + k.gox;
    const int yg = h_l + k.goy;
    d = v_max3(mr, xg, yg);
    v = v_max3(mr, v_u, yg);
    h = v_max3(mr, xg, h_l);
}

// carried form (nw_cell.h: cell_update_carried), compare-select score.  Plain C: hipcc selects v_max3_i32
// for the nested max itself and, unlike between asm statements, pads nothing (the predicated start-up
// groups that run this form were twice as expensive per cell as the steady ones).
__device__ __forceinline__ void cell_carried_hw(const RawRegs& k, int d_ul, int xg_u, int yg_l, int t, int o,
                                                int& d, int& xg, int& yg) {
    const int mr = d_ul + ((t == o) ? k.cmat : k.cmis);
    d = c_max3(mr, xg_u, yg_l);
    xg = max(d + k.gox, xg_u);
    yg = max(d + k.goy, yg_l);
}

__host__ __device__ inline bool fits_i8(int v) { return v >= -128 && v <= 127; }

static_assert(kCkGroups == 16, "band_groups is written for 16-group checkpoint intervals");

// LDS carve of phase 1 (dynamic): code ocode[kOPad+m+kOTail] | int prog[16] | uint32 profile[waves][apad][64]
// (the rows handed from strip to strip live in the workspace -- L2 -- not in LDS: Ws2::rows)
struct P1Lds {
    size_t oc_bytes, tbl_off, total;
    __host__ __device__ explicit P1Lds(int m, int code_bytes, int tbl_bytes = 0) {
        oc_bytes = ((size_t)(kOPad + m + kOTail) * code_bytes + 15) & ~(size_t)15;
        tbl_off = oc_bytes + 64;
        total = tbl_off + (size_t)tbl_bytes;
    }
};

// ---------------------------------------------------------------------------------------------
// phase 1
//
// MODE 1: the substitution score of a cell is a compare + select on the two token ids.
// MODE 2: score PROFILE in LDS.  Each wave keeps, for the 256 rows of the strip it is in, a table
//   profile[o][lane] = the four substitution scores (signed bytes) of the lane's four rows against
//   OCR token o; a step costs one conflict-free ds_read_b32 (bank = lane) for four cells and the
//   byte is unpacked by the SDWA add that forms M^.  The table never needs rebuilding: it holds
//   "mismatch" everywhere and a strip patches the <= 4 entries per lane where its transcript tokens
//   match (and restores them when it leaves).  OCR codes sit in LDS pre-multiplied by the row pitch
//   (256 B).  Needs a small alphabet (apad x 256 B per wave) and scores that fit a signed byte.
// Both modes use the carried cell (non-positive gap opens).  A problem that does not qualify
// (a positive gap open; in MODE 2 a score outside a byte; gox != goy under SAMEGO) runs every group
// through the predicated edge body with the general cell: correct, slower, and rare.
// OC (MODE 1) = uint8_t when every token id of the batch is below 255: the OCR codes then take 1 byte
// each in LDS and a 4096-column problem fits four workgroups per CU instead of three.
// BAND (MODE 2 only): 0 = every group of every strip; 1 = the band's groups only (band_groups), with the certificate
// at the table's last cell; 2 = every group, of the problems the banded launch did not certify (the fallback launch).
// 3 = the funnel's groups only (funnel_groups: narrower towards (n, m), or the band's own where the funnel is declined),
// with the certificate's three words per problem -- v0, the exit maximum, the strips counted -- left for
// nw_band_certify_kernel to compare; a fourth word, set before the launch, says which of the two sets of ranges runs.  The bounds and the exactness argument the certificates rest on are stated in nw_band.h.
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
template <int W, int MODE, bool SAMEGO, typename OC, int BAND = 0>
__global__ __launch_bounds__(W * 64, MODE == 1 ? 5 : 2) void nw_score_kernel(NwArgs a) {
    constexpr int R = 4;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    constexpr bool PROFILE = (MODE == 2);
    using LC = typename std::conditional<PROFILE, uint16_t, OC>::type;      // code type in LDS
    // groups between two looks at the progress word of the strip above: a strip follows the one
    // above at CHK + 17 groups, and the ramp of a workgroup (wave w idles w x that lag at the start,
    // the waves above idle as long at the end) is what a finer grain buys back
    constexpr int CHK = 4;
    constexpr bool FUNNEL = BAND == 3 || BAND == 4;
    constexpr bool LCS = BAND == 4;              // the funnel with the remainder bounded by the suffix LCS (nw_band.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    int p = blockIdx.x;
    if constexpr (BAND == 2) {
        if (a.band_ok[p] != 0) return;           // certified by the banded launch: its workspace stands
    }
    const int64_t t0 = a.t_off[p], o0 = a.o_off[p];
    const int n = (int)(a.t_off[p + 1] - t0);
    const int m = (int)(a.o_off[p + 1] - o0);
    if (n <= 0 || m <= 0) return;

    const int32_t* prm = a.params + (size_t)p * a.params_stride;
    const CellConsts c = make_consts(prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]);
    RawRegs kr;
    kr.cmis = prm[1] - prm[4] - prm[5]; kr.cmat = prm[0] - prm[4] - prm[5];
    kr.gox = prm[2]; kr.goy = prm[3];
    // state of a problem is kept in carried form (XG, YG) iff its gap opens are non-positive; phase 2
    // applies the same predicate when it reads checkpoints and bottom rows
    const bool carried = opens_nonpositive(kr.gox, kr.goy);
    const int xadj = carried ? kr.gox : 0, yadj = carried ? kr.goy : 0;
    const int apad = PROFILE ? a.apad : 0;
    const bool steady_ok = carried && (!PROFILE || (fits_i8(kr.cmis) && fits_i8(kr.cmat) && apad >= 2)) &&
                           (!SAMEGO || kr.gox == kr.goy);
    // keep the two select constants resident in VGPRs (hipcc otherwise re-materialises them with
    // two v_mov per step, 8 % of the loop's VALU instructions)
    if (!PROFILE) asm volatile("" : "+v"(kr.cmis), "+v"(kr.cmat));

    if constexpr (BAND == 1 || FUNNEL) {
        // a problem the steady body does not take, or one beyond the sentinel's range, is left to the full kernel
        if (!(steady_ok && Ws2(n, m).total < kWsRange && n >= 2 && n <= kBandMaxLen && m <= kBandMaxLen)) {
            return;                                // (its word stays 0)
        }
    }
    const P1Lds lds(m, (int)sizeof(LC));
    LC* ocode = reinterpret_cast<LC*>(smem);
    int* prog = reinterpret_cast<int*>(smem + lds.oc_bytes);
    uint32_t* tbl = reinterpret_cast<uint32_t*>(smem + lds.tbl_off);
    const Ws2 ws(n, m);
    uint8_t* const ws_p = a.ws + a.ws_off[p];
    // Bottom rows (Ws2::rows): strip s reads row s and writes row s + 1.  All waves of a workgroup
    // share one CU and its L1, so the workgroup-scope release / acquire on the progress words (LDS)
    // is all the ordering these plain loads and stores need.
    int2* const row0p = reinterpret_cast<int2*>(ws_p + ws.row(0)) + 1;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // codes as the cells compare them: MODE 2 keeps them multiplied by the profile's row pitch
    const int code_shift = PROFILE ? 8 : 0;
    const LC pad_code = PROFILE ? (LC)((apad - 1) << 8) : (LC)~(LC)0;        // never a valid id
    stage_ocr_codes(ocode, a.o_codes, o0, m, code_shift, pad_code, tid, W * 64);
    for (int j = tid; j <= m; j += W * 64)
        row0p[j] = make_int2(raw_of(bnd_V_row0(c, j)) + xadj, raw_of(bnd_D_row0(c, j)));
    if (tid < 16) prog[tid] = 0;
    const uint32_t mis4 = (uint32_t)(kr.cmis & 0xFF) * 0x01010101u;
    if (PROFILE)                                   // (the pad code's row -- columns j <= 0 and j > m -- scores -128: see from_zero)
        for (int k = tid; k < W * apad * 64; k += W * 64) tbl[k] = ((k / 64) % apad == apad - 1) ? 0x80808080u : mis4;
    __syncthreads();

    uint32_t* const tblw = tbl + (size_t)wave * apad * 64;                   // this wave's profile
    const unsigned char* const tbl_lane = reinterpret_cast<const unsigned char*>(tblw) + lane * 4;

    // buffer descriptor of the problem's workspace, for the straight-line stores of the steady state
    // (inputs through readfirstlane: hipcc must be able to PROVE them wave-uniform, or it wraps every
    // buffer operation in a waterfall loop)
    const uint64_t wsa = reinterpret_cast<uint64_t>(ws_p);
    unsigned char* const ws_u = reinterpret_cast<unsigned char*>(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(wsa >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wsa));
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(ws_u, 0, kWsRange, 0x00020000);
    const int nstrips = ws.nstrips, ngroups = ws.ngroups;
    const int prev_wave = (wave + W - 1) % W;
    const int g_lo = (63 + SPG - 1) / SPG;
    // The steady loop runs from the group in which the last lane has started to the END of the strip:
    // a lane that has passed its last column goes on over pad columns (the profile's all-mismatch
    // entry), and what it computes there only ever reaches lanes that are past their last column
    // too (same column, one step later), bottom-row entries beyond column m (room for 8; never read
    // for a column > m) and checkpoint words of finished lanes (phase 2 masks them).  Only the 16
    // start-up groups need the predicated edge body (0.35 ms of the 0.7 ms the edges took).
    const int g_hi = (steady_ok && ws.total < kWsRange) ? ngroups : 0;
    // The 16 start-up groups of a strip, in which lanes start one step apart, through the STEADY body as well (MODE 2):
    // a lane that has not reached column 1 yet runs over virtual columns j <= 0, and what it computes there must leave
    // its column-0 boundary state in place -- D = H = b_i = -(1 + gex) i in the carried form (YG = H~ + goy = M^ at
    // column 0), dsave from the lane above.  It does: the pad code scores -128, so M^ = b_(i-1) - 128 <= b_i; the XG chain
    // of a virtual column starts from V = -2^28 (set below) and carries max(b_i' + gox) over rows i' < i, which is <= b_i
    // because b falls with i iff gex <= -1 (the condition); so D' = max3(M^, XG, YG) = YG = b_i, YG' = max(b_i + goy,
    // b_i) = b_i, and the D handed down by the DPP shift is the b of the lane above.  The bottom-row stores of lanes 31 /
    // 63 for columns j <= 0 land in the pad entries (beyond column m + 8) of the row before: never read.  Saves the
    // EXEC-predicated edge body (twice the cost per group) on 16 of a strip's groups: 1.5 % at 4096 columns, 3 % at 2048.
    const bool from_zero = PROFILE && g_hi > 0 && prm[4] <= -1;
    int pass = 0;
    // funnel: the ranges' source, and the wave's share of the problem's exit maximum and strip count (wave-uniform).
    // Whether the funnel's own ranges run is a property of the problem (funnel_ok: a loop over all its strips), so
    // nw_band_cert_init_kernel works it out once per problem and the waves only read the word.
    const FunnelSys fsys = funnel_sys(prm);
    bool fun_ok = false;
    if constexpr (FUNNEL) fun_ok = a.band_cert[kCertWords * p + 3] != 0;
    // BAND = 4: flag word 2 = nw_lcs_suffix_kernel left this problem's table, and the narrower ranges run; a problem it
    // declined runs the static funnel here (a count of matches no remainder can reach: SufL = Suf)
    bool lcs_on = false;
    if constexpr (LCS) lcs_on = a.band_cert[kCertWords * p + 3] == 2;
    auto strip_range = [&](int s_) {
        if constexpr (LCS)
            if (lcs_on) return funnel_raw<kFunnelLcsScalePm>(n, m, fsys, a.band_w, s_);
        return fun_ok ? funnel_raw(n, m, fsys, a.band_w, s_) : band_groups(n, m, a.band_w, s_);
    };
    auto exit_of = [&](int db_hat, int i, int j, int i2, int j2) {      // from cell (i, j), hatted, to the cell (i2, j2) outside
        return db_hat + prm[4] * i + prm[5] * j + fsys.ap + funnel_suf<int>(n - i2, m - j2, fsys);
    };
    const FunnelLcs lsys = funnel_lcs_sys(prm);
    const int32_t* const lcs_p = LCS && lcs_on ? a.lcs + (size_t)p * lcs_stride(a.lcs_max_n) : nullptr;
    auto exit_at = [&](int db_hat, int i, int j, int i2, int j2, int l) {   // the same with at most l matches to come
        if constexpr (LCS)
            return db_hat + prm[4] * i + prm[5] * j + fsys.ap + funnel_suf_lcs<int>(n - i2, m - j2, l, fsys, lsys);
        else return exit_of(db_hat, i, j, i2, j2);
    };
    int ex_wave = -(1 << 30), cnt_wave = 0;

    for (int s = wave; s < nstrips; s += W, ++pass) {
        // (lane_boundary<false>, nw_cell.h, spelled out)
        int D[R], V[R], H[R], tc[R];            // V, H hold XG, YG when the problem is carried
        const int row0 = s * L::SR + lane * R;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + r + 1;
            D[r] = raw_of(bnd_D_col0(c, i));
            H[r] = raw_of(bnd_H_col0(c, i)) + yadj;
            V[r] = from_zero ? -(1 << 28) : 0;
            tc[r] = (i <= n) ? a.t_codes[t0 + i - 1] : -1;
        }
        int dsave = raw_of(bnd_D_col0(c, row0));
        // banded: the strip's groups gl .. g_fin - 1; one that starts at gl > 0 starts from the sentinel state (its
        // checkpoint of group gl is what phase 2 restarts from, like any other)
        int gl = 0, g_fin = ngroups;
        if constexpr (BAND == 1) {
            const BandRange br = band_groups(n, m, a.band_w, s);
            gl = br.gl; g_fin = br.gh;
            if (gl > 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) D[r] = H[r] = V[r] = kBandSentinel;
                dsave = kBandSentinel;
            }
        }
        if constexpr (FUNNEL) {
            const BandRange br = strip_range(s);
            gl = br.gl; g_fin = br.gh;
            if (gl > 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) D[r] = H[r] = V[r] = kBandSentinel;
                dsave = kBandSentinel;
            }
            ++cnt_wave;
        }
        // the certificate: the lane that owns row n takes the inputs of cell (n, m) on its way into it (group_edge)
        const bool cert_strip = (BAND == 1 || FUNNEL) && s == nstrips - 1;
        const int cert_lane = ((n - 1) % L::SR) / R, cert_r = (n - 1) % R;
        // retire the transcript-code loads here: otherwise hipcc parks their s_waitcnt vmcnt(0) at
        // the first use INSIDE the group loop, where it also drains every checkpoint / row store
        // of the previous group
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" :: "v"(tc[r]));
        // MODE 2: patch the profile with this strip's matches
        auto patch = [&](bool set) {
            if (!PROFILE || !steady_ok) return;
            const uint32_t matb = (uint32_t)(kr.cmat & 0xFF);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (tc[r] < 0 || tc[r] >= apad - 1) continue;
                uint32_t w = mis4;
                if (set) {
#pragma unroll
                    for (int q = 0; q < R; ++q)
                        if (tc[q] == tc[r]) w = (w & ~(0xFFu << (8 * q))) | (matb << (8 * q));
                }
                tblw[tc[r] * 64 + lane] = w;
            }
        };
        patch(true);
        int tcmp[R];                             // transcript codes in the form the LDS codes have
#pragma unroll
        for (int r = 0; r < R; ++r) tcmp[r] = tc[r] << code_shift;           // -1 stays negative
        const bool lane_has_rows = row0 < n;
        const int prod_pass = (wave == 0) ? pass - 1 : pass;
        const int2* const hvd = reinterpret_cast<const int2*>(ws_p + ws.top(s)) + 1;       // the row above: entry j
        // the bottom row this lane writes if it is the last of its 16 (lanes 15, 31, 47: sub-strip rows for
        // phase 2; lane 63: the strip's own, which the next strip starts from)
        const bool sub_last = (lane & (kSubLanes - 1)) == kSubLanes - 1;
        int2* const hvo = reinterpret_cast<int2*>(ws_p + ws.row(s * kSubRows + (lane / kSubLanes) + 1)) + 1;

        auto wait_span = [&](int g_first) {
            if (W == 1 || s == 0) return;
            const int k_last = min((g_first + CHK + 1) * SPG - 1, L::nsteps(m) - 1);
            const int col = min(k_last + 1, m);
            const int need_groups = min(ngroups, (col + 62) / SPG + 1);
            const int need = prod_pass * ngroups + need_groups;
            wait_progress<__ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP, 2>(&prog[prev_wave], need);
        };
        // Progress words say "the bottom-row entries of these groups are in L2": the stores must have
        // COMPLETED, not merely been issued, before the word is written (a workgroup-scope release
        // only orders the LDS side on this target: it emits no vmcnt wait).
        auto publish = [&](int g) {
            if (W == 1) return;
            if ((g % CHK) == 0 || g == ngroups - 1) {     // published values are 1 mod CHK, like the needs
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 63)
                    __hip_atomic_store(&prog[wave], pass * ngroups + g + 1, __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
        int oc_next[SPG];
        int2 hd_next[SPG];
        auto load_group = [&](int g) {
            const int idx = kOPad + g * SPG - lane;
#pragma unroll
            for (int q = 0; q < SPG; ++q) {
                oc_next[q] = ocode[idx + q];
                hd_next[q] = hvd[min(g * SPG + q + 1, m)];
            }
        };
        auto prefetch = [&](int g) {
            if (g + 1 < ngroups) {
                if (((g + 1) % CHK) == 0) wait_span(g + 1);
                load_group(g + 1);
            }
        };
        // whole lane state, taken BEFORE group g runs: what phase 2 restarts from
        auto checkpoint_now = [&](int g) {
            int* st = reinterpret_cast<int*>(ws_p + ws.state(s, g / kCkGroups)) + lane;
#pragma unroll
            for (int r = 0; r < R; ++r) { st[r * 64] = D[r]; st[(R + r) * 64] = H[r]; }
            st[8 * 64] = V[R - 1];
            st[9 * 64] = dsave;
        };
        auto checkpoint = [&](int g) {
            if (g > 0 && (g % kCkGroups) == 0) checkpoint_now(g);
        };
        auto group_edge = [&](int g) {
            checkpoint(g);
            int oc[SPG];
            int2 hd[SPG];
#pragma unroll
            for (int q = 0; q < SPG; ++q) { oc[q] = oc_next[q]; hd[q] = hd_next[q]; }
            prefetch(g);
#pragma unroll
            for (int q = 0; q < SPG; ++q) {
                const int k = g * SPG + q;
                const int j = k - lane + 1;
                const bool active = (j >= 1) && (j <= m) && lane_has_rows;
                int v_up = hd[q].x, d_next = hd[q].y;
                wave_shr1_pair_sched(v_up, V[R - 1], d_next, D[R - 1]);
                if (active) {
                    // The certificate, at cell (n, m): the three values the cell takes its maximum of ARE M^, X^, Y^ of
                    // (n, m) in the carried form.  The walk starts there in the state PM(n, m) names (tb_start), a tag
                    // phase 1 does not form -- so all three have to clear the bound: M(n, m) makes that start state the
                    // reference's, and whichever state it is, its value makes the walk's pointers the reference's.
                    auto step = [&]() {
                        lane_step([&](int d_ul, int x_u, int y_l, int t, int o, int& d, int& x, int& y) {
                                      if (carried) cell_carried_hw(kr, d_ul, x_u, y_l, t, o, d, x, y);
                                      else cell_raw_hw(kr, d_ul, x_u, y_l, t, o, d, x, y); },
                                  D, V, H, dsave, v_up, d_next, tcmp, oc[q]);
                    };
                    if constexpr (BAND == 1 || FUNNEL) {
                        if (cert_strip && lane == cert_lane && j == m) {
                            const int d_ul = cert_r == 0 ? dsave : cert_r == 1 ? D[0] : cert_r == 2 ? D[1] : D[2];
                            const int tn = cert_r == 0 ? tc[0] : cert_r == 1 ? tc[1] : cert_r == 2 ? tc[2] : tc[3];
                            const int cert_m = d_ul + ((tn == a.o_codes[o0 + m - 1]) ? kr.cmat : kr.cmis);
                            const int cert_y = cert_r == 0 ? H[0] : cert_r == 1 ? H[1] : cert_r == 2 ? H[2] : H[3];
                            step();
                            // (the cell's upper input: XG of the row above after this step)
                            const int cert_x = cert_r == 0 ? v_up : cert_r == 1 ? V[0] : cert_r == 2 ? V[1] : V[2];
                            const int v0 = min(cert_m, min(cert_x, cert_y)) + prm[4] * n + prm[5] * m;   // un-hatted
                            // fail-closed: only this comparison, passed, keeps the full kernel off the problem
                            if constexpr (FUNNEL) a.band_cert[kCertWords * p] = v0;      // compared by nw_band_certify_kernel
                            else if (v0 > a.band_u[p]) a.band_ok[p] = 1;
                        } else {
                            step();
                        }
                    } else {
                        step();
                    }
                    if (sub_last) hvo[j] = make_int2(V[R - 1], D[R - 1]);
                }
            }
            publish(g);
        };

        int g = 0;
        if ((BAND == 1 || FUNNEL) && gl > 0) {
            g = gl;
            wait_span(gl);                            // the row above for the first block's groups
            if constexpr (FUNNEL) {
                // the left edge (nw_band.h, 2.): the row above, from the first column of R in it to column 4 gl + 2,
                // each towards the cell below it and, up to column 4 gl + 1, the one diagonally below
                const int gl_above = strip_range(s - 1).gl;
                const int c_lo = gl_above == 0 ? 1 : gl_above * SPG - 60;
                const int c_hi = min(m, gl * SPG + 2), i0 = s * L::SR + 1;
                int ex = -(1 << 30);
                // (BAND = 4: L of the border cell (i0 - 1, j) from the row nw_lcs_suffix_kernel left for this strip)
                const int32_t* const lrow = lcs_p ? lcs_p + lcs_row_off(a.lcs_max_n) + 192 * s : nullptr;
                for (int j = c_lo + lane; j <= c_hi; j += 64) {
                    const int db = hvd[j].y;
                    const int l = lrow ? lcs_row_at(lrow, m, j) : kBandMaxLen;
                    ex = max(ex, exit_at(db, i0 - 1, j, i0, j, l));
                    if (j + 1 <= c_hi) ex = max(ex, exit_at(db, i0 - 1, j, i0, j + 1, l));
                }
                ex_wave = max(ex_wave, wave_max_i32(ex));
                // lane 32's first step takes lane 31's state, the sentinel: phase 2 restarts the lower half-strip's first
                // chunk from lane 31's row, one column before the lane's first
                if (lane == 31) hvo[gl * SPG - 31] = make_int2(kBandSentinel, kBandSentinel);
            }
        } else {
            wait_span(0);
            load_group(0);
            const int e1 = from_zero ? 0 : min(g_lo, ngroups);
            for (; g < e1; ++g) group_edge(g);
        }

        int g_end = g_hi & ~3;                        // steady groups run in blocks of CHK = 4 (g_lo = 16)
        if constexpr (BAND == 1 || FUNNEL) {
            g_end = min(g_end, g_fin);                // (a multiple of 16, or ngroups)
            // (a strip that stops short of ngroups ends in the block loop, where its sentinel tail is written: g_fin is
            // then a multiple of 16 below ngroups, so g_end = g_fin here -- the replay in sim_nw_band.cpp writes the tail
            // on the same condition, g_fin < ngroups)
            // cell (n, m) goes through the edge body, which carries the certificate
            if (cert_strip) g_end = min(g_end, ((m - 1 + cert_lane) / SPG) & ~3);
        }
        if (g < g_end) {
            // ---- steady state: every lane is inside 1 <= j <= m, no EXEC changes.  Blocks of four
            // groups with two input buffers (A / B): the LDS prefetch of the next group lands in the
            // other buffer, no register copies at the back-edge, and everything that depends on the
            // group index -- progress wait and publish (once per block), checkpoint (every fourth
            // block), row / code addresses (running pointers) -- stays out of the groups.
            // MODE 2 reads the OCR codes one group further ahead (X / Y) and turns them into
            // profile entries when the group's other inputs are fetched. ----
            static_assert(CHK == 4 && SPG == 4, "the block loop is written for 4 groups of 4 steps");
            const int4* hrp = reinterpret_cast<const int4*>(hvd + (g * SPG + 1));   // next group's 4 entries (16-B aligned)
            // What lane 63 leaves behind per group -- four entries of the bottom row, two 16-byte
            // stores -- goes through a raw buffer descriptor of the problem's workspace with a per-lane
            // offset that is out of range for every other lane: the hardware drops those lanes'
            // stores, and the code stays STRAIGHT-LINE.  Under `if (lane == 63)` (a branch) hipcc cannot
            // count the stores, so its s_waitcnt for the next group's loads came out as vmcnt(2) and
            // made every group wait for its stores to be acknowledged.
            // The whole offset sits in the per-lane VGPR (+ an immediate per group of the block): with an
            // SGPR offset hipcc does not cover the store-data hazard of 16-byte buffer stores on this
            // chip (a VALU write to a data register in the two issue slots behind the store is what
            // gets stored; seen as ~12 % wrong first words when a second workgroup shares the CU).
            // (32-bit UNSIGNED arithmetic: kWsRange + any real offset < 2^32 wraps nowhere, and the sum is
            // >= kWsRange, i.e. out of the descriptor's range, for every lane but 63; g_hi != 0 only when
            // ws.total < kWsRange, so lane 63's own offsets are all in range)
            static_assert((uint64_t)kWsRange * 2 < (1ull << 32), "only63 + offset stays below 2^32");
            const uint32_t only63 = sub_last ? 0u : (uint32_t)kWsRange;           // in range for lanes 15, 31, 47, 63 only
            // entry j = k - lane + 1 of the lane's own bottom row (index j + 1)
            uint32_t vo_w = only63 + (uint32_t)(ws.row(s * kSubRows + (lane / kSubLanes) + 1) + 8 + (int64_t)(g * SPG - lane + 1) * 8);
            int crd = (kOPad + g * SPG - lane) * (int)sizeof(LC); // byte offset of the next group's codes (per lane)
            asm volatile("" : "+v"(crd));                         // a running VGPR pointer, immediate offsets below
            const unsigned char* const oc_b = reinterpret_cast<const unsigned char*>(ocode);
            const int need_cap = min(ngroups, (m + 62) / SPG + 1);
            const int need_base = prod_pass * ngroups;
            int inA[SPG], inB[SPG];              // MODE 1: OCR codes; MODE 2: packed scores of the 4 rows
            int2 hdA[SPG], hdB[SPG];
            int ocX[SPG], ocY[SPG];
            auto codes = [&](int (&oc)[SPG]) {                    // codes of the next group not yet read
#pragma unroll
                for (int q = 0; q < SPG; ++q) oc[q] = *reinterpret_cast<const LC*>(oc_b + crd + q * (int)sizeof(LC));
                crd += SPG * (int)sizeof(LC);
            };
            auto fetch = [&](const int (&oc)[SPG], int (&in)[SPG], int2 (&hd)[SPG]) {   // inputs of the next group
#pragma unroll
                for (int q = 0; q < SPG; ++q) {
                    if constexpr (PROFILE) in[q] = *reinterpret_cast<const int*>(tbl_lane + oc[q]);
                    else in[q] = oc[q];
                }
                const int4 e01 = hrp[0], e23 = hrp[1];
                hd[0] = make_int2(e01.x, e01.y); hd[1] = make_int2(e01.z, e01.w);
                hd[2] = make_int2(e23.x, e23.y); hd[3] = make_int2(e23.z, e23.w);
                hrp += 2;
            };
            auto wait_block = [&](int g_first) {                  // wait_span without the edge clamps
                if (W == 1 || s == 0) return;
                const int need = need_base + min(need_cap, g_first + CHK + 17);
                wait_progress<__ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP, 2>(&prog[prev_wave], need);
            };
            auto steady = [&](auto blk, const int (&in)[SPG], const int2 (&hd)[SPG]) {
                constexpr int B = decltype(blk)::value;           // group's place in the block: immediate offsets
                int bv[SPG], bd[SPG];
#pragma unroll
                for (int q = 0; q < SPG; ++q) {
                    int x_up = hd[q].x, d_next = hd[q].y;
                    wave_shr1_pair_sched(x_up, V[R - 1], d_next, D[R - 1]);
                    int d_ul = dsave, x_u = x_up;             // (lane_step, nw_cell.h, spelled out)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int d_old = D[r];
                        int mr;
                        if constexpr (PROFILE) mr = c_add_sbyte(d_ul, in[q], r);
                        else mr = d_ul + v_score(tc[r], in[q], kr.cmis, kr.cmat);
                        const int d = c_max3(mr, x_u, H[r]);
                        const int dgx = d + kr.gox;
                        const int dgy = SAMEGO ? dgx : d + kr.goy;
                        x_u = max(dgx, x_u);
                        H[r] = max(dgy, H[r]);
                        V[r] = x_u;
                        D[r] = d;
                        d_ul = d_old;
                    }
                    dsave = d_next;
                    bv[q] = V[R - 1]; bd[q] = D[R - 1];
                }
                typedef int v4i __attribute__((ext_vector_type(4)));
                // the strip's bottom row, by its owner
                __builtin_amdgcn_raw_buffer_store_b128((v4i){bv[0], bd[0], bv[1], bd[1]}, wsrc, (int)(vo_w + B * 32u), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128((v4i){bv[2], bd[2], bv[3], bd[3]}, wsrc, (int)(vo_w + B * 32u + 16u), 0, 0);
            };
            // (hvd of group g was waited for by the last edge group's prefetch)
            if constexpr (PROFILE) { codes(ocX); codes(ocY); fetch(ocX, inA, hdA); }
            else { codes(ocX); fetch(ocX, inA, hdA); }
            constexpr std::integral_constant<int, 0> blk0{};
            constexpr std::integral_constant<int, 1> blk1{};
            constexpr std::integral_constant<int, 2> blk2{};
            constexpr std::integral_constant<int, 3> blk3{};
            auto block = [&]() {                                  // four groups, g .. g + 3
                if constexpr (PROFILE) {
                    fetch(ocY, inB, hdB); codes(ocX); steady(blk0, inA, hdA);
                    fetch(ocX, inA, hdA); codes(ocY); steady(blk1, inB, hdB);
                    fetch(ocY, inB, hdB); codes(ocX); steady(blk2, inA, hdA);
                    wait_block(g + CHK);
                    fetch(ocX, inA, hdA); codes(ocY); steady(blk3, inB, hdB);
                } else {
                    codes(ocY); fetch(ocY, inB, hdB); steady(blk0, inA, hdA);
                    codes(ocX); fetch(ocX, inA, hdA); steady(blk1, inB, hdB);
                    codes(ocY); fetch(ocY, inB, hdB); steady(blk2, inA, hdA);
                    wait_block(g + CHK);
                    codes(ocX); fetch(ocX, inA, hdA); steady(blk3, inB, hdB);
                }
                // progress, one block late: this block issued 8 stores and 8 loads (16 vector-memory
                // operations, + 10 checkpoint stores in every fourth block), so once all but the 16
                // youngest are done, every store of the blocks before this one has completed -- without
                // waiting for the stores just issued.  Published: groups < g.
                vo_w += (uint32_t)(CHK * SPG * 8);
                if (W > 1) {
                    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    if (lane == 63)
                        __hip_atomic_store(&prog[wave], pass * ngroups + g, __ATOMIC_RELEASE,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                g += CHK;
            };
            // Checkpoint intervals whole, so that the ten
            // checkpoint stores sit in straight-line code: behind a branch hipcc's s_waitcnt for the
            // next loads can no longer count them and waits for all of them (a full store round trip
            // every 16 groups).
            static_assert(kCkGroups % CHK == 0, "interval = whole blocks");
            while (g < g_end && (g % kCkGroups) != 0) block();       // up to the first interval border (g_lo = 16)
            while (g + kCkGroups <= g_end) {
                checkpoint_now(g);
#pragma unroll
                for (int b = 0; b < kCkGroups / CHK; ++b) block();
            }
            while (g < g_end) {
                checkpoint(g);
                block();
            }
            if (g < g_fin) {
                if ((g % CHK) == 0) wait_span(g);
                load_group(g);
            } else {
                if constexpr (FUNNEL) {
                    if (g_fin < ngroups) {
                        // the right edge (nw_band.h, 1.): after the strip's last step the lane stands at column jr
                        const int jr = g_fin * SPG - lane;
                        int ex = -(1 << 30);
                        // (BAND = 4: one count for the lane's five border cells, L(row0, jr) -- the cell above them all
                        // in column jr, which every outside neighbour taken here dominates in both coordinates)
                        const int l = lcs_p && jr <= m && row0 < n ? lcs_p[64 * s + lane] : kBandMaxLen;
                        // (BAND = 4 leaves out lane 63's diagonal neighbour where the strip below holds it: the static
                        // funnel takes it regardless, which only raises its word)
                        bool diag_in = false;
                        if constexpr (LCS) {
                            const BandRange nx = strip_range(s + 1);
                            diag_in = lane == 63 && jr + 1 >= (nx.gl == 0 ? 1 : nx.gl * SPG + 3) && jr + 1 <= min(m, nx.gh * SPG);
                        }
                        if (jr <= m) {
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                const int i = row0 + 1 + r;
                                if (i > n) continue;
                                if (jr + 1 <= m) ex = max(ex, exit_at(D[r], i, jr, i, jr + 1, l));
                                if (jr + 1 <= m && i + 1 <= n && !(r == R - 1 && diag_in)) ex = max(ex, exit_at(D[r], i, jr, i + 1, jr + 1, l));
                                if (r == R - 1 && lane < 63 && i + 1 <= n) ex = max(ex, exit_at(D[r], i, jr, i + 1, jr, l));
                            }
                        }
                        if (jr + 1 <= m && row0 + 1 <= n) ex = max(ex, exit_at(dsave, row0, jr, row0 + 1, jr + 1, l));
                        ex_wave = max(ex_wave, wave_max_i32(ex));
                        // the sentinel tails: of lane 31's row, which the lower half-strip's last chunk reads one group
                        // past g_fin (lane 31 wrote up to column 4 g_fin - 31), and of the strip's last row, as for the band
                        int2* const row31 = reinterpret_cast<int2*>(ws_p + ws.row(s * kSubRows + 1)) + 1;
                        if (lane < 3 && g_fin * SPG - 30 + lane <= m)
                            row31[g_fin * SPG - 30 + lane] = make_int2(kBandSentinel, kBandSentinel);
                        int2* const rowp = reinterpret_cast<int2*>(ws_p + ws.row(s * kSubRows + kSubRows)) + 1;
                        const int c_hi = min(m, strip_range(s + 1).gh * SPG + 4);
                        for (int col = g_fin * SPG - 62 + lane; col <= c_hi; col += 64)
                            rowp[col] = make_int2(kBandSentinel, kBandSentinel);
                    }
                }
                if constexpr (BAND == 1) {
                    // Row hand-off past the band: the strip below runs further right than this one did, so the columns
                    // of this strip's last row it (and phase 2, for its chunks) reads beyond this strip's last group
                    // are given the sentinel; lane 63 wrote up to column 4 g_fin - 63.
                    // (a strip with g_fin < ngroups always ends HERE, in the block loop: g_fin is then a multiple of 16
                    // below ngroups, hence <= g_hi & ~3, and only the last strip -- g_fin = ngroups -- leaves the loop early)
                    if (g_fin < ngroups) {
                        int2* const rowp = reinterpret_cast<int2*>(ws_p + ws.row(s * kSubRows + kSubRows)) + 1;
                        const int c_hi = min(m, band_groups(n, m, a.band_w, s + 1).gh * SPG + 4);
                        for (int col = g_fin * SPG - 62 + lane; col <= c_hi; col += 64)
                            rowp[col] = make_int2(kBandSentinel, kBandSentinel);
                    }
                }
                if (W > 1) {                                 // the strip ended in the block loop: all of it is out
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane == 63)
                        __hip_atomic_store(&prog[wave], pass * ngroups + ngroups, __ATOMIC_RELEASE,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        for (; g < g_fin; ++g) group_edge(g);
        patch(false);
    }
    if constexpr (FUNNEL) {
        // the wave's share of the certificate: one atomic pair, after its last strip
        if (lane == 0 && cnt_wave > 0) {
            atomicMax(&a.band_cert[kCertWords * p + 1], ex_wave);
            atomicAdd(&a.band_cert[kCertWords * p + 2], cnt_wave);
        }
    }
}

// The funnel's certificate, one thread per problem, between the funnel launch and the fallback launch: the problem's
// workspace stands iff every strip was counted and v0 clears both the outer band's bound and the exit maximum.
// Fail-closed: v0 starts as INT32_MIN and the count as 0 (nw_band_cert_init_kernel), so a problem the funnel launch
// left alone, or left early, is filled again in full.  The fourth word is the fill's input: 1 if the funnel's own
// ranges run for the problem, 0 if the outer band's do (funnel_ok, the function the host's x0 was worked out under).
__global__ __launch_bounds__(256) void nw_band_cert_init_kernel(NwArgs a, const int32_t* x0) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nprob) return;
    const int n = (int)(a.t_off[p + 1] - a.t_off[p]), m = (int)(a.o_off[p + 1] - a.o_off[p]);
    const bool own = n > 0 && m > 0 && n <= kBandMaxLen && m <= kBandMaxLen &&
                     funnel_ok(n, m, funnel_sys(a.params + (size_t)p * a.params_stride), a.band_w);
    a.band_cert[kCertWords * p] = INT32_MIN;
    a.band_cert[kCertWords * p + 1] = x0[p];
    a.band_cert[kCertWords * p + 2] = 0;
    a.band_cert[kCertWords * p + 3] = own ? 1 : 0;
    a.band_ok[p] = 0;
}
__global__ __launch_bounds__(256) void nw_band_certify_kernel(NwArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nprob) return;
    const int n = (int)(a.t_off[p + 1] - a.t_off[p]);
    const int32_t* c = a.band_cert + kCertWords * (size_t)p;
    const bool ok = n > 0 && c[2] == PtrLayout<4>::nstrips(n) && c[0] > a.band_u[p] && c[0] > c[1];
    a.band_ok[p] = ok ? 1 : 0;
}

// ---- the LCS-bounded funnel (BAND = 4; bound, table layout and limits in nw_band.h) ----
// Which problems it covers is decided here, once per problem, from sizes, system and the batch's alphabet hint alone:
// flag word 2, the exit word at its floor (nw_lcs_suffix_kernel supplies the boundary's part, under the narrower ranges)
// and the strip count at -1, which the LCS kernel's last act raises to 0 -- a problem whose table was not finished
// cannot reach the full count and is filled again.  Every other problem is set up as nw_band_cert_init_kernel does.
__global__ __launch_bounds__(256) void nw_band_cert_init_lcs_kernel(NwArgs a, const int32_t* x0, int alphabet) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nprob) return;
    const int n = (int)(a.t_off[p + 1] - a.t_off[p]), m = (int)(a.o_off[p + 1] - a.o_off[p]);
    const int32_t* prm = a.params + (size_t)p * a.params_stride;
    const FunnelSys f = funnel_sys(prm);
    const bool sized = n > 0 && m > 0 && n <= kBandMaxLen && m <= kBandMaxLen;
    const bool lcs = sized && n >= 2 && m <= kLcsMaxM && n <= a.lcs_max_n && alphabet > 0 && alphabet <= kLcsMaxAlphabet &&
                     prm[0] > prm[1] && funnel_ok<kFunnelLcsScalePm>(n, m, f, a.band_w);
    const bool own = lcs || (sized && funnel_ok(n, m, f, a.band_w));
    a.band_cert[kCertWords * p] = INT32_MIN;
    a.band_cert[kCertWords * p + 1] = lcs ? -(1 << 30) : x0[p];
    a.band_cert[kCertWords * p + 2] = lcs ? -1 : 0;
    a.band_cert[kCertWords * p + 3] = lcs ? 2 : own ? 1 : 0;
    a.band_ok[p] = 0;
}

// L(i, j) = LCS(T[i+1..n], O[j+1..m]) where the fill's exit bound reads it, one wave per problem.  Bit-parallel row
// recurrence (Hyyro / Crochemore) on the REVERSED strings: row r has consumed T[n], .., T[n-r+1] and its bit c - 1 is
// CLEAR where the LCS against O[m], .., O[m-c+1] grows at column c, so L(n - r, m - c) = the clear bits among its first c:
//     V' = (V + (V & M)) | (V & ~M),  M = the columns that match the row's symbol.
// Lane l owns bits 64 l .. 64 l + 63.  The rows run skewed -- at step t lane l is in row t - l + 1 -- so the add's
// carry into a lane is the carry out of its neighbour one step earlier: one DPP shift, no carry resolve across the wave.
// The row's symbol (as the byte offsets of its masks) and the running count of clear bits travel the same way.  Match
// masks in LDS, TWO-LEVEL (nw_band.h: lcs_mask_rows, lcs_mask_offsets): M(c) = A[c >> 3] & B[c & 7], rows [lane] (bank =
// lane), 13 rows at alphabet 27 where one row per symbol took 28.  That is what the kernel's time hangs on: it is the
// latency of one wave (the SIMDs are far from saturated), one row per symbol let LDS hold 10 one-wave workgroups per CU,
// and the 4096 waves of a 4096-problem batch -- 16 per CU -- ran in two rounds.  At 10 240 B or less (every alphabet the
// kernel takes) all 16 are resident at once; a step pays two LDS reads and three VALU more for it (two address adds on
// the halves of the packed offsets instead of one, and the AND's two halves), a lone wave about 5 % of its time.  Lanes
// outside rows 1 .. n run the pad symbol, whose A row is all zero: M = 0 leaves V, the carry (0) and the count as they
// are, and no lane is predicated.
// What is stored is scalar-scheduled (one store step in flight at a time) and laid out of the steps' line, so a step
// pays one scalar compare and an untaken branch for it:
//   edge[64 s + l] = L(256 s + 4 l, 4 gh(s) - l), strips with gh < ngroups -- the right edge's count per lane;
//   rows i = 256 s whole (bits complemented: set = growth; counts of the words before) -- the left edge's, and row 0;
//   and the boundary's share of the exit word, which funnel_exit0 supplies for the static funnel: column 0 in blocks of
//   64 rows under the count of the block's tallest suffix, row 0 exactly.
#ifndef TA_LCS_PROFILE
#define TA_LCS_PROFILE 0    // counter ticks per problem (mask set-up, steps, stores, chunk tail) into the spare words
#endif                      // behind its edge counts (tools/lcs_profile.py); off: the instruction stream is the shipped one
#if TA_LCS_PROFILE
#define LCS_PROFILE_DECL long long pc_t = __builtin_readcyclecounter(), pc_setup = 0, pc_steps = 0, pc_events = 0, pc_tail = 0;
#define LCS_LAP(acc) { const long long now_ = __builtin_readcyclecounter(); acc += now_ - pc_t; pc_t = now_; }
#else
#define LCS_PROFILE_DECL
#define LCS_LAP(acc)
#endif
constexpr int kLcsUnroll = 3;                     // steps per loop iteration, a divisor of 63
static_assert(63 % kLcsUnroll == 0, "nw_lcs_suffix_kernel: 63 steps in whole iterations, the 64th swaps the feed");
__global__ __launch_bounds__(64) void nw_lcs_suffix_kernel(NwArgs a, int alphabet) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int p = blockIdx.x;
    if (a.band_cert[kCertWords * p + 3] != 2) return;
    const int64_t t0 = a.t_off[p], o0 = a.o_off[p];
    const int n = (int)(a.t_off[p + 1] - t0), m = (int)(a.o_off[p + 1] - o0);
    const int32_t* prm = a.params + (size_t)p * a.params_stride;
    const FunnelSys fsys = funnel_sys(prm);
    const FunnelLcs lsys = funnel_lcs_sys(prm);
    const int lane = threadIdx.x;
    const int nstrips = PtrLayout<4>::nstrips(n), ngroups = PtrLayout<4>::ngroups(m);
    const int mask_rows = lcs_mask_rows(alphabet);                           // A[hi], the pad row that stays 0, B[lo]: nw_band.h
    uint64_t* const mask = reinterpret_cast<uint64_t*>(smem);                // [mask_rows][64]
    int* const rg = reinterpret_cast<int*>(smem + (size_t)mask_rows * kLcsMaskRowBytes);   // (gl, gh) per strip
    unsigned char* const mask_lane = smem + lane * 8;
    int32_t* const out = a.lcs + (size_t)p * lcs_stride(a.lcs_max_n);
    int32_t* const rows = out + lcs_row_off(a.lcs_max_n);
    LCS_PROFILE_DECL

    for (int k = 0; k < mask_rows; ++k) mask[k * 64 + lane] = 0;
    for (int b0 = 0; b0 < 64; b0 += 16) {                                   // (16 loads in flight, then their 16 bits)
        int syms[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = 64 * lane + b0 + k;                                // reversed column c + 1 = O[m - c]
            syms[k] = c < m ? a.o_codes[o0 + m - 1 - c] : -1;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {                                       // a bit into two rows, each one LDS OR that returns
            const uint32_t off = lcs_mask_offsets(syms[k], alphabet);        // nothing; outside the alphabet: 0 into the pad's
            const uint64_t bit = (unsigned)syms[k] < (unsigned)alphabet ? 1ull << (b0 + k) : 0;
            __hip_atomic_fetch_or(reinterpret_cast<uint64_t*>(mask_lane + (off >> 16)), bit, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(reinterpret_cast<uint64_t*>(mask_lane + (off & 0xffffu)), bit, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    for (int s = lane; s < nstrips; s += 64) {
        const BandRange r = funnel_raw<kFunnelLcsScalePm>(n, m, fsys, a.band_w, s);
        rg[2 * s] = r.gl; rg[2 * s + 1] = r.gh;
    }
    for (int k = lane; k < 64 * nstrips; k += 64) out[k] = 0;               // rows at or past n: nothing to come
    __threadfence();                                                         // (before the events' stores to the same words)
    __syncthreads();
    auto is_out = [&](int i, int j) {                                        // an interior cell outside R (funnel_exit0's)
        if (i < 1 || i > n || j < 1 || j > m) return false;
        const BandRange r{rg[2 * ((i - 1) / 256)], rg[2 * ((i - 1) / 256) + 1]};
        return j < funnel_jlo(r, i) || j > funnel_jhi(r, i, m);
    };
    auto exit0 = [&](int db, int i2, int j2, int l) {
        return db + fsys.ap + funnel_suf_lcs<int>(n - i2, m - j2, l, fsys, lsys);
    };

    // What the steps store, scalar-scheduled: nx_t is the next step with a store, and the steps compare with nothing else.
    //   the right edge's counts, in RUNS (nw_band.h: lcs_next_run): inside a run the next one is 4 steps on, one lane's
    //   entry and one bit down; a new run is fetched about twice per strip;
    //   the rows 256 s from the last strip's: row i passes lane d at step n - i - 1 + d, 64 steps in every 256.
    LcsRunCursor ev_c = lcs_run_begin(n);
    int ev_t, ev_n, ev_w, ev_b, ev_k;                                        // (ev_k = 64 s + l, the entry)
    auto next_run = [&]() __attribute__((always_inline)) {
        const LcsRun r = lcs_next_run(n, m, ngroups, ev_c, [&](int s) { return __builtin_amdgcn_readfirstlane(rg[2 * s + 1]); });
        ev_t = r.t0; ev_n = r.count; ev_w = r.w; ev_b = r.b; ev_k = 64 * r.s + r.l;
    };
    next_run();
    int row_t = n - 256 * (nstrips - 1) - 1, row_d = 0;                      // the next row store: its step and lane
    int32_t* row_p = rows + 192 * (nstrips - 1);
    int nx_t = min(ev_t, row_t);

    // Per step: three DPP shifts, the two LDS reads of the symbol's rows (issued a step ahead: the symbols do not wait
    // for the arithmetic; each address is the lane's plus one half of the packed offsets, one SDWA add), their AND, the
    // 64-bit recurrence with its carry out, and the running count -- of SET bits, which is two v_bcnt: the clear bits
    // before lane l are 64 l less the count that arrives.
    const int pad = (int)lcs_mask_pad(alphabet);
    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    typedef __attribute__((address_space(3))) const uint64_t lds_word;
    // (the lane's LDS address as a number: the rows' base is then in it once, not added per read)
    const uint32_t lane8 = (uint32_t)(uintptr_t)(lds_byte*)smem + lane * 8;
    auto row_a = [&](int pk) { return *(lds_word*)(uintptr_t)(((uint32_t)pk >> 16) + lane8); };
    auto row_b = [&](int pk) { return *(lds_word*)(uintptr_t)(((uint32_t)pk & 0xffffu) + lane8); };
    auto load_feed = [&](int base) {            // the 64 symbols lane 0 starts from step base on: row base + k + 1 = T[n - base - k]
        const int tk = n - 1 - base - lane;
        return tk >= 0 ? (int)lcs_mask_offsets(a.t_codes[t0 + tk], alphabet) : pad;
    };
    uint64_t V = ~0ull;
    int cy = 0, nc = 0, ex = -(1 << 30);
    // lane 0's next symbols: `feed` rotates one lane down per step (wave_rol:1), so that lane 0 holds the symbol of the
    // step after the one in flight; every 64 steps the next 64 are loaded (a chunk ahead)
    int feed = load_feed(0);
    int symn = __builtin_amdgcn_update_dpp(feed, pad, 0x138, 0xf, 0xf, false);   // step 0: lane 0 its own, the others the pad
    uint64_t An = row_a(symn), Bn = row_b(symn);
    const int nchunks = (n + 63 + 63) / 64;
    LCS_LAP(pc_setup)
    // the stores of step t, out of the steps' line: V and nin are the owning lane's after the step
    auto stores = [&](int t, int nin) __attribute__((always_inline)) {
        LCS_LAP(pc_steps)
        if (t == ev_t) {
            if (lane == ev_w) out[ev_k] = 64 * ev_w - nin + __builtin_popcountll(~V & ((1ull << ev_b) - 1));
            if (--ev_n > 0) { ev_t += 4; --ev_k; --ev_b; } else next_run();
        }
        if (t == row_t) {
            if (lane == row_d) {
                reinterpret_cast<uint64_t*>(row_p)[lane] = ~V;
                row_p[128 + lane] = 64 * lane - nin;
            }
            ++row_t;
            if (++row_d == 64) {                                             // on to row i - 256, 256 steps after this one's first
                row_d = 0; row_t += 192; row_p -= 192;
                if (row_p < rows) row_t = INT32_MAX;
            }
        }
        nx_t = min(ev_t, row_t);
        LCS_LAP(pc_events)
    };
    auto step = [&](int t) __attribute__((always_inline)) {
        const int sym = symn;
        const uint64_t M = An & Bn;
        symn = __builtin_amdgcn_update_dpp(feed, sym, 0x138, 0xf, 0xf, false);    // (lane 0 keeps feed's: the next symbol)
        An = row_a(symn); Bn = row_b(symn);
        const int cin = __builtin_amdgcn_update_dpp(0, cy, 0x138, 0xf, 0xf, true);
        const int nin = __builtin_amdgcn_update_dpp(0, nc, 0x138, 0xf, 0xf, true);
        const uint64_t U = V & M;
        const uint64_t sum = V + U + (uint64_t)(unsigned)cin;
        // carry out of a + b + c at the top bit: b's bit where the sum's is set, a's where it is clear (U is a subset of V)
        const uint32_t sh = (uint32_t)(sum >> 32), uh = (uint32_t)(U >> 32), vh = (uint32_t)(V >> 32);
        cy = (int)(((sh & uh) | (~sh & vh)) >> 31);
        V = sum | (V & ~M);
        nc = nin + __builtin_popcountll(V);
        if (__builtin_expect(t == nx_t, 0)) stores(t, nin);
    };
    for (int ch = 0; ch < nchunks; ++ch) {
        const int base = ch * 64;
        const int feed_next = load_feed(base + 64);
        LCS_LAP(pc_tail)
#pragma unroll 1
        for (int q = 0; q < 63; q += kLcsUnroll) {                           // (kept small: the code must stay in the instruction cache)
#pragma unroll
            for (int k = 0; k < kLcsUnroll; ++k) {
                feed = __builtin_amdgcn_update_dpp(feed, feed, 0x134, 0xf, 0xf, false);   // wave_rol:1
                step(base + q + k);
            }
        }
        feed = feed_next;
        step(base + 63);
        LCS_LAP(pc_steps)
        // column 0 of the boundary: lane 63 has finished row min(base + 1, n); its count bounds L(i, 0) of the rows r =
        // base + 1 - k, k = lane, which consumed no more
        const int ltot = 64 * 64 - __builtin_amdgcn_readlane(nc, 63);
        const int r = base + 1 - lane, i = n - r;
        if (r >= 0 && r <= n) {
            if (is_out(i, 1)) ex = max(ex, exit0(-i, i, 1, ltot));
            if (is_out(i + 1, 1)) ex = max(ex, exit0(-i, i + 1, 1, ltot));
        }
    }
    LCS_LAP(pc_tail)
    const int pc = 64 * (lane + 1) - nc;                                      // clear bits up to and with this lane's word
    // row 0 of the boundary, from the finished table row: cell (0, j) towards (1, j) and (1, j + 1)
    {
        const int before = pc - __builtin_popcountll(~V);                    // clear bits in the words before this lane's
        for (int b = 0; b < 64; ++b) {
            const int cnt = 64 * lane + b, j = m - cnt;                      // L(0, j) = clear bits among the first cnt
            if (j < 0) break;
            const int l = before + (b ? __builtin_popcountll(~V & ((1ull << b) - 1)) : 0);
            if (is_out(1, j)) ex = max(ex, exit0(-j, 1, j, l));
            if (is_out(1, j + 1)) ex = max(ex, exit0(-j, 1, j + 1, l));
        }
    }
    ex = wave_max_i32(ex);
    if (lane == 0) {
        atomicMax(&a.band_cert[kCertWords * p + 1], ex);
        __threadfence();
        atomicAdd(&a.band_cert[kCertWords * p + 2], 1);
#if TA_LCS_PROFILE
        const int spare = 64 * PtrLayout<4>::nstrips(a.lcs_max_n);           // (edge counts end here, the rows start at lcs_row_off)
        if (lcs_row_off(a.lcs_max_n) - spare >= 8) {
            long long* const pc = reinterpret_cast<long long*>(out + spare);
            pc[0] = pc_setup; pc[1] = pc_steps; pc[2] = pc_events; pc[3] = pc_tail;
        }
#endif
    }
}

// ---------------------------------------------------------------------------------------------
// phase 2
// One wave per problem walks back strip by strip, and inside a strip CHUNK by chunk (a chunk =
// the kCkGroups groups between two state checkpoints).  For the chunk the walk is in, the wave
// re-runs the TAGGED cell from the chunk's checkpoint -- straight into LDS: the chunk's pointer
// bytes (16 KiB) never go to memory -- walks them, and steps to the chunk before when the walk
// reaches the chunk's first two steps (the restart state carries no winner tags; two steps later
// every input of a cell has been produced with tags).  Those two steps belong to the chunk before,
// whose re-fill therefore runs one group further (17 groups).
//
// Four kernels do this -- one wave per problem on strips (nw_trace2_kernel), two problems per wave on
// half-strips (nw_trace2h_kernel), and each of those with several waves re-filling ahead of the walk
// (nw_trace2w_kernel, nw_trace2hw_kernel) -- out of ONE set of building blocks, parametrised by the
// lanes UL of the UNIT a re-fill restarts: 64 for a strip, 32 for a half-strip.  A unit has 4 UL rows;
// row x is in unit u = (x - 1) / (4 UL), which is lanes lb .. lb + UL - 1 of strip s (TbUnit).  A thread
// is lane lam of its unit and strip lane lb + lam.
constexpr int kChunk = kCkGroups;                 // groups per chunk
constexpr int kChunkGroups = kChunk + 1;          // + the group holding the next chunk's two halo steps
constexpr int kChunkSteps = kChunkGroups * 4;
// Lanes of a chunk whose pointer bytes are kept.  The walk enters a chunk at a lane l and only ever
// moves to smaller lanes (a step up is a quarter of a lane, a step left none), a quarter lane per
// alignment column at most: the 64 .. 68 skewed steps of a chunk take a diagonal path across ~13 lanes.
// Keeping lanes l - 31 .. l instead of all 64 halves the chunk's LDS (10.1 KB per wave with the ops
// staging buffer gone: the walk writes its columns straight to memory), i.e. SIXTEEN traceback waves per
// CU instead of eight -- the 16 problems a CU gets at 4096 problems are then all resident at once.  A walk
// that does run off the window's top lane (a long run of transcript-side gaps) re-fills the same chunk,
// up to the group it stands in, with the window moved to its lane.
#ifndef TA_TB2_LANES
#define TA_TB2_LANES 32
#endif
constexpr int kWinLanes = TA_TB2_LANES;
static_assert(kWinLanes >= 8 && kWinLanes <= 64, "window lanes");
constexpr int kHalfLanes = 32;
static_assert(kSubRows == 2 && kSubLanes == kHalfLanes, "nw_trace2h_kernel restarts half-strips: phase 1 must keep lane 31's rows");

#ifndef TA_P2_PROFILE
#define TA_P2_PROFILE 0     // cycle counters per problem into row 0 of its workspace (tools/p2_profile.py)
#endif
#if TA_P2_PROFILE
#define PC_LAP(acc) { const long long now_ = __builtin_readcyclecounter(); acc += now_ - pc_t; pc_t = now_; }
#else
#define PC_LAP(acc)
#endif

// one wave's (or half-wave's) LDS writes followed by its own lanes' reads: the LDS executes a wave's operations in
// order; this only keeps the compiler from moving them across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One problem of the batch as phase 2 sees it.  `alive` is false in the idle half of an odd batch's last wave (two
// problems per wave): p is then some real problem's index and the sizes are zero.
struct TbProblem {
    int p;
    bool alive;
    const int32_t *t_codes, *o_codes;
    int64_t t0, o0;
    int n, m;
    uint8_t* ops;
    int cap;
    const int32_t* prm;
    CellConsts c;
    CellRegs kr;
    // phase 1 leaves V~ + gox / H~ + goy in its checkpoints and bottom rows when the gap opens are
    // non-positive (carried cell), and the chunks are then re-filled in that form too
    bool carried;
    int xadj6, yadj6;
    Ws2 ws;
    uint8_t* ws_p;
    __device__ __forceinline__ TbProblem(const NwArgs& a, int p_, bool alive_)
        : p(p_), alive(alive_), t_codes(a.t_codes), o_codes(a.o_codes), t0(a.t_off[p_]), o0(a.o_off[p_]),
          n(alive_ ? (int)(a.t_off[p_ + 1] - t0) : 0), m(alive_ ? (int)(a.o_off[p_ + 1] - o0) : 0),
          ops(a.ops_out + a.ops_off[p_]), cap(n + m), prm(a.params + (size_t)p_ * a.params_stride),
          c(make_consts(prm[0], prm[1], prm[2], prm[3], prm[4], prm[5])),
          kr{c.cmismatch, c.cmatch, c.gox6, c.goy6, ~kTagMask}, carried(opens_nonpositive(c.gox, c.goy)),
          xadj6((carried ? c.gox : 0) * 64), yadj6((carried ? c.goy : 0) * 64), ws(max(n, 1), max(m, 1)),
          ws_p(a.ws + a.ws_off[p_]) {}
};

// Position and state of a walk between two chunks.
// The bottom rows of phase 1 carry no winner tags, so the two pointers a unit's first row takes
// from the row above (PM, PX) are not in a re-filled window.  A step that leaves the unit
// upwards is taken with its next state PENDING (pend = 3: the tag of D, = 4: the tag of XG / V~,
// of the cell (x, y) the walk then stands on -- bottom row of the unit above), and the state is
// read off that cell's tagged outputs (hvb) when the unit above is re-filled.
struct TbWalk { int x, y, st, len, pend, first, probe; };     // first, probe: 0 / 1

// the start of the walk (textSeqCompare.py:100-107) on units of UL lanes
template <int UL>
__device__ __forceinline__ TbWalk tb_start(int n, int m) {
    TbWalk w{n, m, 0, 0, 0, 1, 0};
    if (n > 1 && (n - 1) % (4 * UL) == 0) {                     // the start state PM(n, m) is a tag of the unit above: D(n-1, m-1)
        if (m == 1) w.first = 0;                                // boundary column: M
        else { w.x = n - 1; w.y = m - 1; w.pend = 3; w.probe = 1; }
    }
    return w;
}

// the end of the walk: the boundary runs from (x, y) and the length; returns the length
__device__ __forceinline__ int tb_finish(const NwArgs& a, const TbProblem& P, int x, int y, int len, bool writer) {
    while (y > 0) { if (writer) P.ops[P.cap - 1 - len] = 2; ++len; --y; }
    while (x > 0) { if (writer) P.ops[P.cap - 1 - len] = 1; ++len; --x; }
    if (P.alive && writer) a.ops_len[P.p] = len;
    return len;
}

// A chunk job: unit, chunk, last group to re-fill, steps of that group (1..4); u < 0: none.
struct TbJob { int u, ck, gtop, tops; };
__device__ __forceinline__ TbJob tb_prev_job(const TbJob& j) {
    // the chunk before, entered through its halo: groups up to the first group of the chunk just left, two steps of it
    if (j.u < 0 || j.ck < 1) return TbJob{-1, 0, 0, 0};
    return TbJob{j.u, j.ck - 1, j.ck * kChunk, 2};
}
template <int UL>
__device__ __forceinline__ TbJob tb_job_at(int x, int y) {
    if (x <= 0 || y <= 0) return TbJob{-1, 0, 0, 0};
    const int l = ((x - 1) % 256) / 4, k = (y - 1) + l;
    int ck = (k >> 2) / kChunk;
    // the first two steps of a chunk carry no valid tags: they belong to the chunk before, whose re-fill runs
    // one group further (the one-wave kernel finds that out by a walk of zero steps)
    if (ck > 0 && k < ck * kChunk * 4 + 2) ck -= 1;
    return TbJob{(x - 1) / (4 * UL), ck, k >> 2, (k & 3) + 1};
}
// The job d iterations after the one that starts at (x, y) as job j, if the path keeps to the diagonal: chunk after
// chunk through the halo while the unit lasts (k falls by 5/4 per diagonal step: a column and a quarter lane), then
// the chunk of the unit above that the diagonal enters -- with two groups of margin on its entry group, whole groups:
// a re-fill that went further than the walk's entry point serves it as well (tb_serves).
template <int UL>
__device__ __forceinline__ TbJob tb_predict(int x, int y, TbJob j, int d) {
    for (; d > 0 && j.u >= 0; --d) {
        const int l = ((x - 1) % 256) / 4, k = (y - 1) + l;
        const int to_top = x - j.u * (4 * UL);                   // diagonal steps until the walk leaves the unit
        const int to_halo = j.ck > 0 ? ((k - (j.ck * kChunk * 4 + 1)) * 4 + 4) / 5 : (1 << 28);
        if (to_halo < to_top) {
            x -= to_halo; y -= to_halo;
            j = (y > 0) ? tb_prev_job(j) : TbJob{-1, 0, 0, 0};
        } else {
            x -= to_top; y -= to_top;
            j = tb_job_at<UL>(x, y);
            if (j.u >= 0) { j.gtop = min(j.gtop + 2, j.ck * kChunk + kChunk); j.tops = 4; }
        }
    }
    return j;
}
// a window re-filled for `spec` holds everything the walk of job `j` reads: same chunk, re-filled at least as far
__device__ __forceinline__ bool tb_serves(const TbJob& spec, const TbJob& j) {
    return spec.u >= 0 && spec.u == j.u && spec.ck == j.ck &&
           (spec.gtop > j.gtop || (spec.gtop == j.gtop && spec.tops >= j.tops));
}

// What a wave hands to the wave of the next iteration: the walk, whether it is over, and the job it needs next.
struct TbTok { TbWalk w; int done; TbJob job; };
constexpr int kTokInts = 10;                                  // in LDS: x, y, st, len, pend, flags (1 first, 2 probe, 4 done), job
__device__ __forceinline__ TbTok tok_load(const int* tk) {
    TbTok t;
    t.w = TbWalk{tk[0], tk[1], tk[2], tk[3], tk[4], tk[5] & 1, (tk[5] >> 1) & 1};
    t.done = (tk[5] >> 2) & 1;
    t.job = TbJob{tk[6], tk[7], tk[8], tk[9]};
    return t;
}
__device__ __forceinline__ void tok_store(int* tk, const TbTok& t) {
    tk[0] = t.w.x; tk[1] = t.w.y; tk[2] = t.w.st; tk[3] = t.w.len; tk[4] = t.w.pend;
    tk[5] = t.w.first | (t.w.probe << 1) | (t.done << 2);
    tk[6] = t.job.u; tk[7] = t.job.ck; tk[8] = t.job.gtop; tk[9] = t.job.tops;
}

// The LDS of one re-fill (a wave's, or a half-wave's):
struct TbLds {
    uint4* win;         // pointer bytes of the chunk: [group - g0][lane - l_lo], WL lanes per group
    int2* hvt;          // (V~ or XG, D) of the row above the unit, step k at [k + 1 - k0] (column k + 1 - lb)
    int2* hvb;          // tagged (V~ or XG, D) the unit's bottom row puts out, per step
    uint16_t* ow;       // OCR codes, o index (k0 - lb - (UL - 1)) + i
};

// Unit u of a problem, for lane lam of it: where it lies, the lane's transcript codes and the row above the unit.
template <int UL>
struct TbUnit {
    int u, s, lb, i_h, row0;                    // unit, strip, first strip lane, 1-based index of the row above, the lane's row above
    bool lane_has_rows;
    int tc[4];
    const int2* hrow;                           // the row above: entry j
    __device__ __forceinline__ TbUnit(const TbProblem& P, int u_, int lam) : u(u_) {
        s = u / (64 / UL);
        lb = u % (64 / UL) * UL;
        i_h = u * (4 * UL);
        row0 = s * 256 + (lb + lam) * 4;
        lane_has_rows = row0 < P.n;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = row0 + rr + 1;
            tc[rr] = (i <= P.n) ? P.t_codes[P.t0 + i - 1] : -1;
        }
        hrow = reinterpret_cast<const int2*>(P.ws_p + P.ws.row(u * UL / kSubLanes)) + 1;
    }
};

// Inputs of a chunk's re-fill, fetched into registers: the OCR codes, the row above the unit for columns
// k0 - lb .. min(m, k0 - lb + steps) (tagged only where the tags are known analytically: the table's boundary row
// and column) and the lane state at the chunk's first group.  fetch() requests them, store() puts them where the
// re-fill reads them (LDS; the lane state in registers).  The one-wave and pair kernels fetch the next chunk's between
// the two: the chunk after this one is nearly always the one before it in the same unit, whole, so its inputs are
// requested as soon as this chunk's are in LDS and arrive under this chunk's re-fill and walk.
template <int UL>
struct ChunkIn {
    static constexpr int kOwIt = (kChunkSteps + UL + UL - 1) / UL, kRowIt = (kChunkSteps + 1 + UL - 1) / UL;
    int ow[kOwIt], st[kStateInts];
    int2 row[kRowIt];
    int ck = -1, gtop = -1;                                     // what the registers hold (of this unit)
    __device__ __forceinline__ void fetch(const TbProblem& P, const TbUnit<UL>& U, int lam, int ck_, int gtop_) {
        const int g0 = ck_ * kChunk, k0 = g0 * 4, jlo = k0 - U.lb;
        const int nsteps = (gtop_ - g0 + 1) * 4;
#pragma unroll
        for (int it = 0; it < kOwIt; ++it) {
            const int src = jlo - (UL - 1) + it * UL + lam;
            ow[it] = (src >= 0 && src < P.m) ? P.o_codes[P.o0 + src] : 0xFFFF;
        }
        const int jhi = min(P.m, jlo + nsteps);
#pragma unroll
        for (int it = 0; it < kRowIt; ++it) {
            const int jj = min(jlo + it * UL + lam, jhi);
            // (below 0 only in a unit whose first lane lb > 0 starts that many steps after the chunk's first)
            const int j = UL < 64 ? max(jj, 0) : jj;
            if (U.u == 0) row[it] = make_int2(bnd_V_row0(P.c, j) + P.xadj6, bnd_D_row0(P.c, j));
            else {
                const int2 e = U.hrow[max(jj, 1)];
                row[it] = (UL < 64 ? jj <= 0 : jj == 0) ? make_int2(0, bnd_D_col0(P.c, U.i_h)) : make_int2(enc_of(e.x), enc_of(e.y));
            }
        }
        if (g0 > 0) {
            const int* stp = reinterpret_cast<const int*>(P.ws_p + P.ws.state(U.s, g0 / kCkGroups)) + U.lb + lam;
#pragma unroll
            for (int q = 0; q < kStateInts; ++q) st[q] = stp[q * 64];
        }
        ck = ck_; gtop = gtop_;
    }
    // (a) OCR codes of the chunk, (b) the row above the unit, into LDS; (c) the lane state at the start of group g0
    // (in the form the re-fill keeps: carried or not) into D, V, H, dsave
    __device__ __forceinline__ void store(const TbProblem& P, const TbUnit<UL>& U, int lam, int ck_, int gtop_,
                                          const TbLds& lds, int (&D)[4], int (&V)[4], int (&H)[4], int& dsave) const {
        constexpr int R = 4;
        const int g0 = ck_ * kChunk, k0 = g0 * 4, jlo = k0 - U.lb;
        const int nsteps = (gtop_ - g0 + 1) * 4;
#pragma unroll
        for (int it = 0; it < kOwIt; ++it) {
            const int i = it * UL + lam;
            if (i < nsteps + UL) lds.ow[i] = (uint16_t)ow[it];
        }
        const int jhi = min(P.m, jlo + nsteps);
#pragma unroll
        for (int it = 0; it < kRowIt; ++it) {
            const int jj = jlo + it * UL + lam;
            if (jj <= jhi) lds.hvt[jj - jlo] = row[it];
        }
        lane_boundary<true>(P.c, U.row0, P.yadj6, 0, D, V, H, dsave);
        // a lane that has not started by the chunk's first step (strip lane >= k0: first chunks of a strip
        // when the interval is shorter than 64 steps) keeps the boundary values above: the scores are
        // the same, and only this form carries the column-0 tags the lane's first cells point to
        static_assert(kStateInts == 2 * R + 2, "state = D[R], H[R], V[R-1], dsave");
        if (g0 > 0 && U.lb + lam < k0) {
#pragma unroll
            for (int rr = 0; rr < R; ++rr) { D[rr] = enc_of(st[rr]); H[rr] = enc_of(st[R + rr]); }
            V[R - 1] = enc_of(st[2 * R]);
            dsave = enc_of(st[2 * R + 1]);
        }
    }
};

// Tagged re-fill of groups g0 .. g_top of a chunk into LDS; of group g_top only its first top_steps steps (2 or 4 are
// run).  Of every group the pointer bytes of the unit's lanes l_lo .. l_lo + WL - 1 are kept (WL = UL: all, l_lo = 0).
template <bool CARRIED, bool SAMEGO, int UL, int WL>
__device__ __forceinline__ void refill_chunk(const CellRegs& kr, const TbUnit<UL>& U, int m, const TbLds& lds,
                                             int (&D)[4], int (&V)[4], int (&H)[4], int& dsave, int g0, int g_top,
                                             int lam, int l_lo, int top_steps) {
    constexpr int R = 4, SPG = 4;
    const int k0 = g0 * SPG;
    int oc_next[SPG];
    int2 hd_next[SPG];
    auto load_group = [&](int g) {
#pragma unroll
        for (int q = 0; q < SPG; ++q) {
            const int kk = g * SPG + q;
            oc_next[q] = lds.ow[kk - k0 + (UL - 1) - lam];
            hd_next[q] = lds.hvt[min(kk + 1, m + U.lb) - k0];     // column j = kk + 1 - lb of the row above, clamped to m
        }
    };
    auto cell = [&](int d_ul, int x_u, int y_l, int t, int o, int& d, int& x, int& y) -> unsigned {
        // (the asm-pinned forms: with four waves per SIMD hipcc's own scheduling of the C forms measured 2 % slower here)
        if constexpr (CARRIED) return cell_carried_tagged_hw<SAMEGO>(kr, d_ul, x_u, y_l, t, o, d, x, y);
        else return cell_hw(kr, d_ul, x_u, y_l, t, o, d, x, y);
    };
    // values from the lane above; the first lane of a unit that is no whole strip takes the row above the unit
    // (lane 32 must not see lane 31)
    auto shift_in = [&](int& v_up, int v_src, int& d_next, int d_src, auto edge_c) {
        const int hv = v_up, hd = d_next;
        if constexpr (UL == 64 && decltype(edge_c)::value) wave_shr1_pair<4>(v_up, v_src, d_next, d_src);
        else wave_shr1_pair_sched(v_up, v_src, d_next, d_src);
        if constexpr (UL < 64) {
            v_up = (lam == 0) ? hv : v_up;
            d_next = (lam == 0) ? hd : d_next;
        }
    };
    const bool in_win = (unsigned)(lam - l_lo) < (unsigned)WL;
    load_group(g0);
    // unpredicated groups: from the one in which the strip's last lane has started on (a lane past its last column
    // goes on over pad codes; what it computes reaches only lanes that are past theirs, pointer bytes
    // and captured bottom-row entries of columns > m, none of which is ever read -- as in phase 1)
    const int gs_lo = (63 + SPG - 1) / SPG;
    // one unpredicated group of NQ <= 4 steps (the steps behind the walk's entry point are nobody's: the walk only
    // moves to smaller k, and the lane state is dropped after the chunk)
    auto steady_group = [&](int g, const int (&oc)[SPG], const int2 (&hd)[SPG], unsigned (&acc)[4], auto nq_c) {
        constexpr int NQ = decltype(nq_c)::value;
        int2 cap[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int v_up = hd[q].x, d_next = hd[q].y;
            shift_in(v_up, V[R - 1], d_next, D[R - 1], std::false_type{});
            int d_ul = dsave, v_u = v_up;                     // (lane_step, nw_cell.h, spelled out)
            unsigned b[R];
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const int d_old = D[rr];
                b[rr] = cell(d_ul, v_u, H[rr], U.tc[rr], oc[q], D[rr], V[rr], H[rr]);
                d_ul = d_old;
                v_u = V[rr];
            }
            acc[q] = pack4(b[0], b[1], b[2], b[3]);
            dsave = d_next;
            cap[q] = make_int2(V[R - 1], D[R - 1]);
        }
        if (lam == UL - 1) {                            // the unit's bottom row, tagged: for pending states
#pragma unroll
            for (int q = 0; q < NQ; ++q) lds.hvb[g * SPG - k0 + q] = cap[q];
        }
    };
    auto edge_group = [&](int g, const int (&oc)[SPG], const int2 (&hd)[SPG], unsigned (&acc)[4]) {
#pragma unroll
        for (int q = 0; q < SPG; ++q) {
            const int kk = g * SPG + q;
            const int j = kk - (U.lb + lam) + 1;
            const bool active = (j >= 1) && (j <= m) && U.lane_has_rows;
            int v_up = hd[q].x, d_next = hd[q].y;
            shift_in(v_up, V[R - 1], d_next, D[R - 1], std::true_type{});
            if (active) {
                unsigned b[R];
                lane_step(cell, D, V, H, dsave, v_up, d_next, U.tc, oc[q], b);
                acc[q] = pack4(b[0], b[1], b[2], b[3]);
                if (lam == UL - 1) lds.hvb[kk - k0] = make_int2(V[R - 1], D[R - 1]);
            }
        }
    };
    for (int g = g0; g <= g_top; ++g) {
        int oc[SPG];
        int2 hd[SPG];
#pragma unroll
        for (int q = 0; q < SPG; ++q) { oc[q] = oc_next[q]; hd[q] = hd_next[q]; }
        unsigned acc[4] = {0u, 0u, 0u, 0u};
        if (g < g_top) {
            load_group(g + 1);
            if (g >= gs_lo) steady_group(g, oc, hd, acc, std::integral_constant<int, SPG>{});
            else edge_group(g, oc, hd, acc);
        } else if (g >= gs_lo) {
            // the group the walk enters the chunk in: only its steps up to the entry point (top_steps of them)
            if (top_steps <= 2) steady_group(g, oc, hd, acc, std::integral_constant<int, 2>{});
            else steady_group(g, oc, hd, acc, std::integral_constant<int, SPG>{});
        } else {
            edge_group(g, oc, hd, acc);
        }
        if (WL == UL || in_win) lds.win[(g - g0) * WL + (lam - l_lo)] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// the re-fill in the problem's cell form: carried (non-positive gap opens), with equal opens or not, or general
template <int UL, int WL>
__device__ __forceinline__ void refill_any(const TbProblem& P, const TbUnit<UL>& U, const TbLds& lds, int (&D)[4],
                                           int (&V)[4], int (&H)[4], int& dsave, int g0, int g_top, int lam,
                                           int l_lo, int top_steps) {
    if (P.carried && P.c.gox == P.c.goy) refill_chunk<true, true, UL, WL>(P.kr, U, P.m, lds, D, V, H, dsave, g0, g_top, lam, l_lo, top_steps);
    else if (P.carried) refill_chunk<true, false, UL, WL>(P.kr, U, P.m, lds, D, V, H, dsave, g0, g_top, lam, l_lo, top_steps);
    else refill_chunk<false, false, UL, WL>(P.kr, U, P.m, lds, D, V, H, dsave, g0, g_top, lam, l_lo, top_steps);
}

// set-up + tagged re-fill of one job, whole unit lanes kept (the kernels that re-fill ahead of the walk: the entry
// lane of a chunk re-filled on expectation is not known)
template <int UL>
__device__ __forceinline__ void refill_job(const TbProblem& P, const TbLds& lds, const TbJob& J, int lam) {
    const TbUnit<UL> U(P, J.u, lam);
    ChunkIn<UL> in;
    in.fetch(P, U, lam, J.ck, J.gtop);
    int D[4], V[4], H[4], dsave;
    in.store(P, U, lam, J.ck, J.gtop, lds, D, V, H, dsave);
    wave_sync();
    refill_any<UL, UL>(P, U, lds, D, V, H, dsave, J.ck * kChunk, J.gtop, lam, 0, J.tops);
    wave_sync();
}

// The walk arrives in a re-filled chunk (first group g0, first valid step kvalid) at step k, lane lw of the window,
// row r of the lane: a pending state is read off the unit's tagged bottom row, the start state off the window.
// False: the pending state was the start state's probe -- the walk goes back to (n, m) without walking this chunk.
template <int WL>
__device__ __forceinline__ bool enter_chunk(const TbProblem& P, const TbLds& lds, TbWalk& w, int g0, int kvalid,
                                            int k, int lw, int r) {
    if (w.pend) {                                              // (x, y): the unit's last row, step k of this chunk
        const int2 e = lds.hvb[k - g0 * 4];
        w.st = 2 - (((w.pend == 3) ? e.y : e.x) & 3);
        w.pend = 0;
        if (w.probe) {                                         // that was the start state: back to (n, m)
            w.probe = 0; w.first = 0;
            w.x = P.n; w.y = P.m;
            return false;
        }
    }
    if (w.first && k >= kvalid) {                              // start state, textSeqCompare.py:102
        w.st = ptr_pm(reinterpret_cast<const uint8_t*>(lds.win)[(((k >> 2) - g0) * WL + lw) * 16 + (k & 3) * 4 + r]);
        w.first = 0;
    }
    return true;
}

__global__ __launch_bounds__(64) void nw_trace2_kernel(NwArgs a) {
    constexpr int R = 4, UL = 64;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    __shared__ uint4 win[kChunkGroups * kWinLanes];
    __shared__ int2 hvt[kChunkSteps + 8];
    __shared__ int2 hvb[kChunkSteps];
    __shared__ uint16_t ow[kChunkSteps + 64 + 8];
    const TbLds lds{win, hvt, hvb, ow};

    const int lane = threadIdx.x;
    const TbProblem P(a, blockIdx.x, true);
    TbWalk w = tb_start<UL>(P.n, P.m);
#if TA_P2_PROFILE
    long long pc_setup = 0, pc_fill = 0, pc_walk = 0, pc_chunks = 0, pc_t = __builtin_readcyclecounter(), pc_groups = 0;
    const long long pc_start = pc_t;
    long long pc_iters = 0;
#endif

    while (w.x > 0 && w.y > 0) {
        const TbUnit<UL> U(P, (w.x - 1) / L::SR, lane);
        int l = ((w.x - 1) % L::SR) / R;
        int r = (w.x - 1) % R;
        int k = (w.y - 1) + l;
        int ck = (k >> 2) / kChunk;                             // chunk the walk is in
        int g_top = k >> 2;                                     // last group to re-fill
        bool in_strip = true;
        ChunkIn<UL> in;
        while (in_strip) {
            const int g0 = ck * kChunk;
            const int kvalid = ck > 0 ? g0 * SPG + 2 : 0;
            const int l_lo = kWinLanes == 64 ? 0 : max(0, l - (kWinLanes - 1));   // the window: lanes l_lo .. l_lo + kWinLanes - 1
            if (in.ck != ck || in.gtop != g_top) in.fetch(P, U, lane, ck, g_top);
            int D[R], V[R], H[R], dsave;
            in.store(P, U, lane, ck, g_top, lds, D, V, H, dsave);
            if (ck > 0) in.fetch(P, U, lane, ck - 1, g0);      // the likely next chunk (registers are free again)
            __syncthreads();
            PC_LAP(pc_setup)

            // tagged re-fill of groups g0 .. g_top into LDS; of group g_top only the steps up to the walk's (k & 3)
            refill_any<UL, kWinLanes>(P, U, lds, D, V, H, dsave, g0, g_top, lane, l_lo,
                                      ((k >> 2) == g_top) ? (k & 3) + 1 : SPG);
            __syncthreads();
            PC_LAP(pc_fill)
#if TA_P2_PROFILE
            pc_chunks += 1; pc_groups += g_top - g0 + 1;
#endif

            // walk the chunk
            if (!enter_chunk<kWinLanes>(P, lds, w, g0, kvalid, k, l - l_lo, r)) {
                __syncthreads();
                break;
            }
            {                                                   // columns go straight to the right-aligned output
#if TA_P2_PROFILE
                long long* const itp = &pc_iters;
#else
                long long* const itp = nullptr;
#endif
                w.len += walk_window_vec<true, kWinLanes, true>(win, g0, kvalid, U.i_h, w.x, w.y, w.st,
                                                                P.ops + (P.cap - 1 - w.len), P.cap - w.len, lane, itp, l_lo);
            }
            if (w.st >= 3) { w.pend = w.st; w.st = 0; }        // left the strip upwards: state pending
            PC_LAP(pc_walk)
            // position in layout coordinates after the walk
            l = (w.x > U.i_h) ? ((w.x - 1) % L::SR) / R : -1;
            r = (w.x - 1) & (R - 1);
            k = (w.y - 1) + l;
            if ((w.x <= 0) | (w.y <= 0) | (l < 0)) {
                in_strip = false;                              // the walk left the strip or finished
            } else if (k >= kvalid) {
                // still inside this chunk: the walk ran off the top lane of the window.  The same chunk
                // again, up to the group the walk stands in, with the window at its lane.
                g_top = k >> 2;
            } else {
                // it ran into the chunk's two halo steps (k < kvalid): the chunk before, extended by
                // the group that holds them
                g_top = g0;
                ck -= 1;
            }
        }
    }
    [[maybe_unused]] const int len = tb_finish(a, P, w.x, w.y, w.len, lane == 0);
#if TA_P2_PROFILE
    if (lane == 0) {                                   // row 0 of the workspace is phase 1's: free by now
        long long* out = reinterpret_cast<long long*>(P.ws_p + P.ws.row(0));
        out[0] = pc_setup; out[1] = pc_fill; out[2] = pc_walk; out[3] = pc_chunks; out[4] = pc_groups; out[5] = len;
        out[6] = pc_iters; out[7] = __builtin_readcyclecounter() - pc_start;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// phase 2 for SMALL and MEDIUM batches: NWV waves per problem, speculating along the path.
//
// With one wave per problem (above) a problem's traceback is a chain of ~6 chunks per strip, each
// set-up -> re-fill (70 %) -> walk, and at a thousand problems that lone wave per SIMD IS the launch's
// time (1024 x 2048^2: 0.70 ms, 64 problems: 0.63 ms -- latency, not throughput).  But which chunk
// comes next is almost always known before the walk gets there: the chunk BEFORE the one it is in,
// same strip, entered through the two halo steps.  So the chunks along the path are dealt to the
// waves of a workgroup round-robin -- iteration i (the i-th chunk of the path) belongs to wave
// i mod NWV.  A wave re-fills the chunk it EXPECTS its iteration to be (the newest job it knows, moved
// back by the iterations in between) into its own LDS window while the waves before it are still
// busy, then waits for the token of iteration i - 1 (position, state, alignment length so far and
// the job of iteration i as the walk really left it), re-fills again only if the expectation was
// wrong (the walk left the strip: once per strip), walks, and passes the token on.  Speculative
// re-fills keep all 64 lanes of a chunk (the entry lane is not known yet; 17 KiB of LDS per wave --
// what a batch this small can afford) and, of the halo group, the two steps a walk can enter at.
// Results are the one-wave kernel's, bit for bit: same re-fill, same walk, same pending-state rules.
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void nw_trace2w_kernel(NwArgs a) {
    constexpr int R = 4, UL = 64;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    constexpr int WL = 64;                                      // whole chunks: the entry lane of a speculative chunk is unknown
    __shared__ uint4 win_s[NWV][kChunkGroups * WL];
    __shared__ int2 hvt_s[NWV][kChunkSteps + 8];
    __shared__ int2 hvb_s[NWV][kChunkSteps];
    __shared__ uint16_t ow_s[NWV][kChunkSteps + 64 + 8];
    __shared__ int tok_s[NWV][kTokInts];
    __shared__ int seq_s;                                       // iterations whose token is published

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TbProblem P(a, blockIdx.x, true);
    if (threadIdx.x == 0) seq_s = 0;
    __syncthreads();                                            // the only workgroup barrier: the waves run apart from here
    const TbLds lds{win_s[wave], hvt_s[wave], hvb_s[wave], ow_s[wave]};

    // the token before iteration 0: the start of the walk, the same on every wave
    TbTok T;
    T.w = tb_start<UL>(P.n, P.m);
    T.done = 0;
    T.job = tb_job_at<UL>(T.w.x, T.w.y);
    if (T.job.u < 0) {                                          // an empty string: nothing to walk, boundary run only
        if (wave == 0) tb_finish(a, P, P.n, P.m, 0, lane == 0);
        return;
    }
    int kt = -1;                                                // index of the newest token this wave holds

    // every iteration publishes exactly one token, so no wave ever waits for one that does not come; the bound is a
    // belt against a walk that makes no progress (none known): the wave that reaches it ends the walk for everyone
    const int max_iter = 4 * (L::nstrips(max(P.n, 1)) * (P.ws.ngroups / kChunk + 2)) + 64;
    for (int i = wave; ; i += NWV) {
        // (1) speculation + (2) the token of iteration i - 1.  While that token is not there, the wave re-fills the
        // job its iteration will most likely be: the job of the NEWEST token published (iteration j < i - 1), moved
        // on by the i - 1 - j iterations in between along the diagonal (tb_predict: the chunk before while the strip
        // lasts, then the chunk of the strip above the diagonal enters).  A newer token that changes the expectation (the walk left the
        // strip) replaces the speculation at once -- the waves behind the one that must re-fill the new strip's
        // first chunk re-fill its second, third ... beside it instead of one after the other.
        TbJob spec{-1, 0, 0, 0};
        if (i > kt + 1) {
            int spins = 0, based_on = -2;                         // token the current expectation comes from (-2: none yet)
            while (true) {
                const int have = __builtin_amdgcn_readfirstlane(
                    __hip_atomic_load(&seq_s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (have >= i) break;                            // token i - 1 is there
                const int from = max(kt, have - 1);              // newest token to go by: the one held, or a fresher one
                if (from != based_on) {
                    based_on = from;
                    // the job of iteration from + 1 and where it starts (a fresher token's slot is not rewritten
                    // before iteration from + NWV > i)
                    const TbTok F = (from != kt) ? tok_load(tok_s[from % NWV]) : T;
                    const TbJob want = tb_predict<UL>(F.w.x, F.w.y, F.job, i - from - 1);
                    if (!F.done && want.u >= 0 &&
                        !(spec.u >= 0 && want.u == spec.u && want.ck == spec.ck && want.gtop == spec.gtop)) {
                        spec = want;
                        refill_job<UL>(P, lds, spec, lane);
                        continue;
                    }
                }
                // (bounded: every iteration publishes a token, so the wait always ends -- the bound only makes sure a
                // mistake here could never leave waves spinning on the chip; ~1 s)
                if (++spins >= (1 << 24)) break;
                __builtin_amdgcn_s_sleep(4);
            }
            if (spins >= (1 << 24)) break;
            T = tok_load(tok_s[(i - 1) % NWV]);
            kt = i - 1;
        }
        if (T.done) {
            // the walk is over (another wave finished it).  Pass the word on as the token of THIS iteration: the
            // wave of iteration i + 1 is waiting for it (every iteration publishes exactly one token)
            if (lane == 0) {
                tok_s[i % NWV][5] = 4;
                __hip_atomic_store(&seq_s, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            break;
        }
        // (3) the chunk itself, unless the speculation was right
        const TbJob J = T.job;
        if (!tb_serves(spec, J)) refill_job<UL>(P, lds, J, lane);
        // (4) walk (nw_trace2_kernel)
        TbTok N = T;
        TbWalk& w = N.w;
        const int g0 = J.ck * kChunk;
        const int kvalid = J.ck > 0 ? g0 * SPG + 2 : 0;
        const int l = ((w.x - 1) % L::SR) / R, r = (w.x - 1) % R, k = (w.y - 1) + l;
        if (enter_chunk<WL>(P, lds, w, g0, kvalid, k, l, r)) {
            w.len += walk_window_vec<true, WL, true>(lds.win, g0, kvalid, J.u * L::SR, w.x, w.y, w.st,
                                                     P.ops + (P.cap - 1 - w.len), P.cap - w.len, lane, nullptr, 0);
            if (w.st >= 3) { w.pend = w.st; w.st = 0; }          // left the strip upwards: state pending
        }
        // (5) the token of this iteration
        N.job = tb_job_at<UL>(w.x, w.y);
        N.done = N.job.u < 0 || i >= max_iter;
        if (N.done) tb_finish(a, P, w.x, w.y, w.len, lane == 0);  // the walk is over: boundary runs and the length
        if (lane == 0) {
            tok_store(tok_s[i % NWV], N);
            __hip_atomic_store(&seq_s, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (N.done) break;
        T = N;
        kt = i;
    }
}

// ---------------------------------------------------------------------------------------------
// phase 2 for LARGE batches: TWO problems per wave, each in 32 lanes, walking back HALF-strips.
//
// The one-wave kernel re-fills whole 64-lane chunks although a walk enters a chunk at some lane l and only lanes
// <= l matter: every strip costs 256 + 63 skewed steps of a full wave.  With lane 31's bottom row kept by phase 1
// (Ws2, kSubRows = 2) a strip falls into two half-strips of 128 rows that restart independently -- from the same
// state checkpoints (lanes 0 .. 31 or 32 .. 63 of them) and from the row above the half -- and a half-strip costs
// 128 + 31 steps of HALF a wave.  So a wave carries two problems, one per 32 lanes, each running the one-wave
// kernel's loop (set-up, tagged re-fill of a chunk, walk, next chunk) on its own half-strips; the two halves share
// the instruction stream and diverge only in trip counts (the compiler's EXEC masking: the half with the shorter
// re-fill or walk waits for the other).  Per problem ~0.58 of the re-filled wave-groups of the one-wave kernel.
// Everything that was wave-uniform there (position, state, chunk, pointers) is per lane here, equal within a half;
// ballots are split per half; a half's LDS arrays are its own.  Results are the one-wave kernel's, bit for bit.

// walk_window_vec (nw_hw.h) for one half of a wave: 32 lanes look ahead along the run, the ballots are split per half,
// position and state are per-lane copies.  win: [(group - gw_lo) * 32 + (strip lane - lb)]; x_lo: the row above the
// half-strip.  A step that leaves a half-strip below the table's first upwards ends the walk with st = 3 + state.
__device__ __forceinline__ int walk_half(const uint4* win, int gw_lo, int klow, int x_lo, int lb, int& x, int& y, int& st,
                                         uint8_t* opsbuf, int max_ops, int lam, int half) {
    constexpr int R = 4, LW = kHalfLanes;
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(win);
    int cnt = 0;
    while (true) {
        const int up = (st != 2), left = (st != 1);
        const int xi = x - lam * up, yi = y - lam * left;
        const int li = ((xi - 1 - x_lo) >> 2) + lb;                       // strip lane of the cell this lane looks at
        const int ki = (yi - 1) + li;
        const bool valid = (xi > x_lo) & (yi > 0) & (ki >= klow);
        unsigned b = 0;
        if (valid) b = wb[((ki >> 2) - gw_lo) * (LW * 16) + (li - lb) * 16 + (ki & 3) * R + ((xi - 1) & (R - 1))];
        int nxt = 2 - (int)((b >> (2 * st)) & 3u);
        if (up && x_lo > 0 && xi == x_lo + 1) nxt = 3 + st;
        const unsigned long long vm64 = __ballot(valid);
        const unsigned long long cm64 = __ballot(valid && nxt == st);
        const unsigned vmask = half ? (unsigned)(vm64 >> 32) : (unsigned)vm64;
        const unsigned cmask = half ? (unsigned)(cm64 >> 32) : (unsigned)cm64;
        if ((vmask & 1u) == 0u) break;                                     // the current cell is out
        const int run = (~cmask == 0u) ? LW : (int)__builtin_ctz(~cmask);  // lanes 0 .. run - 1 stay in st
        int steps = run, st_new = st;
        // (an LDS shuffle: every lane of the half asks the same lane.  Two scalar v_readlane per half instead -- each
        // half's run length is uniform in the half -- measured slower, 2.46 against 2.42 ms: the scalar round trip
        // stalls the wave longer than the ds_bpermute it would save)
        const int nxt_at = __shfl(nxt, half * LW + min(run, LW - 1), 64);
        if (run < LW && ((vmask >> run) & 1u)) {                           // the step that leaves state st
            steps = run + 1;
            st_new = nxt_at;
        }
        steps = min(steps, max_ops - cnt);
        if (steps < run + 1) st_new = st;                                  // truncated inside the run
        if (lam < steps) opsbuf[-(cnt + lam)] = (uint8_t)st;
        cnt += steps;
        x -= steps * up;
        y -= steps * left;
        st = st_new;
        if (cnt >= max_ops) break;
    }
    return cnt;
}

__global__ __launch_bounds__(64) void nw_trace2h_kernel(NwArgs a) {
    constexpr int R = 4, UL = kHalfLanes;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    __shared__ uint4 win_s[2][kChunkGroups * UL];
    __shared__ int2 hvt_s[2][kChunkSteps + 8];
    __shared__ int2 hvb_s[2][kChunkSteps];
    __shared__ uint16_t ow_s[2][kChunkSteps + UL + 8];

    const int lane = threadIdx.x, half = lane >> 5, lam = lane & (UL - 1);
    const int pr = blockIdx.x * 2 + half;
    const bool alive = pr < a.nprob;                            // (an odd batch: the last wave's second half idles)
    const TbProblem P(a, alive ? pr : a.nprob - 1, alive);
    const TbLds lds{win_s[half], hvt_s[half], hvb_s[half], ow_s[half]};
    TbWalk w = tb_start<UL>(P.n, P.m);
#if TA_P2_PROFILE
    // (wave-level clocks: the halves move in lockstep, so a phase's time is the slower half's; pc_groups / pc_iters
    // count THIS half's own re-filled groups and walk iterations)
    long long pc_setup = 0, pc_fill = 0, pc_walk = 0, pc_chunks = 0, pc_t = __builtin_readcyclecounter(), pc_groups = 0;
    const long long pc_start = pc_t;
    long long pc_iters = 0;
#endif

    while (w.x > 0 && w.y > 0) {
        const TbUnit<UL> U(P, (w.x - 1) / (R * UL), lam);       // the half-strip the walk is in
        int l = ((w.x - 1) % L::SR) / R;                        // strip lane
        int r = (w.x - 1) % R;
        int k = (w.y - 1) + l;
        int ck = (k >> 2) / kChunk;
        int g_top = k >> 2;
        if (ck > 0 && k < ck * kChunk * SPG + 2) ck -= 1;       // a chunk's first two steps belong to the chunk before
        bool in_strip = true;
        ChunkIn<UL> in;
        while (in_strip) {
            const int g0 = ck * kChunk;
            const int kvalid = ck > 0 ? g0 * SPG + 2 : 0;
            if (in.ck != ck || in.gtop != g_top) in.fetch(P, U, lam, ck, g_top);
            int D[R], V[R], H[R], dsave;
            in.store(P, U, lam, ck, g_top, lds, D, V, H, dsave);
            if (ck > 0) in.fetch(P, U, lam, ck - 1, g0);       // the likely next chunk (the registers are free again)
            wave_sync();
            PC_LAP(pc_setup)
            // tagged re-fill of groups g0 .. g_top
            refill_any<UL, UL>(P, U, lds, D, V, H, dsave, g0, g_top, lam, 0, ((k >> 2) == g_top) ? (k & 3) + 1 : SPG);
            wave_sync();
            PC_LAP(pc_fill)
#if TA_P2_PROFILE
            pc_chunks += 1; pc_groups += g_top - g0 + 1;
#endif
            // walk the chunk
            if (!enter_chunk<UL>(P, lds, w, g0, kvalid, k, l - U.lb, r)) break;
            w.len += walk_half(lds.win, g0, kvalid, U.i_h, U.lb, w.x, w.y, w.st, P.ops + (P.cap - 1 - w.len),
                               P.cap - w.len, lam, half);
            if (w.st >= 3) { w.pend = w.st; w.st = 0; }        // left the half-strip upwards: state pending
            PC_LAP(pc_walk)
            l = (w.x > U.i_h) ? ((w.x - 1) % L::SR) / R : -1;
            r = (w.x - 1) & (R - 1);
            k = (w.y - 1) + l;
            if ((w.x <= 0) | (w.y <= 0) | (l < U.lb)) {
                in_strip = false;                              // the walk left the half-strip or finished
            } else if (k >= kvalid) {
                g_top = k >> 2;                                // (not reached: whole half-strip chunks are kept)
            } else {
                g_top = g0;                                    // the chunk before, through its halo
                ck -= 1;
            }
        }
    }
    [[maybe_unused]] const int len = tb_finish(a, P, w.x, w.y, w.len, lam == 0);
#if TA_P2_PROFILE
    if (alive && lam == 0) {                           // row 0 of the workspace is phase 1's: free by now
        long long* out = reinterpret_cast<long long*>(P.ws_p + P.ws.row(0));
        out[0] = pc_setup; out[1] = pc_fill; out[2] = pc_walk; out[3] = pc_chunks; out[4] = pc_groups; out[5] = len;
        out[6] = pc_iters; out[7] = __builtin_readcyclecounter() - pc_start;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// phase 2 for MEDIUM batches: both of the above at once -- two problems per wave on half-strips (nw_trace2h_kernel:
// ~0.58 of the re-filled cells) AND several waves per pair of problems that re-fill the chunks they expect ahead of
// the walk (nw_trace2w_kernel: the chain of set-up -> re-fill -> walk off the critical path).  A workgroup of NWV
// waves owns two problems, one per 32 lanes of every wave; iteration i -- one chunk job of each problem -- belongs to
// wave i mod NWV, which re-fills the jobs it expects for BOTH halves into its own LDS windows, waits for the tokens of
// iteration i - 1 (one per half), re-fills again the halves whose expectation was wrong, walks both and passes the
// tokens on.  A half whose problem is finished idles (its token says so); the workgroup leaves when both are.
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void nw_trace2hw_kernel(NwArgs a) {
    constexpr int R = 4, UL = kHalfLanes;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    __shared__ uint4 win_s[NWV][2][kChunkGroups * UL];
    __shared__ int2 hvt_s[NWV][2][kChunkSteps + 8];
    __shared__ int2 hvb_s[NWV][2][kChunkSteps];
    __shared__ uint16_t ow_s[NWV][2][kChunkSteps + UL + 8];
    __shared__ int tok_s[NWV][2][kTokInts];
    __shared__ int seq_s;

    const int lane = threadIdx.x & 63, half = lane >> 5, lam = lane & (UL - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pr = blockIdx.x * 2 + half;
    const bool alive = pr < a.nprob;
    const TbProblem P(a, alive ? pr : a.nprob - 1, alive);
    const TbLds lds{win_s[wave][half], hvt_s[wave][half], hvb_s[wave][half], ow_s[wave][half]};
    if (threadIdx.x == 0) seq_s = 0;
    __syncthreads();                                            // the only workgroup barrier

    // this half's token before iteration 0 (the same on every wave)
    TbTok T;
    T.w = tb_start<UL>(P.n, P.m);
    T.job = tb_job_at<UL>(T.w.x, T.w.y);
    T.done = T.job.u < 0;
    if (T.done && wave == 0) tb_finish(a, P, P.n, P.m, 0, lam == 0);   // an empty string (or no problem in this half): boundary run only
    if (__all(T.done)) return;
    int kt = -1;

    const int max_iter = 8 * (2 * L::nstrips(max(P.n, 1)) * (P.ws.ngroups / kChunk + 2)) + 64;
    const int max_iter_w = __builtin_amdgcn_readfirstlane(max(__shfl(max_iter, 0, 64), __shfl(max_iter, UL, 64)));
    for (int i = wave; ; i += NWV) {
        // (1) speculation + (2) the tokens of iteration i - 1 (nw_trace2w_kernel; a half re-fills where `change`, the
        // other half waits)
        TbJob spec{-1, 0, 0, 0};
        if (i > kt + 1) {
            int spins = 0, based_on = -2;
            while (true) {
                const int have = __builtin_amdgcn_readfirstlane(
                    __hip_atomic_load(&seq_s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (have >= i) break;
                const int from = max(kt, have - 1);
                if (from != based_on) {
                    based_on = from;
                    const TbTok F = (from != kt) ? tok_load(tok_s[from % NWV][half]) : T;
                    const TbJob want = F.done ? TbJob{-1, 0, 0, 0} : tb_predict<UL>(F.w.x, F.w.y, F.job, i - from - 1);
                    const bool change = want.u >= 0 &&
                        !(spec.u >= 0 && want.u == spec.u && want.ck == spec.ck && want.gtop == spec.gtop);
                    if (__any(change)) {
                        if (change) { spec = want; refill_job<UL>(P, lds, spec, lam); }
                        continue;
                    }
                }
                if (++spins >= (1 << 24)) break;                 // (bounded: a mistake could never leave waves spinning)
                __builtin_amdgcn_s_sleep(4);
            }
            if (spins >= (1 << 24)) break;
            T = tok_load(tok_s[(i - 1) % NWV][half]);
            kt = i - 1;
        }
        if (__all(T.done)) {                                     // both walks are over: pass the word on and leave
            if (lam == 0) tok_s[i % NWV][half][5] = 4;
            if (lane == 0) __hip_atomic_store(&seq_s, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            break;
        }
        const bool live = !T.done;                               // this half still walks
        // (3) the chunk itself where the speculation was wrong
        const TbJob J = T.job;
        if (live && !tb_serves(spec, J)) refill_job<UL>(P, lds, J, lam);
        // (4) walk (nw_trace2h_kernel)
        TbTok N = T;
        TbWalk& w = N.w;
        if (live) {
            const int lb = (J.u * UL) & 63, i_h = J.u * (R * UL);
            const int g0 = J.ck * kChunk;
            const int kvalid = J.ck > 0 ? g0 * SPG + 2 : 0;
            const int l = ((w.x - 1) % L::SR) / R, r = (w.x - 1) % R, k = (w.y - 1) + l;
            if (enter_chunk<UL>(P, lds, w, g0, kvalid, k, l - lb, r)) {
                w.len += walk_half(lds.win, g0, kvalid, i_h, lb, w.x, w.y, w.st, P.ops + (P.cap - 1 - w.len),
                                   P.cap - w.len, lam, half);
                if (w.st >= 3) { w.pend = w.st; w.st = 0; }
            }
        }
        // (5) the tokens of this iteration
        N.job = live ? tb_job_at<UL>(w.x, w.y) : TbJob{-1, 0, 0, 0};
        N.done = !live || N.job.u < 0 || i >= max_iter_w;
        if (live && N.done) tb_finish(a, P, w.x, w.y, w.len, lam == 0);   // this half's walk ends here: boundary runs and the length
        if (lam == 0) tok_store(tok_s[i % NWV][half], N);
        if (lane == 0) __hip_atomic_store(&seq_s, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__all(N.done)) break;
        T = N;
        kt = i;
    }
}

}  // namespace ta

using namespace ta;

// widest problem of the two-phase aligner: its LDS holds the OCR codes (2 B each) only
extern "C" int32_t ta_nw2_max_m(void) { return 65000; }

extern "C" int64_t ta_nw2_workspace_bytes(int32_t n, int32_t m) {
    if (n <= 0 || m <= 0) return 16;
    return (Ws2(n, m).total + 15) & ~(int64_t)15;
}

template <int W, int MODE, bool SAMEGO, typename OC, int BAND = 0>
static hipError_t launch_score_k(const NwArgs& a, size_t lds, hipStream_t st) {
    hipError_t e = allow_full_lds(&nw_score_kernel<W, MODE, SAMEGO, OC, BAND>);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nw_score_kernel<W, MODE, SAMEGO, OC, BAND>), dim3(a.nprob), dim3(W * 64), lds, st, a);
    return hipGetLastError();
}

// Banded fill: the band's groups of every problem, then today's kernel over the problems that did not certify.
// The second launch has one workgroup per problem of the batch; the workgroup of a certified problem reads its word
// and leaves at once (no host synchronisation, no list: a batch that certifies throughout costs the launch alone).
template <int W>
static hipError_t launch_score_band(const NwArgs& a, size_t lds, bool samego, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.band_ok, 0, sizeof(int32_t) * (size_t)a.nprob, st);
    if (e != hipSuccess) return e;
    e = samego ? launch_score_k<W, 2, true, uint16_t, 1>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 1>(a, lds, st);
    if (e != hipSuccess) return e;
    return samego ? launch_score_k<W, 2, true, uint16_t, 2>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 2>(a, lds, st);
}

// Funnel fill: the certificate's words are set (the exit word to its host part), the funnel's groups of every problem
// run, nw_band_certify_kernel takes the decision at a kernel boundary, and the same fallback launch follows.
template <int W>
static hipError_t launch_score_funnel(const NwArgs& a, const int32_t* x0, size_t lds, bool samego, hipStream_t st) {
    const dim3 grid((a.nprob + 255) / 256);
    hipLaunchKernelGGL(nw_band_cert_init_kernel, grid, dim3(256), 0, st, a, x0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = samego ? launch_score_k<W, 2, true, uint16_t, 3>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 3>(a, lds, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nw_band_certify_kernel, grid, dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return samego ? launch_score_k<W, 2, true, uint16_t, 2>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 2>(a, lds, st);
}

// LCS-bounded funnel: the flag words decide per problem (nw_band_cert_init_lcs_kernel), nw_lcs_suffix_kernel leaves
// the tables of the problems it covers, and the funnel fill (BAND = 4) reads them; certificate and fallback as above.
template <int W>
static hipError_t launch_score_funnel_lcs(const NwArgs& a, const int32_t* x0, size_t lds, bool samego, int alphabet,
                                          hipStream_t st) {
    const dim3 grid((a.nprob + 255) / 256);
    const bool covers = alphabet > 0 && alphabet <= kLcsMaxAlphabet;
    hipLaunchKernelGGL(nw_band_cert_init_lcs_kernel, grid, dim3(256), 0, st, a, x0, covers ? alphabet : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (covers) {
        const size_t lcs_lds = lcs_mask_lds_bytes(alphabet, a.lcs_max_n);   // (as it comes: padded to 10 240 B it ran the same)
        hipLaunchKernelGGL(nw_lcs_suffix_kernel, dim3(a.nprob), dim3(64), lcs_lds, st, a, alphabet);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    e = samego ? launch_score_k<W, 2, true, uint16_t, 4>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 4>(a, lds, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nw_band_certify_kernel, grid, dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return samego ? launch_score_k<W, 2, true, uint16_t, 2>(a, lds, st) : launch_score_k<W, 2, false, uint16_t, 2>(a, lds, st);
}

template <int W>
static hipError_t launch_score_w(const NwArgs& a, size_t lds, bool profile, bool samego, bool codes8, hipStream_t st) {
    if (profile) return samego ? launch_score_k<W, 2, true, uint16_t>(a, lds, st)
                               : launch_score_k<W, 2, false, uint16_t>(a, lds, st);
    return codes8 ? launch_score_k<W, 1, false, uint8_t>(a, lds, st)
                  : launch_score_k<W, 1, false, uint16_t>(a, lds, st);
}

// Phase-1 launch shape.  Waves per workgroup W <= strips of the tallest problem; with the score
// profile the LDS per workgroup is W x apad x 256 B + the codes.  W is chosen by a small model fitted
// to measurements (tools/p1_time.py on 2048 x 1024^2, 1024 / 2048 x 2048^2, 4096 x 4096^2,
// 512 x 8192^2: it picks the fastest W in each): score = min(resident waves per CU, 12)
// x (share of a workgroup's time that is not start-up ramp) x (share of the chip the batch fills).
// What workgroups that share a CU can hold together.  One workgroup may be given 160 KiB, but measured on
// MI355X (nw_score_kernel with its LDS request padded, tools/p1_time.py with TA_NW2_LDS_PAD): three
// workgroups of 41.3 KiB and two of 53.3 KiB run side by side, two of 63.3 KiB do not -- the limit for
// co-residency lies between 124 and 126 KiB.  (The single-wave workgroups of nw_trace2_kernel, 19.4 KiB
// static each, do run eight to a CU; the figure below is for this kernel's launch shapes.)
constexpr size_t kLdsShared = 124 * 1024;
struct P1Plan { int mode, w, apad; size_t lds; bool samego, codes8; };

static P1Plan plan_phase1(int max_n, int max_m, uint32_t flags, int nprob = 1 << 20, bool band_forced = false) {
    P1Plan pl{};
    const int nstrips = PtrLayout<4>::nstrips(max_n);
    const int wmax = nstrips >= 8 ? 8 : nstrips >= 4 ? 4 : nstrips >= 2 ? 2 : 1;
    pl.codes8 = (flags & TA_NW_CODES8) != 0;
    pl.samego = (flags & TA_NW_OPENS_SAME) != 0;
    const int alphabet = (int)((flags >> TA_NW_ALPHABET_SHIFT) & 0xFFu);
    bool profile = alphabet > 0 && alphabet < 255 && !(flags & TA_NW_NO_PROFILE);
    pl.w = wmax;
    const int ngroups = PtrLayout<4>::ngroups(max_m);
    // best W for a workgroup that needs lds(W) bytes; returns the resident waves of the choice
    auto choose = [&](auto lds_of, int w_least, int& w_out) -> int {
        int best_w = 0, best_res = 0;
        double best_score = 0.0;
        for (int cand : {4, 8, 2, 1}) {            // order of preference among equals (measured: 4 >= 8 > 2)
            if (cand > wmax || cand < w_least) continue;
            const size_t need = lds_of(cand);
            if (need > 160 * 1024) continue;
            // resident waves per CU: whole workgroups, within the LDS and within 5 waves per SIMD (VGPRs);
            // beyond three per SIMD the kernel gains nothing (it is bound by VALU issue from there on)
            const int res = (int)std::min<size_t>(kLdsShared / need, 20 / cand) * cand;
            // the waves of a workgroup start 25 groups apart: with few passes over the strips that
            // ramp is a visible share of a workgroup's time (W = 8 on 8 strips of 2048 columns: 25 %)
            const int passes = (nstrips + cand - 1) / cand;
            const double busy = (double)passes * ngroups / ((double)passes * ngroups + 25.0 * (cand - 1));
            // and the batch has to fill the chip: nprob x W waves for 256 CUs x 12
            const double fill = std::min(1.0, (double)nprob * cand / (256.0 * 12.0));
            const double score = std::min(res, 12) * busy * fill;
            if (score > best_score + 1e-9) { best_score = score; best_res = res; best_w = cand; }
        }
        w_out = best_w;
        return best_res;
    };
    if (profile) {
        pl.apad = alphabet + 1;
        int w = 0;
        const int res = choose([&](int cand) { return P1Lds(max_m, 2, cand * pl.apad * 256).total; }, 1, w);
        // a profile that leaves fewer than 8 waves on a CU is not worth its LDS -- for a full fill.  Under a band the
        // caller asked for (band_forced: tests, tuning) there is nothing to weigh it against: the banded instantiations
        // exist for the profile and workgroups of 4 or 8 waves alone, so the profile stays wherever such a workgroup
        // fits.  (A plan that keeps the profile by the rule is the same with and without band_forced.)
        if (w != 0 && res < 8 && band_forced) {
            w = 0;
            choose([&](int cand) { return P1Lds(max_m, 2, cand * pl.apad * 256).total; }, 4, w);
            if (w != 0) pl.w = w;
            else profile = false;
        } else if (w == 0 || res < 8) profile = false;
        else pl.w = w;
    }
    if (!profile) {
        int w = 0;
        // compare-select cell: measured 4 >= 8 > 2 at 4096 x 4096^2 (14.5 / 14.9 / 16.9 ms); narrower
        // workgroups were not fitted for this mode
        choose([&](int) { return P1Lds(max_m, pl.codes8 ? 1 : 2).total; }, std::min(4, wmax), w);
        if (w > 0) pl.w = w;
    }
    if (const int v = (int)((flags >> TA_NW_WAVES_SHIFT) & 0xFu)) {      // caller fixes the width (tests / tuning)
        if ((v == 1 || v == 2 || v == 4 || v == 8) && v <= wmax &&
            (!profile || P1Lds(max_m, 2, v * pl.apad * 256).total <= 160 * 1024))
            pl.w = v;
    }
    pl.mode = profile ? 2 : 1;
    if (!profile) pl.apad = 0;
    pl.lds = profile ? P1Lds(max_m, 2, pl.w * pl.apad * 256).total : P1Lds(max_m, pl.codes8 ? 1 : 2).total;
    return pl;
}

extern "C" int ta_nw2_phase1_plan_batch(int32_t max_n, int32_t max_m, int32_t nprob, uint32_t flags, int32_t* out) {
    if (!out || max_n < 0 || max_m < 0 || nprob < 0) return ta_fail(TA_EINVAL, "bad argument");
    const P1Plan pl = plan_phase1(max_n, max_m, flags, nprob);
    out[0] = pl.mode; out[1] = pl.w; out[2] = (int32_t)pl.lds; out[3] = pl.samego ? 1 : 0;
    return TA_OK;
}

extern "C" int ta_nw2_phase1_plan(int32_t max_n, int32_t max_m, uint32_t flags, int32_t* out) {
    return ta_nw2_phase1_plan_batch(max_n, max_m, 1 << 20, flags, out);
}

// ---- the band's host side: bound, rule for w, plan ----
static int32_t clamp_i32(int64_t v) { return (int32_t)std::max<int64_t>(-(1ll << 30), std::min<int64_t>(v, 1ll << 30)); }

extern "C" int32_t ta_nw2_band_bound(int32_t n, int32_t m, const int32_t* params, int32_t w) {
    if (!params || n < 0 || m < 0 || w < 0) return INT32_MAX;
    return clamp_i32(band_bound(n, m, params, w));
}

// The band is worth its certificate only where a good alignment clears the bound with room to spare: w is the
// smallest width whose bound lies below kBandTheta of what an alignment of nothing but best-scoring pairs would get,
// U(w) < theta a min(n, m).  -1: no width does (a <= 0, or gaps cost so little that a - cv - ch <= 0).
constexpr int kBandThetaNum = 1, kBandThetaDen = 2;
static int band_rule_w(int n, int m, const int32_t* prm) {
    const int64_t a = std::max(prm[0], prm[1]);
    const int64_t cv = std::max<int64_t>((int64_t)prm[4] + std::max(prm[2], 0), -1);
    const int64_t ch = std::max<int64_t>((int64_t)prm[5] + std::max(prm[3], 0), -1);
    if (a <= 0 || a - cv - ch <= 0) return -1;
    const int64_t target = a * std::min(n, m) * kBandThetaNum;     // U(w) * den < target
    int lo = 0, hi = std::max(n, m);                                // U is non-increasing in w
    if (band_bound(n, m, prm, hi) * kBandThetaDen >= target) return -1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (band_bound(n, m, prm, mid) * kBandThetaDen < target) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// groups the banded fill runs for an n x m problem, and all of them
static void band_share(int n, int m, int w, int64_t& run, int64_t& all) {
    const int nstrips = PtrLayout<4>::nstrips(n), ngroups = PtrLayout<4>::ngroups(m);
    run = 0; all = (int64_t)nstrips * ngroups;
    for (int s = 0; s < nstrips; ++s) { const BandRange r = band_groups(n, m, w, s); run += r.gh - r.gl; }
}
constexpr int kBandMinN = 1024;            // tallest problem: below four strips the ramp of a workgroup outweighs what a band saves
constexpr int kBandMaxSharePermille = 800; // the band has to save a fifth of the largest problem's groups

// band: 0 = the rule above, 1 = off, otherwise the width itself (tests, tuning; phase 1 then keeps the score profile
// wherever a workgroup of 4 or 8 waves fits, also where ta_nw2_phase1_plan_batch, which knows of no band, reports none).
// out[0] = width the fill will use (0: today's full kernel), out[1] = width by the rule (-1: none), out[2] = share of
// the largest problem's groups the band runs, in 1/1000 (of out[1] when out[0] = 0), out[3] = its strips, out[4] = index
// of the largest problem; u_out[nprob] = U(out[0]) per problem (when out[0] > 0); ranges_out[2 out[3]] = (gl, gh) per strip
// of the largest problem (for out[0], or out[1] when the band is declined).  All pointers [host].
extern "C" int ta_nw2_band_plan(const int32_t* n_arr, const int32_t* m_arr, int32_t nprob, const int32_t* params,
                                int32_t params_stride, uint32_t flags, int32_t band, int32_t* out, int32_t* u_out,
                                int32_t* ranges_out, int32_t ranges_cap) {
    if (!n_arr || !m_arr || !params || !out || nprob < 0 || band < 0 || (params_stride != 0 && params_stride != 6))
        return ta_fail(TA_EINVAL, "bad argument");
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[1] = -1;
    if (nprob == 0) return TA_OK;
    int big = 0, max_n = 0, max_m = 0;
    for (int p = 0; p < nprob; ++p) {
        if (n_arr[p] < 0 || m_arr[p] < 0) return ta_fail(TA_EINVAL, "negative size");
        if ((int64_t)n_arr[p] * m_arr[p] > (int64_t)n_arr[big] * m_arr[big]) big = p;
        max_n = std::max(max_n, n_arr[p]); max_m = std::max(max_m, m_arr[p]);
    }
    out[4] = big;
    out[3] = PtrLayout<4>::nstrips(n_arr[big]);
    // one width for the batch: the widest any of its problems asks for
    int w_rule = 0;
    for (int p = 0; p < nprob && w_rule >= 0; ++p) {
        if (n_arr[p] <= 0 || m_arr[p] <= 0) continue;
        if (params_stride == 0 && p > 0 && n_arr[p] == n_arr[p - 1] && m_arr[p] == m_arr[p - 1]) continue;   // as the one before
        const int wp = band_rule_w(n_arr[p], m_arr[p], params + (size_t)p * params_stride);
        w_rule = wp < 0 ? -1 : std::max(w_rule, wp);
    }
    out[1] = w_rule;
    const P1Plan pl = plan_phase1(max_n, max_m, flags, nprob, band >= 2);
    // the banded instantiations exist for the score profile and workgroups of 4 or 8 waves: what large problems get
    const bool can = pl.mode == 2 && (pl.w == 4 || pl.w == 8) && max_n <= kBandMaxLen && max_m <= kBandMaxLen &&
                     n_arr[big] > 0 && m_arr[big] > 0;
    int w_use = 0;
    int64_t run = 0, all = 1;
    if (w_rule >= 0) band_share(n_arr[big], m_arr[big], std::max(w_rule, 2), run, all);
    if (band >= 2) w_use = can ? band : 0;
    else if (band == 0 && can && w_rule >= 0 && max_n >= kBandMinN && run * 1000 < all * kBandMaxSharePermille)
        w_use = std::max(w_rule, 2);
    if (w_use > 0) band_share(n_arr[big], m_arr[big], w_use, run, all);
    out[0] = w_use;
    // the rule's band runs as a funnel inside it (out[5] = 1; a forced width keeps the uniform band and U(w) alone)
    const bool funnel = w_use > 0 && band == 0;
    const int32_t* prm_big = params + (size_t)big * params_stride;
    std::vector<BandRange> rg_big((size_t)out[3]);
    if (funnel) {
        funnel_ranges(n_arr[big], m_arr[big], prm_big, w_use, rg_big.data());
        run = 0;
        for (const BandRange& r : rg_big) run += r.gh - r.gl;
        out[5] = 1;
    }
    out[2] = (int32_t)(run * 1000 / all);
    const int w_show = w_use > 0 ? w_use : std::max(w_rule, 0);
    if (ranges_out)
        for (int s = 0; s < out[3] && 2 * s + 1 < ranges_cap; ++s) {
            const BandRange r = funnel ? rg_big[s] : band_groups(n_arr[big], m_arr[big], w_show, s);
            ranges_out[2 * s] = r.gl; ranges_out[2 * s + 1] = r.gh;
        }
    if (u_out && w_use > 0)
        for (int p = 0; p < nprob; ++p)
            u_out[p] = (params_stride == 0 && p > 0 && n_arr[p] == n_arr[p - 1] && m_arr[p] == m_arr[p - 1])
                           ? u_out[p - 1]
                           : clamp_i32(band_bound(n_arr[p], m_arr[p], params + (size_t)p * params_stride, w_use));
    return TA_OK;
}

// Suf(i, j) of nw_band.h for rn = n - i rows and rm = m - j columns left; ap_out (or NULL) = a+, the best single step
extern "C" int32_t ta_nw2_funnel_suf(int32_t rn, int32_t rm, const int32_t* params, int32_t* ap_out) {
    if (!params || rn < 0 || rm < 0) return INT32_MAX;
    const FunnelSys f = funnel_sys(params);
    if (ap_out) *ap_out = f.ap;
    return clamp_i32(funnel_suf<int64_t>(rn, rm, f));
}

// The funnel inside B(w) for every problem of a batch: x0_out[nprob] = the host part of each problem's exit bound
// (funnel_exit0, the exit word's initial value); for problem `big`, ranges_out[2 strips] = (gl, gh) per strip,
// out[0] = 1 if the funnel's own ranges run (0: declined, the band's), out[1] = share of its groups in 1/1000.
// All pointers [host].
extern "C" int ta_nw2_funnel_plan(const int32_t* n_arr, const int32_t* m_arr, int32_t nprob, const int32_t* params,
                                  int32_t params_stride, int32_t w, int32_t big, int32_t* x0_out, int32_t* ranges_out,
                                  int32_t ranges_cap, int32_t* out) {
    if (!n_arr || !m_arr || !params || nprob < 0 || w < 2 || (params_stride != 0 && params_stride != 6) ||
        (nprob > 0 && (big < 0 || big >= nprob)))
        return ta_fail(TA_EINVAL, "bad argument");
    // The ranges (funnel_ok once, then a range per strip) and the exit bound's host part (a pass over n + m boundary
    // cells) are functions of the shape and the six parameters: worked out once per distinct (n, m, system) of the batch.
    std::vector<BandRange> rg;
    std::map<std::array<int32_t, 8>, int32_t> x0_of;
    for (int p = 0; p < nprob; ++p) {
        const int n = n_arr[p], m = m_arr[p];
        if (n < 0 || m < 0 || n > kBandMaxLen || m > kBandMaxLen) return ta_fail(TA_EINVAL, "size outside the band's range");
        if (n == 0 || m == 0) { if (x0_out) x0_out[p] = 0; continue; }
        const int32_t* prm = params + (size_t)p * params_stride;
        const std::array<int32_t, 8> key{n, m, prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
        const auto hit = x0_of.find(key);
        if (hit != x0_of.end() && p != big) { if (x0_out) x0_out[p] = hit->second; continue; }
        rg.resize(PtrLayout<4>::nstrips(n));
        const bool own = funnel_ranges(n, m, prm, w, rg.data());
        const int32_t x0 = hit != x0_of.end() ? hit->second : clamp_i32(funnel_exit0(n, m, prm, rg.data()));
        x0_of[key] = x0;
        if (x0_out) x0_out[p] = x0;
        if (p == big) {
            int64_t run = 0;
            for (size_t s = 0; s < rg.size(); ++s) {
                run += rg[s].gh - rg[s].gl;
                if (ranges_out && 2 * (int)s + 1 < ranges_cap) { ranges_out[2 * s] = rg[s].gl; ranges_out[2 * s + 1] = rg[s].gh; }
            }
            if (out) {
                out[0] = own ? 1 : 0;
                out[1] = (int32_t)(run * 1000 / ((int64_t)rg.size() * PtrLayout<4>::ngroups(m)));
            }
        }
    }
    return TA_OK;
}

static hipError_t launch_score(NwArgs a, int max_n, int max_m, uint32_t flags, hipStream_t st, const int32_t* band_x0 = nullptr) {
    const P1Plan pl = plan_phase1(max_n, max_m, flags, a.nprob, a.band_w > 0);   // (a band by the rule: the same plan either way)
    if (pl.lds > 160 * 1024) return hipErrorInvalidValue;
    a.apad = pl.apad;
    if (a.band_w > 0) {
        if (pl.mode != 2 || !a.band_u || !a.band_ok) return hipErrorInvalidValue;
        if (a.band_cert) {
            if (!band_x0) return hipErrorInvalidValue;
            if (a.lcs) {
                const int alphabet = (int)((flags >> TA_NW_ALPHABET_SHIFT) & 0xFFu);
                if (pl.w == 8) return launch_score_funnel_lcs<8>(a, band_x0, pl.lds, pl.samego, alphabet, st);
                if (pl.w == 4) return launch_score_funnel_lcs<4>(a, band_x0, pl.lds, pl.samego, alphabet, st);
                return hipErrorInvalidValue;
            }
            if (pl.w == 8) return launch_score_funnel<8>(a, band_x0, pl.lds, pl.samego, st);
            if (pl.w == 4) return launch_score_funnel<4>(a, band_x0, pl.lds, pl.samego, st);
            return hipErrorInvalidValue;
        }
        if (pl.w == 8) return launch_score_band<8>(a, pl.lds, pl.samego, st);
        if (pl.w == 4) return launch_score_band<4>(a, pl.lds, pl.samego, st);
        return hipErrorInvalidValue;
    }
    switch (pl.w) {
    case 8: return launch_score_w<8>(a, pl.lds, pl.mode == 2, pl.samego, pl.codes8, st);
    case 4: return launch_score_w<4>(a, pl.lds, pl.mode == 2, pl.samego, pl.codes8, st);
    case 2: return launch_score_w<2>(a, pl.lds, pl.mode == 2, pl.samego, pl.codes8, st);
    default: return launch_score_w<1>(a, pl.lds, pl.mode == 2, pl.samego, pl.codes8, st);
    }
}

// Phase-2 launch shape: 1, 2 or 4 = waves per problem (nw_trace2_kernel / nw_trace2w_kernel), 3 = two problems per wave
// on half-strips (nw_trace2h_kernel), 5 / 6 = two / four waves per PAIR of problems on half-strips
// (nw_trace2hw_kernel).  By batch size, from measurements at 2048^2 (tools/tb_waves_time.py,
// profiles/r04_traceback_waves_per_problem.txt; ms with 1 / 2 / 4 waves / pairs / pairs x 2 / pairs x 4):
//    64 x 0.63 / 0.36 / 0.22 / 0.86 /  --  /  --        768 x 0.66 / 0.50 / 0.48 / 0.87 / 0.66 / 0.46
//  1024 x 0.67 / 0.52 / 0.56 / 0.87 / 0.67 / 0.48      1280 x 0.91 / 0.78 / 0.72 / 0.88 / 0.68 / 0.73
//  1536 x 0.91 / 0.97 / 0.84 / 0.89 / 0.68 / 0.73      2048 x 0.93 / 1.02 / 1.11 / 0.91 / 0.72 / 0.90
//  3072 x 1.21 / 1.51 / 1.65 / 1.23 / 1.34 / 1.34      4096 x 1.49 / 2.06 / 2.16 / 1.24 / 1.41 / 1.75
// and 4096 x 4096^2 2.88 / 3.93 / 4.31 / 2.45 / 2.86 / 3.55 (four-wave workgroups hold 75 - 81 KB of LDS: two per CU).
// The pair kernels only when the batch shares one scoring system (their halves run in lockstep, and problems scored
// differently have paths of very different length).
extern "C" int32_t ta_nw2_traceback_plan(int32_t nprob, int32_t params_stride, uint32_t flags) {
    const int tbw = (int)((flags >> TA_NW_TBWAVES_SHIFT) & 0x7u);
    if (tbw >= 1 && tbw <= 6) return tbw;
    if (nprob <= 832) return 4;
    if (params_stride != 0) return nprob <= 1088 ? 2 : nprob <= 1600 ? 4 : 1;
    if (nprob <= 1088) return 6;
    if (nprob <= 2560) return 5;
    return 3;
}

// TA_NW_CHECK_IDS: every token id of the batch against the bound the caller's flags assert (one workgroup per problem)
__global__ __launch_bounds__(256) void nw_check_ids_kernel(NwArgs a, int bound, int* bad) {
    const int p = blockIdx.x;
    int mine = 0;
    for (int64_t i = a.t_off[p] + threadIdx.x; i < a.t_off[p + 1]; i += 256) mine |= (unsigned)a.t_codes[i] >= (unsigned)bound;
    for (int64_t i = a.o_off[p] + threadIdx.x; i < a.o_off[p + 1]; i += 256) mine |= (unsigned)a.o_codes[i] >= (unsigned)bound;
    if (__ballot(mine) != 0 && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

static int check_ids(const NwArgs& a, uint32_t flags, hipStream_t st) {
    int bound = 65535;                                        // the ABI's own limit (ids < 65536; 65535 is the pad code)
    if (flags & TA_NW_CODES8) bound = 255;
    const int alpha = (int)((flags >> TA_NW_ALPHABET_SHIFT) & 0xFFu);
    if (alpha > 0 && !(flags & TA_NW_NO_PROFILE)) bound = alpha < bound ? alpha : bound;
    // stream-ordered allocation: hipMalloc / hipFree would synchronise the whole DEVICE (the page pipeline's other streams
    // included), this call waits for `st` alone
    int* bad = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&bad), sizeof(int), st);
    if (e != hipSuccess) return ta_fail_hip(e, "TA_NW_CHECK_IDS: hipMallocAsync");
    int host_bad = 0;
    e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(nw_check_ids_kernel, dim3(a.nprob), dim3(256), 0, st, a, bound, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    (void)hipFreeAsync(bad, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return ta_fail_hip(e, "TA_NW_CHECK_IDS");
    if (host_bad) return ta_fail(TA_EINVAL, "a token id is outside the range the flags assert (TA_NW_CODES8 / TA_NW_ALPHABET)");
    return TA_OK;
}

extern "C" int ta_nw2_batch(const int32_t* t_codes, const int64_t* t_off,
                            const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                            const int32_t* params, int32_t params_stride,
                            uint8_t* ws, const int64_t* ws_off,
                            uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                            int32_t max_n, int32_t max_m, int64_t score_bound,
                            uint32_t flags, void* stream) {
    return ta_nw2_batch_band(t_codes, t_off, o_codes, o_off, nprob, params, params_stride, ws, ws_off, ops_out, ops_off,
                             ops_len, max_n, max_m, score_bound, flags, 0, nullptr, nullptr, stream);
}

extern "C" int ta_nw2_batch_band(const int32_t* t_codes, const int64_t* t_off,
                                 const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                                 const int32_t* params, int32_t params_stride,
                                 uint8_t* ws, const int64_t* ws_off,
                                 uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                                 int32_t max_n, int32_t max_m, int64_t score_bound,
                                 uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok, void* stream) {
    return ta_nw2_batch_funnel(t_codes, t_off, o_codes, o_off, nprob, params, params_stride, ws, ws_off, ops_out, ops_off,
                               ops_len, max_n, max_m, score_bound, flags, band_w, band_u, band_ok, nullptr, nullptr, stream);
}

extern "C" int ta_nw2_batch_funnel(const int32_t* t_codes, const int64_t* t_off,
                                   const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                                   const int32_t* params, int32_t params_stride,
                                   uint8_t* ws, const int64_t* ws_off,
                                   uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                                   int32_t max_n, int32_t max_m, int64_t score_bound,
                                   uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok,
                                   const int32_t* band_x0, int32_t* band_cert, void* stream) {
    return ta_nw2_batch_funnel_lcs(t_codes, t_off, o_codes, o_off, nprob, params, params_stride, ws, ws_off, ops_out, ops_off,
                                   ops_len, max_n, max_m, score_bound, flags, band_w, band_u, band_ok, band_x0, band_cert,
                                   nullptr, stream);
}

extern "C" int64_t ta_nw2_funnel_lcs_words(int32_t nprob, int32_t max_n) {
    if (nprob < 0 || max_n < 0 || max_n > kBandMaxLen) return -1;
    return (int64_t)nprob * lcs_stride(max_n);
}
extern "C" int ta_nw2_funnel_ranges(int32_t n, int32_t m, const int32_t* params, int32_t w, int32_t scale_pm,
                                    int32_t* ranges_out, int32_t ranges_cap, int32_t* out) {
    if (!params || n <= 0 || m <= 0 || n > kBandMaxLen || m > kBandMaxLen || w < 2 ||
        (scale_pm != kFunnelFullPm && scale_pm != kFunnelLcsScalePm))
        return ta_fail(TA_EINVAL, "bad argument (scale_pm: 1000 or ta_nw2_funnel_lcs_scale_pm())");
    std::vector<BandRange> rg(PtrLayout<4>::nstrips(n));
    const bool own = scale_pm == kFunnelFullPm ? funnel_ranges(n, m, params, w, rg.data())
                                               : funnel_ranges<kFunnelLcsScalePm>(n, m, params, w, rg.data());
    int64_t run = 0;
    for (size_t s = 0; s < rg.size(); ++s) {
        run += rg[s].gh - rg[s].gl;
        if (ranges_out && 2 * (int)s + 1 < ranges_cap) { ranges_out[2 * s] = rg[s].gl; ranges_out[2 * s + 1] = rg[s].gh; }
    }
    if (out) {
        out[0] = own ? 1 : 0;
        out[1] = (int32_t)(run * 1000 / ((int64_t)rg.size() * PtrLayout<4>::ngroups(m)));
    }
    return TA_OK;
}
extern "C" int32_t ta_nw2_funnel_lcs_scale_pm(void) { return kFunnelLcsScalePm; }
extern "C" int32_t ta_nw2_funnel_lcs_max_m(void) { return kLcsMaxM; }
extern "C" int32_t ta_nw2_funnel_suf_lcs(int32_t rn, int32_t rm, int32_t l, const int32_t* params) {
    if (!params || rn < 0 || rm < 0 || l < 0) return INT32_MAX;
    return clamp_i32(funnel_suf_lcs<int64_t>(rn, rm, l, funnel_sys(params), funnel_lcs_sys(params)));
}

extern "C" int ta_nw2_batch_funnel_lcs(const int32_t* t_codes, const int64_t* t_off,
                                       const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                                       const int32_t* params, int32_t params_stride,
                                       uint8_t* ws, const int64_t* ws_off,
                                       uint8_t* ops_out, const int64_t* ops_off, int32_t* ops_len,
                                       int32_t max_n, int32_t max_m, int64_t score_bound,
                                       uint32_t flags, int32_t band_w, const int32_t* band_u, int32_t* band_ok,
                                       const int32_t* band_x0, int32_t* band_cert, int32_t* lcs, void* stream) {
    if (lcs && !band_cert) return ta_fail(TA_EINVAL, "funnel-lcs: the table goes with the funnel's certificate array");
    if ((band_x0 == nullptr) != (band_cert == nullptr) || (band_cert && band_w < 2))
        return ta_fail(TA_EINVAL, "funnel: the exit words' host part and the certificate array, with a band width >= 2, or neither");
    if (nprob < 0 || max_n < 0 || max_m < 0) return ta_fail(TA_EINVAL, "negative size");
    if (band_w < 0 || (band_w > 0 && (!band_u || !band_ok || band_w == 1)))
        return ta_fail(TA_EINVAL, "band: width >= 2 with its bound and list arrays, or 0");
    if (nprob == 0) return TA_OK;
    if (!t_off || !o_off || !params || !ws_off || !ops_off || !ops_len)
        return ta_fail(TA_EINVAL, "null pointer argument");
    if (params_stride != 0 && params_stride != 6) return ta_fail(TA_EINVAL, "params_stride must be 0 or 6");
    if (score_bound < 0 || score_bound >= (1ll << 23))
        return ta_fail(TA_ERANGE, "(n+m+2)*max|param| does not fit the 32-bit encoded scores");
    if (max_m > ta_nw2_max_m()) return ta_fail(TA_ELIMIT, "m exceeds the LDS capacity for the OCR codes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    NwArgs a{t_codes, t_off, o_codes, o_off, params, params_stride, ws, ws_off,
             ops_out, ops_off, ops_len, nprob};
    a.band_w = band_w; a.band_u = band_u; a.band_ok = band_ok; a.band_cert = band_cert;
    a.lcs = max_n <= kBandMaxLen ? lcs : nullptr; a.lcs_max_n = max_n;
    if ((flags & TA_NW_FILL) && max_n > 0 && max_m > 0) {
        if (!t_codes || !o_codes || !ws) return ta_fail(TA_EINVAL, "null code/workspace pointer");
        if (flags & TA_NW_CHECK_IDS) {
            const int rc = check_ids(a, flags, st);
            if (rc != TA_OK) return rc;
        }
        const hipError_t e = launch_score(a, max_n, max_m, flags, st, band_x0);
        if (e != hipSuccess) return ta_fail_hip(e, "nw_score_kernel launch");
    }
    if (flags & TA_NW_TRACEBACK) {
        if (!ops_out && (max_n + max_m) > 0) return ta_fail(TA_EINVAL, "null ops_out");
        // launch shape by batch size (ta_nw2_traceback_plan above): several waves per problem that speculate along the
        // path for small and medium batches, two problems per wave on half-strips for batches that fill the chip and
        // share one scoring system -- the two halves of a wave run in lockstep, and problems scored differently have
        // paths of very different length (the grid search, 2187 x 800 x 900 with a system per problem: 0.76 ms against
        // 0.59 with one wave per problem; the same shape under one system 0.52 against 0.53)
        // every length starts as -1: the multi-wave tracebacks wait for each other's tokens with BOUNDED spins, and a walk
        // that gave up must not leave the length of an earlier run (or of nothing) behind -- the host refuses a negative one
        {
            const hipError_t em = hipMemsetAsync(ops_len, 0xFF, sizeof(int32_t) * (size_t)nprob, st);
            if (em != hipSuccess) return ta_fail_hip(em, "ops_len reset");
        }
        const int tbw = ta_nw2_traceback_plan(nprob, params_stride, flags);
        if (tbw == 3) hipLaunchKernelGGL(nw_trace2h_kernel, dim3((nprob + 1) / 2), dim3(64), 0, st, a);
        else if (tbw == 5) hipLaunchKernelGGL(nw_trace2hw_kernel<2>, dim3((nprob + 1) / 2), dim3(128), 0, st, a);
        else if (tbw == 6) hipLaunchKernelGGL(nw_trace2hw_kernel<4>, dim3((nprob + 1) / 2), dim3(256), 0, st, a);
        else if (tbw == 4) hipLaunchKernelGGL(nw_trace2w_kernel<4>, dim3(nprob), dim3(256), 0, st, a);
        else if (tbw == 2) hipLaunchKernelGGL(nw_trace2w_kernel<2>, dim3(nprob), dim3(128), 0, st, a);
        else hipLaunchKernelGGL(nw_trace2_kernel, dim3(nprob), dim3(64), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return ta_fail_hip(e, "phase 2 (traceback) launch");
    }
    return TA_OK;
}
