// ta_nw_span.hip -- where in a longer transcript does a page's text lie?  Score-only wavefront fill of the affine-gap
// table with a FREE column 0 (an alignment of the whole OCR string may start at any transcript position) in which
// every value carries its ORIGIN, the row it left column 0 at; the maximum of the last column then names the span
// (i0, i1) the global aligner is given.  Definition of record: DESIGN.md section 4.6; checker tests/span_ref.py; the
// cell, boundary, lane step and the reduction are nw_span.h, which tests/native/sim_span.cpp replays on the CPU.
//
// Shape: that of the one-pass fill (ta_nw.hip).  One workgroup per problem, W waves; strips of 64 * R rows, wave w
// takes strips w, w + W, ...; lane l owns R consecutive rows and sweeps the columns skewed by its lane id, so the row
// above arrives by DPP wave_shr:1; a strip's bottom row (V~, D: two values per column) goes to the wave on the next
// strip through ONE hand-off row in LDS, which every strip overwrites behind its own reads, guarded by progress words
// in LDS that the consumer polls.  All waves of a workgroup are resident, the waits are inside the workgroup, nothing
// waits between workgroups.  Nothing is written to HBM but the result: int32 (i0, i1, score) per problem.
//
// The CHAINED search (ta_nw_span_chain; checker tests/span_chain_ref.py; host replay
// tests/native/sim_span_chain.cpp) puts the pages of a book in reading order: the same kernel in a second instantiation
// whose column 0 and row 0 carry the previous page's renormalised prefix maximum and which writes every row's
// last-column value and origin to HBM, a carry kernel (tiled prefix maximum) and a walk back from the last page; one
// fill and one carry launch per page index, ordered by the stream alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "nw_cell.h"
#include "nw_hw.h"
#include "nw_span.h"
#include "ta_common.h"

namespace ta {

struct SpanArgs {
    const int32_t* t_codes; const int64_t* t_start; const int32_t* t_len;
    const int32_t* o_codes; const int64_t* o_off;
    const int32_t* params; int32_t params_stride;
    int32_t* out;
    int32_t nprob;
};

constexpr int kSpanR = 4;                      // rows per lane: strips of 256 rows
constexpr int kSpanMaxM = 8000;                // 16 bytes of hand-off row + 2 bytes of code per OCR token: 142 KiB of LDS
constexpr int kSpanMaxParam = 1 << 19;         // |3 p| < 2^21: the substitution constants' low dwords are zero
constexpr int kSpanDummy = 68;                 // scratch entries for the bottom-row writes of lanes 0 .. 62 (lane + q, q < 4)

// LDS carve (dynamic): double2 hvd[m + 2] | double2 dummy[kSpanDummy] | uint16 ocode[kOPad + m + kOTail] | int prog[16]
//                      | int res[8][4]
struct SpanLds {
    size_t hvd_bytes, dummy_bytes, oc_bytes, total;
    __host__ __device__ explicit SpanLds(int m) {
        hvd_bytes = (size_t)(m + 2) * 16;
        dummy_bytes = (size_t)kSpanDummy * 16;
        oc_bytes = ((size_t)(kOPad + m + kOTail) * 2 + 15) & ~(size_t)15;
        total = hvd_bytes + dummy_bytes + oc_bytes + 64 + 128;
    }
};

// lane l receives the two values of lane l - 1, lane 0 keeps what it holds (wave_shr:1 on the four dwords)
__device__ __forceinline__ void span_shr1(SpanVal& v_io, SpanVal v_src, SpanVal& d_io, SpanVal d_src) {
    int vl = __double2loint(v_io), vh = __double2hiint(v_io), dl = __double2loint(d_io), dh = __double2hiint(d_io);
    wave_shr1_pair_sched(vl, __double2loint(v_src), vh, __double2hiint(v_src));
    wave_shr1_pair_sched(dl, __double2loint(d_src), dh, __double2hiint(d_src));
    v_io = __hiloint2double(vh, vl);
    d_io = __hiloint2double(dh, dl);
}

// ---- the chained search: the pages of a book in reading order in one transcript ----
// Step s = one launch of the fill and one of the carry for page s of every chain that has one; the stream's order is
// the only dependency between the steps, no workgroup waits for another.  The chains are ranked by their page counts
// (more pages first) once per call, so that step s is a launch of exactly the chains that have a page s.
struct SpanChainArgs {
    const int32_t* t_codes; const int64_t* t_start; const int32_t* t_len;
    const int32_t* o_codes; const int64_t* o_off; const int32_t* page_first;
    const int32_t* params; int32_t params_stride;
    int32_t* order;                            // [nchains] chain ids, more pages first
    int32_t *F, *O, *G;                        // [npages][stride]: last column, its origins, the carry
    int64_t stride;
    int32_t* out; int64_t* total;
    int32_t nchains, npages, max_n, max_m, floor, step;
};
constexpr int kChainThreads = 256;

// what every kernel of the chain knows of its problem; ok = false: nothing to do, or a chain refused as a whole
struct SpanChainProblem {
    int chain, first, count, n;
    const int32_t* prm;
    bool ok;
};
__device__ __forceinline__ SpanChainProblem span_chain_problem(const SpanChainArgs& a, int chain) {
    SpanChainProblem q;
    q.chain = chain;
    q.first = a.page_first[chain];
    q.count = a.page_first[chain + 1] - q.first;
    q.n = a.t_len[chain];
    q.prm = a.params + (size_t)chain * a.params_stride;
    q.ok = q.first >= 0 && q.count >= 0 && (int64_t)q.first + q.count <= a.npages;
    if (q.ok) {
        const CellConsts c = make_consts(q.prm[0], q.prm[1], q.prm[2], q.prm[3], q.prm[4], q.prm[5]);
        const SpanConsts k = span_consts(c, q.prm[0], q.prm[1]);
        int64_t max_m = 0, min_m = 0;          // every page of the chain must fit: a page refused refuses the chain
        for (int p = q.first; p < q.first + q.count; ++p) {
            const int64_t m = a.o_off[p + 1] - a.o_off[p];
            max_m = max(max_m, m);
            min_m = min(min_m, m);
        }
        q.ok = min_m >= 0 && max_m <= a.max_m && span_chain_fits(k, q.n, (int)max_m, a.max_n, a.max_m);
    }
    return q;
}

// One problem's fill by one workgroup of W waves.  CHAIN = false: the single search -- the free column 0, the maximum of
// the last column to out[3].  CHAIN = true: page a.step of a chain (ta_nw_span_chain) -- column 0 and row 0 carry G (the
// previous page's carry array; NULL on page 0: the free 0), every row's last-column value and origin go to F / O (this
// page's arrays) and nothing is reduced.
template <int W, bool CHAIN = false>
__global__ __launch_bounds__(W * 64) void nw_span_kernel(std::conditional_t<CHAIN, SpanChainArgs, SpanArgs> a) {
    constexpr int R = kSpanR;
    using L = PtrLayout<R>;                    // strips, groups and steps as the aligner counts them (no pointer bytes here)
    constexpr int SPG = L::SPG;
    constexpr int CHK = 4;                     // groups between two looks at the progress word of the strip above
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    int p = blockIdx.x;                        // whose transcript and parameters
    int pg = p;                                // whose OCR text: the problem's own, or the chain's page of this step
    const int32_t* G = nullptr;                // CHAIN only: slot 0 of the carry in, of the last column and origins out
    int32_t *F = nullptr, *O = nullptr;
    if constexpr (CHAIN) {
        const SpanChainProblem q = span_chain_problem(a, a.order[p]);
        if (!q.ok || a.step >= q.count) return;
        p = q.chain;
        pg = q.first + a.step;
        const int64_t at = (int64_t)pg * a.stride;
        G = a.step ? a.G + (at - a.stride) : nullptr;
        F = a.F + at;
        O = a.O + at;
    }
    const int tid = threadIdx.x;
    const int n = a.t_len[p];
    const int64_t t0 = a.t_start[p], o0 = a.o_off[pg];
    const int m = (int)(a.o_off[pg + 1] - o0);
    int32_t* const out = a.out + (size_t)pg * 3;
    if (n <= 0 || m <= 0) {
        if constexpr (CHAIN) {                 // m = 0: F(i) = G'(i), origin i; n = 0: row 0 alone, G'(0) - m
            for (int i = tid; i <= (m <= 0 ? n : 0); i += W * 64)
                span_trivial_last(i, m > 0 ? m : 0, G ? G[i + kSpanChainPad] : 0, F, O);
        } else {                               // m = 0: (0, 0) with score 0; n = 0: (0, 0) with score -m (row 0)
            if (tid == 0) { out[0] = 0; out[1] = 0; out[2] = m > 0 ? -m : 0; }
        }
        return;
    }
    const int32_t* prm = a.params + (size_t)p * a.params_stride;
    const CellConsts c = make_consts(prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]);
    const SpanConsts k = span_consts(c, prm[0], prm[1]);
    int hi_mat = __double2hiint(k.cmat), hi_mis = __double2hiint(k.cmis);
    if constexpr (!CHAIN) {
        if ((__double2loint(k.cmat) | __double2loint(k.cmis)) != 0) { // parameters beyond kSpanMaxParam: refused, not mis-scored
            if (tid == 0) { out[0] = -1; out[1] = -1; out[2] = INT32_MIN; }
            return;
        }
    }
    asm volatile("" : "+v"(hi_mat), "+v"(hi_mis));                   // the two select constants stay in VGPRs
    // t == o ? match : mismatch as a value: the two constants differ in the high dword only
    const auto score = [&](int t, int o) -> SpanVal { return __hiloint2double(t == o ? hi_mat : hi_mis, 0); };

    const SpanLds lds(m);
    double2* hvd = reinterpret_cast<double2*>(smem);
    double2* dummy = reinterpret_cast<double2*>(smem + lds.hvd_bytes);
    uint16_t* ocode = reinterpret_cast<uint16_t*>(smem + lds.hvd_bytes + lds.dummy_bytes);
    int* prog = reinterpret_cast<int*>(smem + lds.hvd_bytes + lds.dummy_bytes + lds.oc_bytes);
    int* res = prog + 16;

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    stage_ocr_codes(ocode, a.o_codes, o0, m, 0, (uint16_t)0xFFFF, tid, W * 64);
    if constexpr (CHAIN) {
        const int g0 = G ? G[kSpanChainPad] : 0;
        for (int j = tid; j <= m; j += W * 64) hvd[j] = make_double2(span_V_row0(c, j, g0), span_D_row0(c, j, g0));
        if (tid == 0) span_trivial_last(0, m, g0, F, O);
    } else {
        for (int j = tid; j <= m; j += W * 64) hvd[j] = make_double2(span_V_row0(c, j), span_D_row0(c, j));
    }
    if (tid < 16) prog[tid] = 0;
    __syncthreads();

    const int nstrips = L::nstrips(n);
    const int ngroups = L::ngroups(m);
    const int prev_wave = (wave + W - 1) % W;
    // groups [g_lo, g_hi) are "steady": every lane is inside 1 <= j <= m on every step
    const int g_lo = (63 + SPG - 1) / SPG;
    const int g_hi = m / SPG;
    SpanBest wbest = span_none();              // best of this wave's strips (wave-uniform)
    int pass = 0;

    for (int s = wave; s < nstrips; s += W, ++pass) {
        SpanVal D[R], V[R], H[R], dsave;
        int tc[R];
        const int row0 = s * L::SR + lane * R;             // 0-based index of this lane's first row
        if constexpr (CHAIN)
            span_lane_boundary_chain<R>(c, row0, D, V, H, dsave,
                                        [&](int i) { return (G && i <= n) ? G[i + kSpanChainPad] : 0; },
                                        [&](int r, int i) { tc[r] = (i <= n) ? a.t_codes[t0 + i - 1] : -1; });
        else
            span_lane_boundary<R>(c, row0, D, V, H, dsave,
                                  [&](int r, int i) { tc[r] = (i <= n) ? a.t_codes[t0 + i - 1] : -1; });
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" :: "v"(tc[r]));   // retire the code loads before the group loops
        const bool lane_has_rows = row0 < n;
        const int prod_pass = (wave == 0) ? pass - 1 : pass;   // pass in which prev_wave did strip s - 1

        // Hand-off protocol of ta_nw.hip's narrow launch: strips of one workgroup hand their rows over in LDS, and the
        // LDS executes a wave's operations in order -- the producer's entries, then its progress word; the consumer's
        // read of the word, then of the entries.  The strip above must be CHK + 1 groups ahead before a span is touched.
        auto wait_span = [&](int g_first) {
            if (s == 0 || W == 1) return;
            // the last step of groups [g_first, g_first + CHK] reads hand-off column min(k_last + 1, m), written by
            // the producer's lane 63 at its step col + 62
            const int k_last = min((g_first + CHK + 1) * SPG - 1, L::nsteps(m) - 1);
            const int col = min(k_last + 1, m);
            const int need_groups = min(ngroups, (col + 62) / SPG + 1);
            wait_progress<__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP, 1>(&prog[prev_wave],
                                                                             prod_pass * ngroups + need_groups);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        // progress is published after groups 0, CHK, 2 CHK, ... and the last: the consumer's needs are 1 mod CHK
        auto publish = [&](int g) {
            if (W == 1) return;
            if ((g % CHK) == 0 || g == ngroups - 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 63)
                    __hip_atomic_store(&prog[wave], pass * ngroups + g + 1, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
        int oc_next[SPG];
        double2 hd_next[SPG];
        auto load_group = [&](int g) {
            const int idx = kOPad + g * SPG - lane;        // o index of step k is k - lane
#pragma unroll
            for (int q = 0; q < SPG; ++q) {
                oc_next[q] = ocode[idx + q];
                hd_next[q] = hvd[min(g * SPG + q + 1, m)]; // lane 0's column at step k is k + 1
            }
        };
        auto prefetch = [&](int g) {
            if (g + 1 < ngroups) {
                if (((g + 1) % CHK) == 0) wait_span(g + 1);
                load_group(g + 1);
            }
        };
        // one group with per-lane activity tests (ramp-up, ramp-down, short rows)
        auto group_edge = [&](int g) {
            int oc[SPG];
            double2 hd[SPG];
#pragma unroll
            for (int q = 0; q < SPG; ++q) { oc[q] = oc_next[q]; hd[q] = hd_next[q]; }
            prefetch(g);
#pragma unroll
            for (int q = 0; q < SPG; ++q) {
                const int kk = g * SPG + q;
                const int j = kk - lane + 1;               // this lane's column at step kk (1-based)
                const bool active = (j >= 1) && (j <= m) && lane_has_rows;
                SpanVal v_up = hd[q].x, d_next = hd[q].y;  // lane 0: the row above; lanes 1 .. 63: from lane - 1
                span_shr1(v_up, V[R - 1], d_next, D[R - 1]);
                if (active) {
                    span_lane_step<R>(score, k, D, V, H, dsave, v_up, d_next, tc, oc[q]);
                    if (lane == 63) hvd[j] = make_double2(V[R - 1], D[R - 1]);
                }
            }
            publish(g);
        };

        wait_span(0);
        load_group(0);
        int g = 0;
        const int e1 = min(g_lo, ngroups);
        for (; g < e1; ++g) group_edge(g);

        if (g < g_hi) {
            // ---- steady state: straight-line code, no EXEC changes.  Lanes whose rows lie below row n compute
            // don't-care values that never reach a valid row (and are left out of the maximum below).  Two groups per
            // iteration with two input buffers, so the back-edge needs no register copies.  Lane 63 writes its bottom
            // row to hvd[j], j = kk - 62; the other lanes a scratch slot, so the store needs no EXEC mask. ----
            double2* wptr = (lane == 63) ? (hvd + (g * SPG - 62)) : (dummy + lane);
            const int winc = (lane == 63) ? SPG : 0;
            int ocA[SPG], ocB[SPG];
            double2 hdA[SPG], hdB[SPG];
#pragma unroll
            for (int q = 0; q < SPG; ++q) { ocA[q] = oc_next[q]; hdA[q] = hd_next[q]; }
            auto fetch = [&](int gn, int (&oc)[SPG], double2 (&hd)[SPG]) {       // inputs of group gn
                if (gn < ngroups) {
                    if ((gn % CHK) == 0) wait_span(gn);
                    const int idx = kOPad + gn * SPG - lane;
#pragma unroll
                    for (int q = 0; q < SPG; ++q) {
                        oc[q] = ocode[idx + q];
                        hd[q] = hvd[min(gn * SPG + q + 1, m)];
                    }
                }
            };
            auto steady = [&](int gg, const int (&oc)[SPG], const double2 (&hd)[SPG]) {
#pragma unroll
                for (int q = 0; q < SPG; ++q) {
                    SpanVal v_up = hd[q].x, d_next = hd[q].y;
                    span_shr1(v_up, V[R - 1], d_next, D[R - 1]);
                    span_lane_step<R>(score, k, D, V, H, dsave, v_up, d_next, tc, oc[q]);
                    wptr[q] = make_double2(V[R - 1], D[R - 1]);
                }
                wptr += winc;
                publish(gg);
            };
            while (g + 1 < g_hi) {
                fetch(g + 1, ocB, hdB);
                steady(g, ocA, hdA);
                fetch(g + 2, ocA, hdA);
                steady(g + 1, ocB, hdB);
                g += 2;
            }
            if (g < g_hi) {
                fetch(g + 1, ocB, hdB);
                steady(g, ocA, hdA);
                ++g;
#pragma unroll
                for (int q = 0; q < SPG; ++q) { oc_next[q] = ocB[q]; hd_next[q] = hdB[q]; }
            } else {
#pragma unroll
                for (int q = 0; q < SPG; ++q) { oc_next[q] = ocA[q]; hd_next[q] = hdA[q]; }
            }
        }
        for (; g < ngroups; ++g) group_edge(g);

        // ---- the last column: D[r] = D(row, m) of the lane's rows ----
        if constexpr (CHAIN) {                 // every row's value and origin, for the carry and the walk back
            if (lane_has_rows) span_store_last<R>(c, row0, n, m, D, F, O);
        } else {                               // wave maximum of (score, -i1), origin alongside
            SpanBest lb = lane_has_rows ? span_lane_best<R>(c, row0, n, m, D) : span_none();
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const SpanBest other{__shfl_xor(lb.score, off), __shfl_xor(lb.i1, off), __shfl_xor(lb.origin, off)};
                lb = span_pick(lb, other);
            }
            wbest = span_pick(wbest, lb);
        }
    }

    if constexpr (!CHAIN) {
        // ---- the waves' results combine through LDS into one store per problem; row 0 (i1 = 0) joins here ----
        if (lane == 0) { res[wave * 4 + 0] = wbest.score; res[wave * 4 + 1] = wbest.i1; res[wave * 4 + 2] = wbest.origin; }
        __syncthreads();
        if (tid == 0) {
            SpanBest b = span_row0(m);
            for (int w = 0; w < W; ++w) b = span_pick(b, SpanBest{res[w * 4 + 0], res[w * 4 + 1], res[w * 4 + 2]});
            out[0] = b.origin; out[1] = b.i1; out[2] = b.score;
        }
    }
}

template <int W>
static hipError_t launch_span(const SpanArgs& a, int max_m, hipStream_t st) {
    const size_t lds = SpanLds(max_m).total;
    hipError_t e = allow_full_lds(&nw_span_kernel<W>);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nw_span_kernel<W>), dim3(a.nprob), dim3(W * 64), lds, st, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kChainThreads) void nw_span_chain_order_kernel(SpanChainArgs a) {
    const int c = blockIdx.x * kChainThreads + threadIdx.x;
    if (c >= a.nchains) return;
    const int mine = a.page_first[c + 1] - a.page_first[c];
    int rank = 0;
    for (int d = 0; d < a.nchains; ++d) {
        const int other = a.page_first[d + 1] - a.page_first[d];
        rank += (other > mine || (other == mine && d < c)) ? 1 : 0;
    }
    a.order[rank] = c;
}

// inclusive maximum scan of one value per lane over the wave, lane order (as ta_forced_omit.hip's wave_max_scan)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ int span_dpp_or_self(int v) {
    return __builtin_amdgcn_update_dpp(v, v, kCtrl, kRowMask, 0xf, false);
}
__device__ __forceinline__ int span_wave_max_scan(int v) {
    v = max(v, span_dpp_or_self<0x111, 0xf>(v));           // row_shr:1
    v = max(v, span_dpp_or_self<0x112, 0xf>(v));           // row_shr:2
    v = max(v, span_dpp_or_self<0x114, 0xf>(v));           // row_shr:4
    v = max(v, span_dpp_or_self<0x118, 0xf>(v));           // row_shr:8
    v = max(v, span_dpp_or_self<0x142, 0xa>(v));           // row_bcast:15 into rows 1 and 3
    v = max(v, span_dpp_or_self<0x143, 0xc>(v));           // row_bcast:31 into rows 2 and 3
    return v;
}

// The carry of the page just filled: one workgroup per chain.  Pass 1: top = the maximum of F.  Pass 2: the inclusive
// prefix maximum in tiles of kChainThreads * kSpanCarryPer rows -- a lane's own rows serially, the lanes of a wave by
// DPP, the waves through LDS, a running value from tile to tile -- renormalised by top and clamped at -floor.
__global__ __launch_bounds__(kChainThreads) void nw_span_carry_kernel(SpanChainArgs a) {
    constexpr int NW = kChainThreads / 64;
    __shared__ int wave_max[2][NW];
    const SpanChainProblem q = span_chain_problem(a, a.order[blockIdx.x]);
    if (!q.ok || a.step + 1 >= q.count) return;            // (a chain's last page hands nothing on)
    const int64_t at = (int64_t)(q.first + a.step) * a.stride;
    const int32_t* F = a.F + at;
    int32_t* G = a.G + at;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = q.n;

    int top = kSpanNone;
    for (int i = tid; i <= n; i += kChainThreads) top = max(top, F[i + kSpanChainPad]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top = max(top, __shfl_xor(top, off));
    if (lane == 0) wave_max[0][wave] = top;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) top = max(top, wave_max[0][w]);

    int running = kSpanNone;                               // the maximum of every row in front of the tile
    int buf = 1;
    for (int base = 0; base <= n; base += kChainThreads * kSpanCarryPer, buf ^= 1) {
        const int first = base + tid * kSpanCarryPer;
        int v[kSpanCarryPer];
        const int mine = span_carry_load(F, first, n, v);
        const int incl = span_wave_max_scan(mine);         // lanes 0 .. lane of this wave
        if (lane == 63) wave_max[buf][wave] = incl;
        int before = __shfl_up(incl, 1);                   // lanes in front of this one
        if (lane == 0) before = kSpanNone;
        __syncthreads();                                   // (two buffers: the next tile's writes need no second barrier)
        int tile = kSpanNone;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (w < wave) before = max(before, wave_max[buf][w]);
            tile = max(tile, wave_max[buf][w]);
        }
        span_carry_store(G, first, n, v, max(before, running), top, a.floor);
        running = max(running, tile);
    }
}

// The walk back: one workgroup per chain, its pages in descending order; per page a reduction over the rows up to the
// limit (span_walk_pick: largest F, then smallest row), then the origin of the winner becomes the next limit.
__global__ __launch_bounds__(kChainThreads) void nw_span_walk_kernel(SpanChainArgs a) {
    constexpr int NW = kChainThreads / 64;
    __shared__ int res[NW][2];
    __shared__ int next_limit;
    const SpanChainProblem q = span_chain_problem(a, blockIdx.x);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!(q.first >= 0 && q.count >= 0 && (int64_t)q.first + q.count <= a.npages)) {
        if (tid == 0) a.total[q.chain] = INT64_MIN;        // page_first itself is broken: no page of this chain is known
        return;
    }
    if (!q.ok) {
        for (int p = tid; p < q.count; p += kChainThreads) {
            int32_t* out = a.out + (size_t)(q.first + p) * 3;
            out[0] = -1; out[1] = -1; out[2] = INT32_MIN;
        }
        if (tid == 0) a.total[q.chain] = INT64_MIN;
        return;
    }
    int limit = q.n;
    long long total = 0;
    for (int p = q.count - 1; p >= 0; --p) {
        const int64_t at = (int64_t)(q.first + p) * a.stride;
        SpanWalk w = span_walk_lane(a.F + at, limit, tid, kChainThreads);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) w = span_walk_pick(w, SpanWalk{__shfl_xor(w.f, off), __shfl_xor(w.j, off)});
        if (lane == 0) { res[wave][0] = w.f; res[wave][1] = w.j; }
        __syncthreads();
        if (tid == 0) {
            SpanWalk b = span_walk_none();
            for (int x = 0; x < NW; ++x) b = span_walk_pick(b, SpanWalk{res[x][0], res[x][1]});
            int32_t* out = a.out + (size_t)(q.first + p) * 3;
            span_walk_result(b, a.O + at, p ? a.G + (at - a.stride) : nullptr, out);
            total += out[2];
            next_limit = out[0];
        }
        __syncthreads();
        limit = next_limit;
    }
    if (tid == 0) a.total[q.chain] = total;
}

struct SpanChainLayout {
    int64_t stride, order_bytes, array_bytes, total;
    SpanChainLayout(int64_t nchains, int64_t npages, int max_n) {
        stride = span_chain_stride(max_n);
        order_bytes = (nchains * 4 + 15) & ~(int64_t)15;
        array_bytes = npages * stride * 4;
        total = order_bytes + 3 * array_bytes;
    }
};

template <int W>
static hipError_t launch_span_chain(const SpanChainArgs& a, int count, hipStream_t st) {
    const size_t lds = SpanLds(a.max_m).total;
    hipError_t e = allow_full_lds(&nw_span_kernel<W, true>);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nw_span_kernel<W, true>), dim3(count), dim3(W * 64), lds, st, a);
    return hipGetLastError();
}

}  // namespace ta

using namespace ta;

extern "C" int32_t ta_nw_span_max_m(void) { return kSpanMaxM; }

extern "C" int64_t ta_nw_span_workspace_bytes(int32_t nprob, int32_t max_n, int32_t max_m) {
    if (nprob < 0 || max_n < 0 || max_m < 0) return TA_EINVAL;
    if (max_m > kSpanMaxM || max_n > kSpanMaxN) return TA_EINVAL;
    return 0;                                  // everything between the strips of a problem lives in LDS
}

extern "C" int ta_nw_span_batch(const int32_t* t_codes, const int64_t* t_start, const int32_t* t_len,
                                const int32_t* o_codes, const int64_t* o_off, int32_t nprob,
                                const int32_t* params, int32_t params_stride, int32_t* out,
                                int32_t max_n, int32_t max_m, int64_t score_bound, int32_t max_param,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    if (nprob < 0 || max_n < 0 || max_m < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative size");
    if (nprob == 0) return TA_OK;
    if (!t_start || !t_len || !o_off || !params || !out) return ta_fail(TA_EINVAL, "null pointer argument");
    if (params_stride != 0 && params_stride != 6) return ta_fail(TA_EINVAL, "params_stride must be 0 or 6");
    if (max_m > kSpanMaxM) return ta_fail(TA_EINVAL, "m exceeds the LDS hand-off row of the span fill");
    if (max_n > kSpanMaxN) return ta_fail(TA_EINVAL, "n exceeds the origin field of the span fill (2^28 - 1)");
    if (score_bound < 0 || score_bound >= (1ll << 23))
        return ta_fail(TA_ERANGE, "(n+m+2)*max|param| does not fit the 24-bit score field");
    if (max_param < 0 || max_param > kSpanMaxParam)
        return ta_fail(TA_ERANGE, "scoring parameters too large for the span fill (2^19)");
    if (max_n > 0 && max_m > 0 && (!t_codes || !o_codes)) return ta_fail(TA_EINVAL, "null code pointer");
    (void)workspace;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const SpanArgs a{t_codes, t_start, t_len, o_codes, o_off, params, params_stride, out, nprob};
    const int nstrips = (max_m > 0) ? PtrLayout<kSpanR>::nstrips(max_n) : 0;
    const hipError_t e = nstrips >= 8 ? launch_span<8>(a, max_m, st)
                         : nstrips >= 4 ? launch_span<4>(a, max_m, st)
                         : nstrips >= 2 ? launch_span<2>(a, max_m, st)
                                        : launch_span<1>(a, max_m, st);
    if (e != hipSuccess) return ta_fail_hip(e, "nw_span_kernel launch");
    return TA_OK;
}

extern "C" int64_t ta_nw_span_chain_workspace_bytes(int32_t nchains, int32_t npages, int32_t max_n) {
    if (nchains < 0 || npages < 0 || max_n < 0 || max_n > kSpanMaxN) return TA_EINVAL;
    return SpanChainLayout(nchains, npages, max_n).total;
}

extern "C" int ta_nw_span_chain(const int32_t* t_codes, const int64_t* t_start, const int32_t* t_len,
                                const int32_t* o_codes, const int64_t* o_off, const int32_t* page_first,
                                int32_t nchains, int32_t npages, const int32_t* host_pages,
                                const int32_t* params, int32_t params_stride, int32_t floor,
                                int32_t* out, int64_t* total,
                                int32_t max_n, int32_t max_m, int64_t score_bound, int32_t max_param,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    if (nchains < 0 || npages < 0 || max_n < 0 || max_m < 0 || workspace_bytes < 0)
        return ta_fail(TA_EINVAL, "negative size");
    if (nchains == 0) return npages == 0 ? TA_OK : ta_fail(TA_EINVAL, "pages without a chain");
    if (!t_start || !t_len || !o_off || !page_first || !host_pages || !params || !total || (npages > 0 && !out))
        return ta_fail(TA_EINVAL, "null pointer argument");
    if (params_stride != 0 && params_stride != 6) return ta_fail(TA_EINVAL, "params_stride must be 0 or 6");
    if (max_m > kSpanMaxM) return ta_fail(TA_EINVAL, "m exceeds the LDS hand-off row of the span fill");
    if (max_n > kSpanMaxN) return ta_fail(TA_EINVAL, "n exceeds the origin field of the span fill (2^28 - 1)");
    if (floor <= 0) return ta_fail(TA_EINVAL, "the carry's floor must be positive");
    if (score_bound < 0 || score_bound + floor >= (1ll << 23))
        return ta_fail(TA_ERANGE, "(n+m+2)*max|param| + floor does not fit the 24-bit score field");
    if (max_param < 0 || max_param > kSpanMaxParam)
        return ta_fail(TA_ERANGE, "scoring parameters too large for the span fill (2^19)");
    if (max_n > 0 && max_m > 0 && (!t_codes || !o_codes)) return ta_fail(TA_EINVAL, "null code pointer");
    int64_t sum = 0;
    int32_t steps = 0;
    for (int32_t c = 0; c < nchains; ++c) {
        if (host_pages[c] < 0) return ta_fail(TA_EINVAL, "negative page count");
        sum += host_pages[c];
        steps = host_pages[c] > steps ? host_pages[c] : steps;
    }
    if (sum != npages) return ta_fail(TA_EINVAL, "the chains' page counts do not add up to npages");
    const SpanChainLayout lay(nchains, npages, max_n);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < lay.total)
        return ta_fail(TA_EINVAL, "workspace missing, misaligned or smaller than ta_nw_span_chain_workspace_bytes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    SpanChainArgs a{t_codes, t_start, t_len, o_codes, o_off, page_first, params, params_stride,
                    reinterpret_cast<int32_t*>(ws),
                    reinterpret_cast<int32_t*>(ws + lay.order_bytes),
                    reinterpret_cast<int32_t*>(ws + lay.order_bytes + lay.array_bytes),
                    reinterpret_cast<int32_t*>(ws + lay.order_bytes + 2 * lay.array_bytes),
                    lay.stride, out, total, nchains, npages, max_n, max_m, floor, 0};
    hipLaunchKernelGGL(nw_span_chain_order_kernel, dim3((nchains + kChainThreads - 1) / kChainThreads),
                       dim3(kChainThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "nw_span_chain_order_kernel launch");
    const int nstrips = (max_m > 0) ? PtrLayout<kSpanR>::nstrips(max_n) : 0;
    for (int32_t s = 0; s < steps; ++s) {
        int32_t count = 0;                     // the chains that have a page s: the first `count` of the ranking
        for (int32_t c = 0; c < nchains; ++c) count += host_pages[c] > s ? 1 : 0;
        a.step = s;
        e = nstrips >= 8 ? launch_span_chain<8>(a, count, st)
            : nstrips >= 4 ? launch_span_chain<4>(a, count, st)
            : nstrips >= 2 ? launch_span_chain<2>(a, count, st)
                           : launch_span_chain<1>(a, count, st);
        if (e != hipSuccess) return ta_fail_hip(e, "nw_span_chain_kernel launch");
        hipLaunchKernelGGL(nw_span_carry_kernel, dim3(count), dim3(kChainThreads), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return ta_fail_hip(e, "nw_span_carry_kernel launch");
    }
    hipLaunchKernelGGL(nw_span_walk_kernel, dim3(nchains), dim3(kChainThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "nw_span_walk_kernel launch");
    return TA_OK;
}
