// ta_refine.hip -- the refined lines' column runs replaced on the device ("Realisation on the
// device"): the rule of forced.refine_columns as a kernel, behind ta_harvest_lines / ta_harvest_pack / ta_forced_align_lines
// on the same stream, so that a chunk's refinement needs no look at the harvest table from the host.  Integers only; the
// checker of record is tests/refine_ref.py.
//
// A line is refined iff its reason is 0, it has a packed slot k (acc_line[k] == line, k < count[0]), the forced alignment
// gave that slot TA_FORCED_OK, L[k] <= TA_FORCED_MAX_TARGET and its page is plain.  A refined line owns the columns from
// its first to its last OCR-carrying column; in the new columns every transcript character of that run keeps ONE column --
// a pair (op 0) with a new box row if it is one of the kept characters t_first .. + L, an op-1 column otherwise -- and the
// run's op-2 columns are gone.  So the new columns are the old ones with some codes changed and some columns dropped: one
// stream compaction, the generated pairs fall into place by themselves.
//
// refine_columns_kernel, one wave per page:
//   check    the page's own device numbers; the harvest's verdict; o_line never decreasing inside the page's lines
//   lines    a lane per line: the predicate above, the slot by binary search in acc_line (ta_harvest_pack leaves it
//            ascending), the packed row held against the table's; refined[] and slot[] are written here
//   columns  in tiles of 64, a lane per column (byte loads next to each other).  The exclusive counts of "carries a
//            transcript character", "carries an OCR character", "is kept" and "is kept and carries an OCR character" are
//            ballots: popcount of the mask below the lane plus the running total of the tiles before, all in registers --
//            a wave needs no hand-over through LDS for them.  A column's line is its OCR character's, or for an op-1
//            column the line of both OCR characters around it if they agree.  The first and the last OCR column of a
//            refined line hold the line's kept range against the run's transcript range ta .. tb.
// The outputs are buffers of their own, left-aligned in the page's region.  A page that fails a check gets a status and
// its columns copied through unchanged (second pass, behind a barrier), none of its lines refined.  No atomics.
//
// kOmit (ta_refine_columns_omit; the checker of record is tests/refine_omit_ref.py): the slots come
// from ta_forced_align_omit_lines, whose path may leave characters out.  Character i of slot k is PRESENT iff
// frames[3 (lab_off[k] + i)] >= 0.  In `lines` the wave counts the present characters of every line of the tile that has
// a filled slot with TA_FORCED_OK, L <= TA_FORCED_MAX_TARGET and its rows inside `frames` -- the slots of a tile go through
// 64 words of LDS, then for one slot after the other the L rows are taken in strides of 64, a ballot and a popcount each --
// and writes omitted[] beside refined[] and slot[]; a line of the strict predicate without a present character is not
// refined.  In `columns` a kept character of a refined run that is not present becomes an op-1 column; the rows of the
// present ones keep the strict numbering.  The kOmit = false instantiation is the kernel as it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kF = TA_HARVEST_FIELDS;

struct RefineArgs {
    const uint8_t* ops; const int64_t* ops_off; const int32_t* ops_len; int64_t ops_bytes;
    const int64_t* t_off; const int64_t* o_off; int64_t t_len, o_len;
    const int32_t* o_line; const int64_t* line_first; const int32_t* idx;
    const int32_t* table; const int32_t* h_status; int32_t nlines;
    const int32_t* acc_line; const int32_t* L; const int64_t* lab_off; const int64_t* count; int32_t nslots; int64_t label_cap;
    const int32_t* f_status; const uint8_t* plain; int32_t box_base;
    uint8_t* ops_new; int32_t* ops_new_len; int32_t* idx_new; int32_t* idx_new_len; int32_t* refined; int32_t* slot;
    int32_t* status;
    const int32_t* frames; int32_t* omitted;              // ta_refine_columns_omit alone
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int popc(unsigned long long m) { return __builtin_popcountll(m); }

template <bool kOmit>
__global__ __launch_bounds__(64) void refine_columns_kernel(RefineArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t t0 = a.t_off[p], t1 = a.t_off[p + 1], o0 = a.o_off[p], o1 = a.o_off[p + 1], r0 = a.ops_off[p];
    const int64_t lf0 = a.line_first[p], lf1 = a.line_first[p + 1];
    const int len = uni(a.ops_len[p]);
    // ---- check: every bound the kernel relies on, on the page's own numbers ---------------------------------------------
    const bool inside = lf0 >= 0 && lf0 <= lf1 && lf1 <= a.nlines && t0 >= 0 && t1 >= t0 && t1 <= a.t_len && o0 >= 0 &&
                        o1 >= o0 && o1 <= a.o_len && t1 - t0 <= TA_HARVEST_MAX_COLUMNS && o1 - o0 <= TA_HARVEST_MAX_COLUMNS &&
                        len >= 0 && len <= (t1 - t0) + (o1 - o0) && r0 >= 0 && r0 + (t1 - t0) + (o1 - o0) <= a.ops_bytes;
    if (!inside) {                                      // nothing can be copied: the lengths say so
        if (lane == 0) {
            a.ops_new_len[p] = -1;
            a.idx_new_len[p] = -1;
            a.status[p] = TA_REFINE_BOUNDS;
        }
        return;
    }
    const int n = uni((int)(t1 - t0)), m = uni((int)(o1 - o0));
    const uint8_t* col = a.ops + r0 + (n + m - len);    // right-aligned in the page's region
    const int32_t* ol = a.o_line + o0;
    int st = uni(a.h_status[p]) != TA_HARVEST_OK ? TA_REFINE_HARVEST : TA_REFINE_OK;
    if (st == TA_REFINE_OK) {
        bool bad = false;
        for (int base = 0; base < m; base += 64) {
            const int j = base + lane;
            if (j < m) {
                const int64_t l = ol[j], prev = j ? (int64_t)ol[j - 1] : lf0;
                bad |= l < lf0 || l >= lf1 || l < prev;
            }
        }
        if (__any(bad)) st = TA_REFINE_COLUMNS;
    }

    // ---- lines: which are refined, and their slots -----------------------------------------------------------------------
    int64_t filled = a.count[0];
    filled = filled < 0 ? 0 : filled > a.nslots ? a.nslots : filled;
    const bool plain = a.plain[p] != 0;
    int nref = 0;
    bool tbad = false;
    for (int64_t base = lf0; base < lf1; base += 64) {
        const int64_t q = base + lane;
        int r = 0, k = -1, kc = -1;                       // kc: the slot whose present characters are counted
        if (q < lf1 && st == TA_REFINE_OK && (kOmit || (plain && a.table[kF * q] == 0))) {
            int lo = 0, hi = (int)filled;
            while (lo < hi) {                           // the first slot whose line is not below q
                const int mid = (lo + hi) >> 1;
                if (a.acc_line[mid] < q) lo = mid + 1;
                else hi = mid;
            }
            if (lo < (int)filled && a.acc_line[lo] == q) {
                const int Lk = a.L[lo];
                if (a.f_status[lo] == TA_FORCED_OK && Lk <= TA_FORCED_MAX_TARGET) {
                    const int64_t l0 = a.lab_off[lo];
                    if (kOmit && Lk >= 1 && l0 >= 0 && l0 + Lk <= a.label_cap) kc = lo;
                    if (!kOmit || (plain && a.table[kF * q] == 0)) {
                        r = 1;
                        k = lo;
                        const int tf = a.table[kF * q + 1];
                        tbad |= Lk < 1 || Lk != a.table[kF * q + 2] || l0 < 0 || l0 + Lk > a.label_cap || tf < 0 || tf + Lk > n;
                    }
                }
            }
        }
        if (kOmit) {                                    // the tile's slots through LDS, their rows wave-wide
            __shared__ int tile_slot[64];
            tile_slot[lane] = kc;
            __syncthreads();
            int gone = -1;
            for (unsigned long long todo = __ballot(kc >= 0); todo; todo &= todo - 1) {
                const int src = __builtin_ctzll(todo), ks = tile_slot[src];
                const int Ls = a.L[ks];
                const int32_t* fr = a.frames + 3 * a.lab_off[ks];
                int present = 0;
                for (int i0 = 0; i0 < Ls; i0 += 64) present += popc(__ballot(i0 + lane < Ls && fr[3 * (i0 + lane)] >= 0));
                if (lane == src) gone = Ls - present;
            }
            __syncthreads();                            // the next tile writes tile_slot again
            if (r && gone == a.L[k]) {                  // no character on the path: not refined, its run stays
                r = 0;
                k = -1;
            }
            if (q < lf1) a.omitted[q] = gone;
        }
        if (q < lf1) {
            a.refined[q] = r;
            a.slot[q] = k;
        }
        nref += popc(__ballot(r));
    }
    if (__any(tbad)) st = TA_REFINE_CONTAIN;
    __threadfence();                                    // refined and slot are read back below, by other lanes
    __syncthreads();

    // ---- columns ------------------------------------------------------------------------------------------------------
    if (st == TA_REFINE_OK) {
        int ti = 0, oj = 0, cn = 0, jn = 0, nfirst = 0;
        bool bad = false, cbad = false;
        for (int base = 0; base < len; base += 64) {
            const int c = base + lane;
            const int op = c < len ? (int)col[c] : 3;
            bad |= c < len && op > 2;
            const bool ht = op == 0 || op == 1, ho = op == 0 || op == 2;
            const unsigned long long tm = __ballot(ht), om = __ballot(ho);
            const int i = ti + popc(tm & below), j = oj + popc(om & below);
            int q = -1;
            bool first = false, last = false;
            if (ho && j < m) {
                q = ol[j];
                first = j == 0 || ol[j - 1] != q;
                last = j == m - 1 || ol[j + 1] != q;
            } else if (op == 1 && j >= 1 && j < m) {   // between two OCR characters: inside a run if they share a line
                const int qa = ol[j - 1];
                if (qa == ol[j]) q = qa;
            }
            const bool run = nref > 0 && q >= 0 && a.refined[q] != 0;
            int tf = 0, Lq = 0;
            int64_t row = 0;
            if (run) {
                tf = a.table[kF * (int64_t)q + 1];
                Lq = a.table[kF * (int64_t)q + 2];
                row = (int64_t)a.box_base + a.lab_off[a.slot[q]] - tf;
            }
            const bool keep = c < len && !(run && op == 2);
            bool kept = run && ht && i >= tf && i < tf + Lq;
            if (kOmit && kept) kept = a.frames[3 * (row + i - a.box_base)] >= 0;
            const int nop = run && ht ? (kept ? 0 : 1) : op;
            const bool carries = keep && nop != 1;
            if (run && ho) {                            // the kept characters inside ta .. tb of the run
                if (first) cbad |= i > tf;
                if (last) cbad |= tf + Lq > i + (ht ? 1 : 0);
            }
            nfirst += popc(__ballot(run && ho && first));
            const unsigned long long km = __ballot(keep), nm = __ballot(carries);
            if (keep) a.ops_new[r0 + cn + popc(km & below)] = (uint8_t)nop;
            if (carries) a.idx_new[r0 + jn + popc(nm & below)] = run ? (int32_t)(row + i) : (j < m ? a.idx[o0 + j] : 0);
            ti += popc(tm);
            oj += popc(om);
            cn += popc(km);
            jn += popc(nm);
        }
        if (__any(bad) || ti != n || oj != m) st = TA_REFINE_COLUMNS;
        else if (__any(cbad) || nfirst != nref) st = TA_REFINE_CONTAIN;
        if (st == TA_REFINE_OK) {
            if (lane == 0) {
                a.ops_new_len[p] = cn;
                a.idx_new_len[p] = jn;
                a.status[p] = TA_REFINE_OK;
            }
            return;
        }
        __threadfence();                                // the copy below overwrites what other lanes wrote above
        __syncthreads();
    }

    // ---- a page that was refused: its columns and rows as they are, none of its lines refined ---------------------------
    for (int c = lane; c < len; c += 64) a.ops_new[r0 + c] = col[c];
    for (int j = lane; j < m; j += 64) a.idx_new[r0 + j] = a.idx[o0 + j];
    for (int64_t q = lf0 + lane; q < lf1; q += 64) {
        a.refined[q] = 0;
        a.slot[q] = -1;
        if (kOmit) a.omitted[q] = -1;
    }
    if (lane == 0) {
        a.ops_new_len[p] = len;
        a.idx_new_len[p] = m;
        a.status[p] = st;
    }
}

// what both entries refuse, then the launch
template <bool kOmit>
int refine_columns(const RefineArgs& a, int32_t nprob, bool null, void* stream) {
    if (nprob < 0 || a.nlines < 0 || a.nslots < 0 || a.ops_bytes < 0 || a.t_len < 0 || a.o_len < 0 || a.label_cap < 0 ||
        a.box_base < 0)
        return ta_fail(TA_EINVAL, "negative size");
    if (a.nlines > TA_HARVEST_MAX_LINES) return ta_fail(TA_ELIMIT, "more than TA_HARVEST_MAX_LINES lines");
    if ((int64_t)a.box_base + a.label_cap > INT32_MAX) return ta_fail(TA_ELIMIT, "box rows beyond 32 bits");
    if (nprob == 0) return TA_OK;
    if (null) return ta_fail(TA_EINVAL, "null pointer argument");
    hipLaunchKernelGGL(refine_columns_kernel<kOmit>, dim3((unsigned)nprob), dim3(64), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, kOmit ? "refine_columns_kernel launch (omit)" : "refine_columns_kernel launch");
    return TA_OK;
}

}  // namespace

extern "C" int ta_refine_columns(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                                 const int64_t* t_off, const int64_t* o_off, int64_t t_len, int64_t o_len, int32_t nprob,
                                 const int32_t* o_line, const int64_t* line_first, const int32_t* idx,
                                 const int32_t* table, const int32_t* harvest_status, int32_t nlines,
                                 const int32_t* acc_line, const int32_t* L, const int64_t* lab_off, const int64_t* count,
                                 int32_t nslots, int64_t label_cap, const int32_t* forced_status, const uint8_t* plain,
                                 int32_t box_base, uint8_t* ops_new, int32_t* ops_new_len, int32_t* idx_new,
                                 int32_t* idx_new_len, int32_t* refined, int32_t* slot, int32_t* status, void* stream) {
    const bool null = !ops || !ops_off || !ops_len || !t_off || !o_off || !o_line || !line_first || !idx || !table ||
                      !harvest_status || !acc_line || !L || !lab_off || !count || !forced_status || !plain || !ops_new ||
                      !ops_new_len || !idx_new || !idx_new_len || !refined || !slot || !status;
    const RefineArgs a{ops, ops_off, ops_len, ops_bytes, t_off, o_off, t_len, o_len, o_line, line_first, idx, table,
                       harvest_status, nlines, acc_line, L, lab_off, count, nslots, label_cap, forced_status, plain, box_base,
                       ops_new, ops_new_len, idx_new, idx_new_len, refined, slot, status, nullptr, nullptr};
    return refine_columns<false>(a, nprob, null, stream);
}

extern "C" int ta_refine_columns_omit(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                                      const int64_t* t_off, const int64_t* o_off, int64_t t_len, int64_t o_len,
                                      int32_t nprob, const int32_t* o_line, const int64_t* line_first, const int32_t* idx,
                                      const int32_t* table, const int32_t* harvest_status, int32_t nlines,
                                      const int32_t* acc_line, const int32_t* L, const int64_t* lab_off,
                                      const int64_t* count, int32_t nslots, int64_t label_cap,
                                      const int32_t* forced_status, const int32_t* frames, const uint8_t* plain,
                                      int32_t box_base, uint8_t* ops_new, int32_t* ops_new_len, int32_t* idx_new,
                                      int32_t* idx_new_len, int32_t* refined, int32_t* slot, int32_t* omitted,
                                      int32_t* status, void* stream) {
    const bool null = !ops || !ops_off || !ops_len || !t_off || !o_off || !o_line || !line_first || !idx || !table ||
                      !harvest_status || !acc_line || !L || !lab_off || !count || !forced_status || !frames || !plain ||
                      !ops_new || !ops_new_len || !idx_new || !idx_new_len || !refined || !slot || !omitted || !status;
    const RefineArgs a{ops, ops_off, ops_len, ops_bytes, t_off, o_off, t_len, o_len, o_line, line_first, idx, table,
                       harvest_status, nlines, acc_line, L, lab_off, count, nslots, label_cap, forced_status, plain, box_base,
                       ops_new, ops_new_len, idx_new, idx_new_len, refined, slot, status, frames, omitted};
    return refine_columns<true>(a, nprob, null, stream);
}
