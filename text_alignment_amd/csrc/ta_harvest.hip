// ta_harvest.hip -- harvesting of line-level training texts from aligned pages: from the
// alignment columns of a ta_nw_batch / ta_nw2_batch call, where they lie, per text line the piece of the page's
// transcript that the line's OCR characters were aligned with, counts that say how far to trust it and an accept /
// reject decision; then the accepted lines packed into the layout ta_ctc_align reads.  Integers only; the checker of
// record is tests/harvest_ref.py.
//
// harvest_lines_kernel, one wave per page, three stages:
//   check    the page's own device numbers (offsets, ops_len, the line range) and its o_line (never decreasing, inside
//            the page's lines); a page that fails is refused: bit PAGE on all of its lines, a status word
//   columns  the alignment columns in chunks of 64, a lane per column: the column's (i, j) is the running count of the
//            chunks before plus the popcount of the ballot masks below the lane.  Every OCR character gets the number of
//            transcript characters in front of its column and what its column is (gap / equal pair / unequal pair),
//            every transcript character whether it stands in an equal pair -- byte and int arrays in the workspace.
//            The columns must carry exactly n transcript and m OCR characters, or the page is refused
//   lines    the page's lines in order, wave-uniform.  o_line never decreases, so a line's OCR characters are one run
//            jlo .. jhi and its transcript characters -- pairs and the op-1 columns between its first and last OCR
//            column -- the run ta .. tb read off the two ends; the counts are ballots over the run, the trim and the
//            codec test one pass over ta .. tb, a seam the characters between one line's tb and the next one's ta.
//            A line's row is held back until the seam behind it is known.
// No atomics: every number has one writer, the result does not depend on any order.
// harvest_pack_kernel, a wave per 64 lines: the wave sums the accepted lines in front of its chunk itself (no hand-over
// between workgroups), places its own and copies their t_class ranges; the last one writes the totals.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kF = TA_HARVEST_FIELDS;

// the workspace: t_abs first (ta_harvest_pack reads it knowing nlines alone), every piece 16-byte aligned
struct HarvestWs {
    int64_t t_abs, o_ti, o_flag, t_flag, bytes;
};
__host__ __device__ inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline HarvestWs harvest_ws(int64_t nlines, int64_t t_len, int64_t o_len) {
    HarvestWs w;
    w.t_abs = 0;
    w.o_ti = w.t_abs + up16(8 * nlines);
    w.o_flag = w.o_ti + up16(4 * o_len);
    w.t_flag = w.o_flag + up16(o_len);
    w.bytes = w.t_flag + up16(t_len) + 16;
    return w;
}

struct HarvestArgs {
    const uint8_t* ops; const int64_t* ops_off; const int32_t* ops_len; int64_t ops_bytes;
    const int32_t* t_codes; const int64_t* t_off; const int32_t* o_codes; const int64_t* o_off;
    int64_t t_len, o_len;
    const int32_t* o_line; const int64_t* line_first; const int32_t* t_class; const int32_t* T;
    int32_t nlines, num, den;
    int64_t* t_abs; int32_t* o_ti; uint8_t* o_flag; uint8_t* t_flag;      // the workspace's pieces
    int32_t* table; int32_t* status;
};

struct Row {
    int line, reason, t_first, L, eq, ne, in1, g2, seam;
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int popc(unsigned long long m) { return __builtin_popcountll(m); }

// how many of cls[a .. b) are no space (class 1); wave-uniform
__device__ __forceinline__ int count_glyphs(const int32_t* cls, int a, int b, int lane) {
    int s = 0;
    for (int base = a; base < b; base += 64) {
        const int i = base + lane;
        s += popc(__ballot(i < b && cls[i] != 1));
    }
    return s;
}

__device__ __forceinline__ void emit(const HarvestArgs& a, const Row& r, int64_t t0, int lane) {
    if (lane == 0) {
        int32_t* out = a.table + (int64_t)kF * r.line;
        out[0] = r.reason | (r.seam > 0 ? TA_HARVEST_SEAM : 0);
        out[1] = r.t_first; out[2] = r.L; out[3] = r.eq; out[4] = r.ne; out[5] = r.in1; out[6] = r.g2; out[7] = r.seam;
        a.t_abs[r.line] = t0 + r.t_first;
    }
}

__global__ __launch_bounds__(64) void harvest_lines_kernel(HarvestArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t t0 = a.t_off[p], t1 = a.t_off[p + 1], o0 = a.o_off[p], o1 = a.o_off[p + 1], r0 = a.ops_off[p];
    const int64_t lf0 = a.line_first[p], lf1 = a.line_first[p + 1];
    const int len = uni(a.ops_len[p]);
    // the page's line range first: without it there is no row to write a refusal into
    if (!(lf0 >= 0 && lf0 <= lf1 && lf1 <= a.nlines)) {
        if (lane == 0) a.status[p] = TA_HARVEST_LINES;
        return;
    }
    // ---- check: every bound the kernel relies on, on the page's own numbers (the host checked its copies as well) ----
    int st = TA_HARVEST_OK, n = 0, m = 0;
    if (!(t0 >= 0 && t1 >= t0 && t1 <= a.t_len && o0 >= 0 && o1 >= o0 && o1 <= a.o_len &&
          t1 - t0 <= TA_HARVEST_MAX_COLUMNS && o1 - o0 <= TA_HARVEST_MAX_COLUMNS)) st = TA_HARVEST_MISMATCH;
    else {
        n = (int)(t1 - t0);
        m = (int)(o1 - o0);
        if (len < 0) st = TA_HARVEST_UNFINISHED;
        else if (len > n + m || r0 < 0 || r0 + n + m > a.ops_bytes) st = TA_HARVEST_MISMATCH;
    }
    st = uni(st); n = uni(n); m = uni(m);
    const int32_t* ol = a.o_line + o0;
    if (st == TA_HARVEST_OK) {
        bool bad = false;
        for (int base = 0; base < m; base += 64) {
            const int j = base + lane;
            if (j < m) {
                const int64_t l = ol[j], prev = j ? (int64_t)ol[j - 1] : lf0;
                bad |= l < lf0 || l >= lf1 || l < prev;
            }
        }
        if (__any(bad)) st = TA_HARVEST_LINES;
    }

    // ---- columns ----------------------------------------------------------------------------------------------------
    if (st == TA_HARVEST_OK) {
        const uint8_t* col = a.ops + r0 + (n + m - len);              // right-aligned in the problem's region
        const int32_t* tc = a.t_codes + t0;
        const int32_t* oc = a.o_codes + o0;
        int ti = 0, oj = 0;
        bool bad = false;
        for (int base = 0; base < len; base += 64) {
            const int c = base + lane;
            const int op = c < len ? (int)col[c] : 3;
            bad |= c < len && op > 2;
            const bool ht = op == 0 || op == 1, ho = op == 0 || op == 2;
            const unsigned long long tm = __ballot(ht), om = __ballot(ho);
            const int i = ti + popc(tm & below), j = oj + popc(om & below);
            const bool it = ht && i < n, jo = ho && j < m;           // beyond n or m: nothing is touched, the counts refuse the page
            bool eq = false;
            if (op == 0 && it && jo) eq = tc[i] == oc[j];
            if (it) a.t_flag[t0 + i] = eq;
            if (jo) {
                a.o_ti[o0 + j] = i;
                a.o_flag[o0 + j] = op == 2 ? 0 : (eq ? 1 : 2);
            }
            ti += popc(tm);
            oj += popc(om);
        }
        if (__any(bad) || ti != n || oj != m) st = TA_HARVEST_MISMATCH;
    }
    if (st != TA_HARVEST_OK) {
        for (int64_t k = lf0 * kF + lane; k < lf1 * kF; k += 64) a.table[k] = k % kF == 0 ? TA_HARVEST_PAGE : 0;
        for (int64_t l = lf0 + lane; l < lf1; l += 64) a.t_abs[l] = 0;
        if (lane == 0) a.status[p] = st;
        return;
    }
    __threadfence();                                    // the per-character arrays are read back below, by other lanes
    __syncthreads();

    // ---- lines ------------------------------------------------------------------------------------------------------
    const int32_t* cls = a.t_class + t0;
    const uint8_t* of = a.o_flag + o0;
    Row pend = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool have = false;
    int prev_tb = 0, jcur = 0;
    for (int l = (int)lf0; l < (int)lf1; ++l) {
        Row row = {l, 0, 0, 0, 0, 0, 0, 0, 0};
        const int jlo = jcur;
        for (;;) {                                      // the line's OCR characters: a run, o_line never decreases
            const int j = jcur + lane;
            const bool mine = j < m && ol[j] == l;
            const int f = mine ? (int)of[j] : 3;
            const int k = popc(__ballot(mine));
            row.eq += popc(__ballot(f == 1));
            row.ne += popc(__ballot(f == 2));
            row.g2 += popc(__ballot(f == 0));
            jcur += k;
            if (k < 64) break;
        }
        const int Tl = uni(a.T[l]);
        int ta = 0, tb = 0, first = -1, last = -1;
        bool codec = false;
        if (jcur > jlo) {
            ta = uni(a.o_ti[o0 + jlo]);
            tb = uni(a.o_ti[o0 + jcur - 1] + (of[jcur - 1] != 0));
            row.in1 = tb - ta - (row.eq + row.ne);
            for (int base = ta; base < tb; base += 64) {           // trim the spaces at both ends; a class below 1 is no space
                const int i = base + lane;
                const int c = i < tb ? cls[i] : 1;
                const unsigned long long ns = __ballot(c != 1);
                codec |= __ballot(c < 1) != 0ull;
                if (ns) {
                    if (first < 0) first = base + __builtin_ctzll(ns);
                    last = base + 63 - __builtin_clzll(ns);
                }
            }
        }
        if (first < 0) row.reason |= TA_HARVEST_EMPTY;
        else {
            row.t_first = first;
            row.L = last - first + 1;
            if (!(a.t_flag[t0 + first] && a.t_flag[t0 + last])) row.reason |= TA_HARVEST_UNANCHORED;
        }
        const long long total = (long long)row.eq + row.ne + row.in1 + row.g2;
        if (total == 0 || (long long)row.eq * a.den < (long long)a.num * total) row.reason |= TA_HARVEST_LOW;
        if (codec) row.reason |= TA_HARVEST_CODEC;
        if (2 * row.L + 1 > Tl || row.L > TA_HARVEST_MAX_TARGET) row.reason |= TA_HARVEST_TOO_LONG;
        if (jcur > jlo) {                               // the seam in front borders this line and the last one with characters
            row.seam = count_glyphs(cls, prev_tb, ta, lane);
            if (have) {
                pend.seam += row.seam;
                emit(a, pend, t0, lane);
            }
            pend = row;
            have = true;
            prev_tb = tb;
        } else {
            emit(a, row, t0, lane);                     // no OCR character: borders nothing
        }
    }
    if (have) {
        pend.seam += count_glyphs(cls, prev_tb, n, lane);
        emit(a, pend, t0, lane);
    }
    if (lane == 0) a.status[p] = TA_HARVEST_OK;
}

struct PackArgs {
    const int32_t* table; const int64_t* t_abs; const int32_t* t_class; int64_t t_len;
    int32_t nlines, nblocks; int64_t cap;
    int32_t* acc_line; int32_t* L; int64_t* lab_off; int32_t* labels; int64_t* count;
};

__global__ __launch_bounds__(64) void harvest_pack_kernel(PackArgs a) {
    __shared__ long long s_sum[64];
    __shared__ int s_cnt[64], s_len[64];
    __shared__ long long s_src[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int base = 64 * b;
    // ---- the accepted lines in front of this chunk, every row re-checked -----------------------------------------
    long long sum = 0;
    int cnt = 0;
    bool bad = false;
    for (int l = lane; l < base; l += 64)
        if (a.table[(int64_t)kF * l] == 0) {
            const int len = a.table[(int64_t)kF * l + 2];
            bad |= len < 1 || len > TA_HARVEST_MAX_TARGET;
            sum += len;
            ++cnt;
        }
    // ---- this chunk's lines ----------------------------------------------------------------------------------------
    const int l = base + lane;
    int len = 0;
    long long src = 0;
    bool acc = false;
    if (l < a.nlines && a.table[(int64_t)kF * l] == 0) {
        acc = true;
        len = a.table[(int64_t)kF * l + 2];
        src = a.t_abs[l];
        if (len < 1 || len > TA_HARVEST_MAX_TARGET || src < 0 || src + len > a.t_len) { bad = true; len = 0; }
    }
    s_sum[lane] = sum; s_cnt[lane] = cnt; s_len[lane] = len; s_src[lane] = src;
    __syncthreads();
    long long before = 0, excl = 0;
    int nbefore = 0, tot = 0;
    for (int q = 0; q < 64; ++q) {
        before += s_sum[q];
        nbefore += s_cnt[q];
        if (q < lane) excl += s_len[q];
        tot += s_len[q];
    }
    const unsigned long long am = __ballot(acc);
    const bool broken = __any(bad) || before + tot > a.cap;
    if (!broken) {
        if (acc) {
            const int k = nbefore + popc(am & ((1ull << lane) - 1ull));
            a.acc_line[k] = l;
            a.L[k] = len;
            a.lab_off[k] = before + excl;
        }
        long long dst = before;
        for (unsigned long long rest = am; rest; rest &= rest - 1ull) {
            const int q = __builtin_ctzll(rest);
            const int lq = s_len[q];
            const long long sq = s_src[q];
            for (int i = lane; i < lq; i += 64) a.labels[dst + i] = a.t_class[sq + i];
            dst += lq;
        }
    }
    if (b == a.nblocks - 1 && lane == 0) {              // the last chunk has seen every row
        a.count[0] = broken ? -1 : nbefore + popc(am);
        a.count[1] = broken ? -1 : before + tot;
    }
}

}  // namespace

extern "C" int64_t ta_harvest_workspace_bytes(int32_t nlines, int64_t t_len, int64_t o_len) {
    if (nlines < 0 || t_len < 0 || o_len < 0) return TA_EINVAL;
    if (nlines > TA_HARVEST_MAX_LINES || t_len > ((int64_t)1 << 40) || o_len > ((int64_t)1 << 40)) return TA_ELIMIT;
    return harvest_ws(nlines, t_len, o_len).bytes;
}

extern "C" int ta_harvest_lines(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len, int64_t ops_bytes,
                                const int32_t* t_codes, const int64_t* t_off, const int32_t* o_codes,
                                const int64_t* o_off, int32_t nprob, const int32_t* o_line, const int64_t* line_first,
                                const int32_t* t_class, const int32_t* T, int32_t nlines, int32_t num, int32_t den,
                                const int64_t* t_off_host, const int64_t* o_off_host, const int64_t* line_first_host,
                                void* workspace, int64_t workspace_bytes, int32_t* table, int32_t* status, void* stream) {
    if (nprob < 0 || nlines < 0 || ops_bytes < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative size");
    if (num < 1 || den < 1 || num > den || den > TA_HARVEST_MAX_DEN)
        return ta_fail(TA_EINVAL, "minimum agreement: 0 < num <= den <= TA_HARVEST_MAX_DEN");
    if (nlines > TA_HARVEST_MAX_LINES) return ta_fail(TA_ELIMIT, "more than TA_HARVEST_MAX_LINES lines");
    if (nprob == 0) return nlines == 0 ? TA_OK : ta_fail(TA_EINVAL, "lines without a page");
    if (!ops || !ops_off || !ops_len || !t_codes || !t_off || !o_codes || !o_off || !o_line || !line_first ||
        !t_class || !T || !t_off_host || !o_off_host || !line_first_host || !workspace || !table || !status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return ta_fail(TA_EINVAL, "workspace not 16-byte aligned");
    if (t_off_host[0] < 0 || o_off_host[0] < 0 || line_first_host[0] != 0 || line_first_host[nprob] != nlines)
        return ta_fail(TA_EINVAL, "offsets must start at or above 0, line_first run from 0 to nlines");
    for (int p = 0; p < nprob; ++p) {
        const int64_t n = t_off_host[p + 1] - t_off_host[p], m = o_off_host[p + 1] - o_off_host[p];
        if (n < 0 || m < 0 || line_first_host[p + 1] < line_first_host[p])
            return ta_fail(TA_EINVAL, "t_off, o_off and line_first must not decrease");
        if (n > TA_HARVEST_MAX_COLUMNS || m > TA_HARVEST_MAX_COLUMNS)
            return ta_fail(TA_ELIMIT, "a page exceeds TA_HARVEST_MAX_COLUMNS");
    }
    const int64_t t_len = t_off_host[nprob], o_len = o_off_host[nprob];
    const int64_t need = ta_harvest_workspace_bytes(nlines, t_len, o_len);
    if (need == TA_ELIMIT) return ta_fail(TA_ELIMIT, "batch too large for the harvest workspace");
    if (workspace_bytes < need) return ta_fail(TA_EINVAL, "workspace smaller than ta_harvest_workspace_bytes");
    const HarvestWs w = harvest_ws(nlines, t_len, o_len);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    HarvestArgs a{ops, ops_off, ops_len, ops_bytes, t_codes, t_off, o_codes, o_off, t_len, o_len, o_line, line_first,
                  t_class, T, nlines, num, den, reinterpret_cast<int64_t*>(ws + w.t_abs),
                  reinterpret_cast<int32_t*>(ws + w.o_ti), ws + w.o_flag, ws + w.t_flag, table, status};
    hipLaunchKernelGGL(harvest_lines_kernel, dim3((unsigned)nprob), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "harvest_lines_kernel launch");
    return TA_OK;
}

extern "C" int ta_harvest_pack(const int32_t* table, const void* workspace, int64_t workspace_bytes,
                               const int32_t* t_class, int64_t t_len, int32_t nlines, int64_t label_cap,
                               int32_t* acc_line, int32_t* L, int64_t* lab_off, int32_t* labels, int64_t* count,
                               void* stream) {
    if (nlines < 0 || t_len < 0 || label_cap < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative size");
    if (nlines > TA_HARVEST_MAX_LINES) return ta_fail(TA_ELIMIT, "more than TA_HARVEST_MAX_LINES lines");
    if (!table || !workspace || !t_class || !acc_line || !L || !lab_off || !labels || !count)
        return ta_fail(TA_EINVAL, "null pointer argument");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return ta_fail(TA_EINVAL, "workspace not 16-byte aligned");
    if (workspace_bytes < up16(8 * (int64_t)nlines)) return ta_fail(TA_EINVAL, "workspace smaller than the lines' offsets");
    const int nblocks = nlines ? (nlines + 63) / 64 : 1;
    PackArgs a{table, static_cast<const int64_t*>(workspace), t_class, t_len, nlines, nblocks, label_cap,
               acc_line, L, lab_off, labels, count};
    hipLaunchKernelGGL(harvest_pack_kernel, dim3((unsigned)nblocks), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "harvest_pack_kernel launch");
    return TA_OK;
}
