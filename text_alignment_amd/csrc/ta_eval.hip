// ta_eval.hip -- scoring of syllable boxes against ground truth for a whole scoring-system sweep (reference
// evaluate_text_alignment.py:16-131 for every (page, scoring system) of the grid search, :134-198).
//
//   ta_eval_integral        inclusive int32 summed-area tables of a batch of uint8 ink planes (blockIdx.z = page):
//                           row scans, then per 64-row chunk a column scan in place, a carry down the chunks' last
//                           rows, and the carry added to the other rows of each chunk.
//   ta_eval_syllable_boxes  per NW problem, its syllable boxes in raw page coordinates, read from the alignment columns
//                           where the traceback left them (ta_host_syllable_boxes + rotate_boxes of page_batch.py).
//   ta_eval_score           per (problem, counted gt box): first strict maximum of the intersection over the
//                           box's candidates, IOU and black-area IOU (three rectangles x four table lookups).
//
// Compiled with -ffp-contract=off: the rotation reproduces numpy's float64 expression operation by operation.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ta_common.h"

namespace {

constexpr int kEvalPages = 8;       // pages per launch of the summed-area kernels (kernel argument struct)
constexpr int kChunk = 64;          // rows per chunk of the column scan
constexpr int kThreads = 256;

struct SatPages {
    const uint8_t* ink[kEvalPages];
    int32_t* sat[kEvalPages];
    int32_t h[kEvalPages];
    int32_t w[kEvalPages];
};

// inclusive prefix sum over a block of 256 threads (wave64: four waves)
__device__ inline int32_t block_scan(int32_t v, int32_t* lds4, int32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) lds4[wave] = v;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
        const int32_t t = lds4[k];
        before += (k < wave) ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return v + before;
}

// one block per row: the row's inclusive prefix sums of (ink != 0), four bytes per thread per step
__global__ void __launch_bounds__(kThreads) sat_rows_kernel(SatPages P) {
    const int pg = blockIdx.z, y = blockIdx.x;
    if (y >= P.h[pg]) return;
    const int w = P.w[pg];
    const uint8_t* row = P.ink[pg] + (size_t)y * w;
    int32_t* out = P.sat[pg] + (size_t)y * w;
    __shared__ int32_t lds4[kThreads / 64];
    int32_t carry = 0;
    for (int x0 = 0; x0 < w; x0 += 4 * kThreads) {
        const int x = x0 + 4 * threadIdx.x;
        int32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (x + k < w) ? (row[x + k] != 0) : 0;
        v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
        int32_t total;
        const int32_t incl = block_scan(v[3], lds4, &total);
        const int32_t base = carry + incl - v[3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < w) out[x + k] = base + v[k];
        carry += total;
    }
}

// block (column tile, chunk): column prefix sums within the chunk's 64 rows, in place
__global__ void __launch_bounds__(kThreads) sat_chunk_cols_kernel(SatPages P) {
    const int pg = blockIdx.z;
    const int w = P.w[pg], h = P.h[pg];
    const int x = blockIdx.x * kThreads + threadIdx.x, y0 = blockIdx.y * kChunk;
    if (x >= w || y0 >= h) return;
    const int y1 = min(y0 + kChunk, h);
    int32_t* col = P.sat[pg] + x;
    int32_t acc = 0;
    for (int y = y0; y < y1; ++y) {
        acc += col[(size_t)y * w];
        col[(size_t)y * w] = acc;
    }
}

// one thread per column: the last row of every chunk becomes final (adds the last row of the chunk before)
__global__ void __launch_bounds__(kThreads) sat_carry_kernel(SatPages P) {
    const int pg = blockIdx.z;
    const int w = P.w[pg], h = P.h[pg];
    const int x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= w) return;
    int32_t* col = P.sat[pg] + x;
    int32_t prev = col[(size_t)(min(kChunk, h) - 1) * w];
    for (int y0 = kChunk; y0 < h; y0 += kChunk) {
        const size_t last = (size_t)(min(y0 + kChunk, h) - 1) * w;
        prev += col[last];
        col[last] = prev;
    }
}

// block (column tile, chunk >= 1): rows of the chunk except its last get the final last row of the chunk before
__global__ void __launch_bounds__(kThreads) sat_add_kernel(SatPages P) {
    const int pg = blockIdx.z;
    const int w = P.w[pg], h = P.h[pg];
    const int x = blockIdx.x * kThreads + threadIdx.x, y0 = (blockIdx.y + 1) * kChunk;
    if (x >= w || y0 >= h) return;
    const int y1 = min(y0 + kChunk, h) - 1;
    int32_t* col = P.sat[pg] + x;
    const int32_t add = col[(size_t)(y0 - 1) * w];
    for (int y = y0; y < y1; ++y) col[(size_t)y * w] += add;
}

// ------------------------------------------------------------------------------------------------ syllable boxes
struct BoxArgs {
    const uint8_t* ops; const int64_t* ops_off; const int32_t* ops_len;
    const int64_t* t_off; const int64_t* o_off; int32_t nprob;
    const int32_t* prob_page;
    const int32_t* char_box; const int64_t* char_off;
    const int32_t* syl_first; const int32_t* syl_last; const int64_t* syl_off;
    const double* rot;                  // per page: sin, cos, px, py, px - dx, py - dy
    int32_t max_syl; int32_t lds_cols;
    int32_t* out_box; uint8_t* out_present; int32_t* status;
};

__device__ inline int32_t rot_coord(double v) {
    // np.round (half to even) then astype('int16'): float64 -> int32 -> the low 16 bits, sign-extended
    return (int32_t)(int16_t)(int32_t)rint(v);
}

// one workgroup per problem; LDS: the column of every transcript character, then the OCR index of every column
__global__ void __launch_bounds__(kThreads) eval_boxes_kernel(BoxArgs A) {
    extern __shared__ int32_t lds[];
    __shared__ int32_t wave_t[kThreads / 64], wave_o[kThreads / 64];
    __shared__ int32_t bad;
    const int p = blockIdx.x;
    const int pg = A.prob_page[p];
    const int64_t s0 = A.syl_off[pg], nsyl = A.syl_off[pg + 1] - s0;
    int32_t* box = A.out_box + (size_t)p * A.max_syl * 4;
    uint8_t* present = A.out_present + (size_t)p * A.max_syl;
    for (int s = threadIdx.x; s < A.max_syl; s += kThreads) present[s] = 0;
    const int64_t n = A.t_off[p + 1] - A.t_off[p], m = A.o_off[p + 1] - A.o_off[p];
    const int32_t L = A.ops_len[p];
    if (L < 0) {                                  // the traceback did not finish
        if (threadIdx.x == 0) A.status[p] = TA_EVAL_UNFINISHED;
        return;
    }
    const int64_t nchars = A.char_off[pg + 1] - A.char_off[pg];
    if (m != nchars || n + L > A.lds_cols || L > n + m || nsyl > A.max_syl) {
        if (threadIdx.x == 0) A.status[p] = TA_EVAL_MISMATCH;
        return;
    }
    const uint8_t* ops = A.ops + A.ops_off[p] + n + m - L;
    int32_t* col_of_t = lds;                      // [n]
    int32_t* o_at = lds + n;                      // [L]: OCR index of a column, -1 for none
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad = 0;
    int32_t nt = 0, no = 0;
    for (int c0 = 0; c0 < L; c0 += kThreads) {
        const int c = c0 + threadIdx.x;
        const int op = (c < L) ? ops[c] : 1;
        const bool ht = (c < L) && op != 2, ho = (c < L) && op != 1;
        const uint64_t bt = __ballot(ht), bo = __ballot(ho);
        const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        const int32_t rt = __popcll(bt & below), ro = __popcll(bo & below);
        if (lane == 0) { wave_t[wave] = __popcll(bt); wave_o[wave] = __popcll(bo); }
        __syncthreads();
        int32_t bt_before = 0, bo_before = 0, at = 0, ao = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            bt_before += (k < wave) ? wave_t[k] : 0; at += wave_t[k];
            bo_before += (k < wave) ? wave_o[k] : 0; ao += wave_o[k];
        }
        const int32_t ti = nt + bt_before + rt, oi = no + bo_before + ro;
        if (ht) {
            if (ti < n) col_of_t[ti] = c; else bad = 1;
        }
        if (c < L) o_at[c] = ho ? ((oi < m) ? oi : (bad = 1, -1)) : -1;
        nt += at; no += ao;
        __syncthreads();
    }
    if (nt != n || no != m) bad = 1;
    __syncthreads();
    if (bad) {
        if (threadIdx.x == 0) A.status[p] = TA_EVAL_MISMATCH;
        return;
    }
    const int32_t* cb = A.char_box + 4 * A.char_off[pg];
    const double* R = A.rot + 6 * pg;
    const double sn = R[0], cs = R[1];
    const int64_t px = (int64_t)R[2], py = (int64_t)R[3];
    const double qx = R[4], qy = R[5];
    for (int64_t s = threadIdx.x; s < nsyl; s += kThreads) {
        const int32_t f = A.syl_first[s0 + s], l = A.syl_last[s0 + s];
        if (f < 0 || l < f || l >= n) { bad = 1; continue; }
        const int32_t c0 = col_of_t[f], c1 = col_of_t[l] + 1;
        int32_t low = INT_MIN;
        for (int c = c0; c < c1; ++c) {
            const int32_t o = o_at[c];
            if (o >= 0) low = max(low, cb[4 * o + 1]);
        }
        if (low == INT_MIN) continue;             // aligned to no OCR character: no box
        int32_t ulx = INT_MAX, uly = INT_MAX, lrx = INT_MIN, lry = INT_MIN;
        for (int c = c0; c < c1; ++c) {
            const int32_t o = o_at[c];
            if (o < 0 || cb[4 * o + 1] != low) continue;
            ulx = min(ulx, cb[4 * o]); uly = min(uly, cb[4 * o + 1]);
            lrx = max(lrx, cb[4 * o + 2]); lry = max(lry, cb[4 * o + 3]);
        }
        // rotate_boxes: x = v - px (int64), nx = (x * c) - (y * s) + (px - dx), ny = (x * s) + (y * c) + (py - dy)
        const double x0 = (double)(ulx - px), y0 = (double)(uly - py), x1 = (double)(lrx - px), y1 = (double)(lry - py);
        int32_t* b = box + 4 * s;
        b[0] = rot_coord(((x0 * cs) - (y0 * sn)) + qx);
        b[1] = rot_coord(((x0 * sn) + (y0 * cs)) + qy);
        b[2] = rot_coord(((x1 * cs) - (y1 * sn)) + qx);
        b[3] = rot_coord(((x1 * sn) + (y1 * cs)) + qy);
        present[s] = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) A.status[p] = bad ? TA_EVAL_MISMATCH : TA_EVAL_OK;
}

// ------------------------------------------------------------------------------------------------ scores
struct ScoreArgs {
    int32_t nprob; const int32_t* prob_page;
    const int32_t* boxes; const uint8_t* present; const int32_t* box_status; int32_t max_syl;
    const int32_t* gt; const int64_t* rep_off;              // counted gt boxes [.][4] = ulx, uly, lrx, lry; per page
    const int64_t* cand_off; const int32_t* cand;           // CSR per gt box: syllable indices, ascending
    const int32_t* const* sat; const int32_t* sat_h; const int32_t* sat_w;
    const int64_t* out_off;                                  // first output of problem p
    double* iou; double* area; int32_t* status;
};

// ink pixels of [x0..x1] x [y0..y1] inclusive; false if the rectangle is not inside the plane
__device__ inline bool rect_ink(const int32_t* S, int h, int w, int x0, int y0, int x1, int y1, int64_t* out) {
    if (x0 < 0 || y0 < 0 || x1 >= w || y1 >= h || x1 < x0 || y1 < y0) return false;
    auto at = [&](int x, int y) -> int64_t { return (x < 0 || y < 0) ? 0 : (int64_t)S[(size_t)y * w + x]; };
    *out = at(x1, y1) - at(x0 - 1, y1) - at(x1, y0 - 1) + at(x0 - 1, y0 - 1);
    return true;
}

__global__ void __launch_bounds__(64) eval_score_kernel(ScoreArgs A) {
    const int p = blockIdx.y;
    const int pg = A.prob_page[p];
    const int64_t r0 = A.rep_off[pg], nrep = A.rep_off[pg + 1] - r0;
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= nrep) return;
    const int64_t o = A.out_off[p] + r;
    const int32_t bs = A.box_status[p];
    if (bs != TA_EVAL_OK) { A.iou[o] = __builtin_nan(""); A.area[o] = __builtin_nan(""); A.status[o] = bs; return; }
    const int32_t* g = A.gt + 4 * (r0 + r);
    const int32_t gx0 = g[0], gy0 = g[1], gx1 = g[2], gy1 = g[3];
    const int32_t* B = A.boxes + (size_t)p * A.max_syl * 4;
    const uint8_t* pres = A.present + (size_t)p * A.max_syl;
    int64_t best_int = 0;
    int best = -1;
    for (int64_t k = A.cand_off[r0 + r]; k < A.cand_off[r0 + r + 1]; ++k) {
        const int s = A.cand[k];
        if (s < 0 || s >= A.max_syl || !pres[s]) continue;
        const int32_t* b = B + 4 * s;
        const int64_t dx = (int64_t)min(gx1, b[2]) - max(gx0, b[0]);
        const int64_t dy = (int64_t)min(gy1, b[3]) - max(gy0, b[1]);
        const int64_t v = (dx > 0 && dy > 0) ? dx * dy : 0;
        if (v > best_int) { best_int = v; best = s; }       // the FIRST maximum; no positive one scores 0
    }
    if (best < 0) { A.iou[o] = 0.0; A.area[o] = 0.0; A.status[o] = TA_EVAL_OK; return; }
    const int32_t* b = B + 4 * best;
    const int32_t nx0 = max(gx0, b[0]), ny0 = max(gy0, b[1]), nx1 = min(gx1, b[2]), ny1 = min(gy1, b[3]);
    const int64_t ai = (int64_t)(nx1 - nx0) * (ny1 - ny0);
    const int64_t a1 = (int64_t)(gx1 - gx0) * (gy1 - gy0), a2 = (int64_t)(b[2] - b[0]) * (b[3] - b[1]);
    A.iou[o] = (double)ai / (double)(a1 + a2 - ai);
    int64_t k1, k2, ki;
    const int32_t* S = A.sat[pg];
    const int h = A.sat_h[pg], w = A.sat_w[pg];
    if (!rect_ink(S, h, w, gx0, gy0, gx1, gy1, &k1) || !rect_ink(S, h, w, b[0], b[1], b[2], b[3], &k2) ||
        !rect_ink(S, h, w, nx0, ny0, nx1, ny1, &ki)) {
        A.area[o] = __builtin_nan(""); A.status[o] = TA_EVAL_OUT_OF_RANGE; return;
    }
    const int64_t den = k1 + k2 - ki;
    if (den == 0) { A.area[o] = __builtin_nan(""); A.status[o] = TA_EVAL_ZERO_AREA; return; }
    A.area[o] = (double)ki / (double)den;
    A.status[o] = TA_EVAL_OK;
}

#define EVAL_LAUNCH_CHECK(what)                               \
    do {                                                      \
        hipError_t e_ = hipGetLastError();                    \
        if (e_ != hipSuccess) return ta_fail_hip(e_, what);   \
    } while (0)

}  // namespace

extern "C" int ta_eval_integral(int32_t n, const uint8_t* const* ink, const int32_t* h, const int32_t* w,
                                int32_t* const* sat, void* stream) {
    if (n < 0) return ta_fail(TA_EINVAL, "negative count");
    if (n == 0) return TA_OK;
    if (!ink || !h || !w || !sat) return ta_fail(TA_EINVAL, "null pointer argument");
    for (int i = 0; i < n; ++i) {
        if (h[i] < 0 || w[i] < 0) return ta_fail(TA_EINVAL, "negative size");
        if ((int64_t)h[i] * w[i] > (int64_t)INT32_MAX) return ta_fail(TA_EINVAL, "a page has more than 2^31 - 1 pixels");
        if ((int64_t)h[i] * w[i] > 0 && (!ink[i] || !sat[i])) return ta_fail(TA_EINVAL, "null pointer argument");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int p0 = 0; p0 < n; p0 += kEvalPages) {
        SatPages P{};
        int m = 0, hmax = 0, wmax = 0;
        for (int i = p0; i < n && i < p0 + kEvalPages; ++i) {
            if ((int64_t)h[i] * w[i] == 0) continue;
            P.ink[m] = ink[i]; P.sat[m] = sat[i]; P.h[m] = h[i]; P.w[m] = w[i];
            hmax = h[i] > hmax ? h[i] : hmax; wmax = w[i] > wmax ? w[i] : wmax;
            ++m;
        }
        if (!m) continue;
        const int tiles = (wmax + kThreads - 1) / kThreads, chunks = (hmax + kChunk - 1) / kChunk;
        hipLaunchKernelGGL(sat_rows_kernel, dim3(hmax, 1, m), dim3(kThreads), 0, st, P);
        hipLaunchKernelGGL(sat_chunk_cols_kernel, dim3(tiles, chunks, m), dim3(kThreads), 0, st, P);
        hipLaunchKernelGGL(sat_carry_kernel, dim3(tiles, 1, m), dim3(kThreads), 0, st, P);
        if (chunks > 1) hipLaunchKernelGGL(sat_add_kernel, dim3(tiles, chunks - 1, m), dim3(kThreads), 0, st, P);
        EVAL_LAUNCH_CHECK("sat kernels");
    }
    return TA_OK;
}

extern "C" int32_t ta_eval_max_columns(void) { return TA_EVAL_MAX_COLUMNS; }

extern "C" int ta_eval_syllable_boxes(const uint8_t* ops, const int64_t* ops_off, const int32_t* ops_len,
                                      const int64_t* t_off, const int64_t* o_off, int32_t nprob, const int32_t* prob_page,
                                      const int32_t* char_box, const int64_t* char_off, const int32_t* syl_first,
                                      const int32_t* syl_last, const int64_t* syl_off, const double* rot,
                                      int32_t max_syl, int32_t max_cols, int32_t* out_box, uint8_t* out_present,
                                      int32_t* status, void* stream) {
    if (nprob < 0 || max_syl < 0 || max_cols < 0) return ta_fail(TA_EINVAL, "negative count");
    if (nprob == 0) return TA_OK;
    if (!ops || !ops_off || !ops_len || !t_off || !o_off || !prob_page || !char_box || !char_off || !syl_first ||
        !syl_last || !syl_off || !rot || !status || (max_syl > 0 && (!out_box || !out_present)))
        return ta_fail(TA_EINVAL, "null pointer argument");
    if (max_cols > TA_EVAL_MAX_COLUMNS)
        return ta_fail(TA_ELIMIT, "a problem's transcript + alignment columns exceed the LDS of ta_eval_syllable_boxes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(max_cols > 0 ? max_cols : 1) * sizeof(int32_t);
    if (lds > 64 * 1024) {
        hipError_t e = allow_full_lds(eval_boxes_kernel);
        if (e != hipSuccess) return ta_fail_hip(e, "eval_boxes_kernel LDS attribute");
    }
    BoxArgs A{ops, ops_off, ops_len, t_off, o_off, nprob, prob_page, char_box, char_off, syl_first, syl_last, syl_off,
              rot, max_syl, max_cols, out_box, out_present, status};
    hipLaunchKernelGGL(eval_boxes_kernel, dim3(nprob), dim3(kThreads), lds, st, A);
    EVAL_LAUNCH_CHECK("eval_boxes_kernel");
    return TA_OK;
}

extern "C" int ta_eval_score(int32_t nprob, const int32_t* prob_page, const int32_t* boxes, const uint8_t* present,
                             const int32_t* box_status, int32_t max_syl, const int32_t* gt, const int64_t* rep_off,
                             const int64_t* cand_off, const int32_t* cand, const int32_t* const* sat,
                             const int32_t* sat_h, const int32_t* sat_w, const int64_t* out_off, int32_t max_rep,
                             double* iou, double* area, int32_t* status, void* stream) {
    if (nprob < 0 || max_syl < 0 || max_rep < 0) return ta_fail(TA_EINVAL, "negative count");
    if (nprob == 0 || max_rep == 0) return TA_OK;
    if (!prob_page || !boxes || !present || !box_status || !gt || !rep_off || !cand_off || !cand || !sat || !sat_h ||
        !sat_w || !out_off || !iou || !area || !status)
        return ta_fail(TA_EINVAL, "null pointer argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScoreArgs A{nprob, prob_page, boxes, present, box_status, max_syl, gt, rep_off, cand_off, cand, sat, sat_h, sat_w,
                out_off, iou, area, status};
    hipLaunchKernelGGL(eval_score_kernel, dim3((max_rep + 63) / 64, nprob), dim3(64), 0, st, A);
    EVAL_LAUNCH_CHECK("eval_score_kernel");
    return TA_OK;
}
