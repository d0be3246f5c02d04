// ta_distort.hip -- random elastic distortion of text-line strips on the GPU, the training augmentation of
// ocropy's `rdistort` / the ocrodeg recipe (third-party arithmetic, parity unpinned; the
// checker of record is tests/distort_ref.py).
//
// Per strip (h x w uint8, white background) and field (0: row displacement, 1: column displacement):
//   N = standard normal noise from Philox4x32-10, counter words (pixel, 0, line counter), key = seed, Box-Muller
//   F = gaussian_filter(N, dsigma) as scipy defines it: axis 0 then axis 1, radius int(4 dsigma + 0.5), mode 'reflect'
//   D = F * (distort / max |F|)
// and the strip is resampled bilinearly at (y + D0, x + D1), cval = the strip's maximum outside, floor(v + 0.5).
// Everything is float64 with explicit non-fused operations; each output sums its taps in scipy's order (centre tap,
// then the pairs from the outermost inwards).
//
// Four kernels per batch, one launch each:
//   ds_imax_kernel      the strip's maximum (cval)
//   ds_noise_col_kernel a tile of columns: noise straight into LDS -- the column EXTENDED by its reflections, so the tap
//                       loop has no index arithmetic -- and the vertical pass over it; the noise never reaches HBM
//   ds_row_kernel       the horizontal pass over a row tile staged in LDS (extended the same way) and max |F| per
//                       (line, field): an atomic max on the bit pattern of the non-negative double -- order-free
//   ds_resample_kernel  scale, sample, round into the packed output
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "corr1d.h"
#include "ta_common.h"

namespace ta {

constexpr int kDsThreads = 256;
constexpr int kDsColCells = 6144;                  // doubles of LDS of the column kernel (48 KB): (h + 2 r) x tile columns
constexpr int kDsColTile = 64;                     // at most this many columns per tile
constexpr int kDsRowMaxNO = 9;
constexpr int kDsRowCells = kDsThreads * kDsRowMaxNO + 2 * TA_DISTORT_MAX_RADIUS + kDsRowMaxNO;     // 6409 doubles, 50 KB
constexpr int kDsRowW5 = kDsThreads * 5;           // the widest strip with 5 outputs per lane in the row pass,
constexpr int kDsRowW7 = kDsThreads * 7;           // with 7; beyond it kDsRowMaxNO
constexpr int kDsGridTiles = 4096;                 // column tiles in the grid at most: a strip with more is swept
static_assert(TA_DISTORT_MAX_H + 2 * TA_DISTORT_MAX_RADIUS <= kDsColCells, "one extended column must fit the LDS tile");

struct DsArgs {
    const uint8_t* pix; const int64_t* pix_off;      // [h][w] per line; the output has the same layout
    const int32_t* hh; const int32_t* ww;
    const uint64_t* counters;                        // [nlines]
    int32_t nlines;
    uint32_t seed_lo, seed_hi;
    const double* gw; int32_t rad;                   // gw: the CENTRE tap of the 2 rad + 1 weights
    double distort;
    double* V; double* F;                            // [2][h w] per line at 2 pix_off[line]: after the vertical pass, after both
    unsigned long long* fmax;                        // [nlines][2] bits of max |F|
    uint32_t* imax;                                  // [nlines] (stride 2 words)
    uint8_t* out; double* fields;                    // fields: optional [2][h w] per line, the scaled D
};

// index of the reflected extension (d c b a | a b c d | d c b a) of a line of n elements: period 2 n
__device__ __forceinline__ int ds_reflect(int k, int n) {
    int m = k % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// Philox4x32-10 (Salmon et al. 2011): counter c[4], key k[2]
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// standard normal of pixel p of a line, field 0 from outputs (0, 1), field 1 from (2, 3)
__device__ __forceinline__ double ds_noise(uint64_t p, uint64_t counter, uint32_t k0, uint32_t k1, int field) {
    uint32_t c[4] = {(uint32_t)p, (uint32_t)(p >> 32), (uint32_t)counter, (uint32_t)(counter >> 32)};
    philox4x32_10(c, k0, k1);
    const uint32_t ra = field ? c[2] : c[0], rb = field ? c[3] : c[1];
    const double ua = dmul(dadd((double)ra, 0.5), 2.3283064365386963e-10);          // 2^-32
    const double ub = dmul(dadd((double)rb, 0.5), 2.3283064365386963e-10);
    return dmul(sqrt(dmul(-2.0, log(ua))), cos(dmul(6.283185307179586, ub)));
}

__global__ __launch_bounds__(kDsThreads) void ds_imax_kernel(DsArgs a) {
    __shared__ int smax[kDsThreads];
    const int line = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)a.hh[line] * a.ww[line];
    const uint8_t* p = a.pix + a.pix_off[line];
    int hi = 0;
    for (int64_t e = tid; e < n; e += kDsThreads) hi = max(hi, (int)p[e]);
    smax[tid] = hi;
    block_reduce<kDsThreads>(tid, [&](int i, int j) { smax[i] = max(smax[i], smax[j]); });
    if (tid == 0) a.imax[2 * line] = (uint32_t)smax[0];
}

// columns per tile of the column pass: a power of two, as many as fit, (h + 2 rad) * ct <= kDsColCells.  The kernel
// and the host's grid take it from here
__host__ __device__ __forceinline__ int ds_col_tile(int h, int rad) {
    int ct = kDsColTile;
    while (ct > 1 && (h + 2 * rad) * ct > kDsColCells) ct >>= 1;
    return ct;
}

// grid (nlines, column tiles, 2 fields).  A tile is `ct` columns (ds_col_tile) by h + 2 rad rows: rows rad .. rad + h
// hold the noise, the rows around them its reflections.
__global__ __launch_bounds__(kDsThreads) void ds_noise_col_kernel(DsArgs a) {
    constexpr int NO = 4;
    __shared__ double L[kDsColCells];
    const int line = blockIdx.x, field = blockIdx.z, tid = threadIdx.x;
    const int h = a.hh[line], w = a.ww[line], rad = a.rad;
    const int ct = ds_col_tile(h, rad);
    const int64_t n = (int64_t)h * w;
    double* V = a.V + 2 * a.pix_off[line] + (int64_t)field * n;
    const uint64_t counter = a.counters[line];
    const int c = tid & (ct - 1), g = tid / ct, ngroups = kDsThreads / ct;
    for (int jt = blockIdx.y * ct; jt < w; jt += gridDim.y * ct) {
        __syncthreads();                                    // the tile before this one has been read
        for (int e = tid; e < h * ct; e += kDsThreads) {
            const int r = e / ct, cc = e & (ct - 1);
            if (jt + cc < w)
                L[(rad + r) * ct + cc] = ds_noise((uint64_t)((int64_t)r * w + jt + cc), counter, a.seed_lo, a.seed_hi, field);
        }
        __syncthreads();
        for (int e = tid; e < 2 * rad * ct; e += kDsThreads) {
            const int q = e / ct, cc = e & (ct - 1);
            const int r = q < rad ? q : q + h;              // extended row: above the strip, then below it
            L[r * ct + cc] = L[(rad + ds_reflect(r - rad, h)) * ct + cc];
        }
        __syncthreads();
        if (jt + c >= w) continue;
        for (int i0 = NO * g; i0 < h; i0 += NO * ngroups) {
            // (a full group's windows end at row i0 + NO - 1 + rad of the extension; the last group of a strip whose
            // height is no multiple of NO would read past it, so its outputs are computed one by one)
            double t[NO];
            if (i0 + NO <= h) {
                const double* C = L + (rad + i0) * ct + c;  // C[k * ct] = row i0 + k of the extended column
                ring_taps<NO>(C, ct, a.gw, rad, t);
#pragma unroll
                for (int q = 0; q < NO; ++q) V[(int64_t)(i0 + q) * w + jt + c] = t[q];
            } else {
                for (int i = i0; i < h; ++i) {
                    const double* C = L + (rad + i) * ct + c;
                    ring_taps<1>(C, ct, a.gw, rad, t);
                    V[(int64_t)i * w + jt + c] = t[0];
                }
            }
        }
    }
}

template <int NO>
__device__ __forceinline__ double ds_row_body(const double* S, double* D, const double* wc, int h, int w, int rad, double* L) {
    constexpr int kTile = kDsThreads * NO;
    const int tid = threadIdx.x;
    const int span = kTile + 2 * rad;
    double amax = 0.0;
    for (int i = blockIdx.y; i < h; i += gridDim.y) {
        const double* row = S + (int64_t)i * w;
        for (int jt = 0; jt < w; jt += kTile) {
            __syncthreads();                                // the tile before this one has been read
            for (int k = tid; k < span; k += kDsThreads) L[k] = row[ds_reflect(jt - rad + k, w)];
            __syncthreads();
            const int j0 = jt + NO * tid;
            if (j0 < w) {
                const double* C = L + rad + NO * tid;       // C[k] = element j0 + k of the extended row
                double t[NO];
                ring_taps<NO>([&](int k) -> double { return C[k]; }, wc, rad, t);
#pragma unroll
                for (int q = 0; q < NO; ++q)
                    if (j0 + q < w) { D[(int64_t)i * w + j0 + q] = t[q]; amax = fmax(amax, fabs(t[q])); }
            }
        }
    }
    return amax;
}

// grid (nlines, rows, 2 fields).  The outputs per thread follow the width so that one pass of the workgroup covers
// the row, all odd (an odd lane stride in doubles keeps a quarter-wave on different banks), as in ta_lineest.hip.
__global__ __launch_bounds__(kDsThreads) void ds_row_kernel(DsArgs a) {
    __shared__ double L[kDsRowCells];
    __shared__ double smax[kDsThreads];
    const int line = blockIdx.x, field = blockIdx.z, tid = threadIdx.x;
    const int h = a.hh[line], w = a.ww[line];
    const int64_t n = (int64_t)h * w;
    const double* S = a.V + 2 * a.pix_off[line] + (int64_t)field * n;
    double* D = a.F + 2 * a.pix_off[line] + (int64_t)field * n;
    double amax;
    if (w <= kDsRowW5) amax = ds_row_body<5>(S, D, a.gw, h, w, a.rad, L);
    else if (w <= kDsRowW7) amax = ds_row_body<7>(S, D, a.gw, h, w, a.rad, L);
    else amax = ds_row_body<kDsRowMaxNO>(S, D, a.gw, h, w, a.rad, L);
    smax[tid] = amax;
    block_reduce<kDsThreads>(tid, [&](int i, int j) { smax[i] = fmax(smax[i], smax[j]); });
    // non-negative doubles order as their bit patterns do (a NaN cannot arise: the noise is finite)
    if (tid == 0) atomicMax(a.fmax + 2 * line + field, (unsigned long long)__double_as_longlong(smax[0]));
}

__global__ __launch_bounds__(kDsThreads) void ds_resample_kernel(DsArgs a) {
    const int line = blockIdx.x;
    const int h = a.hh[line], w = a.ww[line];
    const int64_t n = (int64_t)h * w;
    const uint8_t* p = a.pix + a.pix_off[line];
    uint8_t* out = a.out + a.pix_off[line];
    const double* F0 = a.F + 2 * a.pix_off[line];
    const double* F1 = F0 + n;
    const double m0 = __longlong_as_double((long long)a.fmax[2 * line]), m1 = __longlong_as_double((long long)a.fmax[2 * line + 1]);
    const double s0 = m0 > 0.0 ? a.distort / m0 : 0.0, s1 = m1 > 0.0 ? a.distort / m1 : 0.0;
    const uint8_t cval = (uint8_t)a.imax[2 * line];
    double* fld = a.fields ? a.fields + 2 * a.pix_off[line] : nullptr;
    for (int64_t e = (int64_t)blockIdx.y * kDsThreads + threadIdx.x; e < n; e += (int64_t)gridDim.y * kDsThreads) {
        const int y = (int)(e / w), x = (int)(e % w);
        const double d0 = dmul(F0[e], s0), d1 = dmul(F1[e], s1);
        if (fld) { fld[e] = d0; fld[n + e] = d1; }
        const double sy = dadd((double)y, d0), sx = dadd((double)x, d1);
        uint8_t v = cval;
        if (sy >= 0.0 && sy <= (double)(h - 1) && sx >= 0.0 && sx <= (double)(w - 1)) {
            const int y0 = (int)floor(sy), x0 = (int)floor(sx);
            const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
            const double ty = dadd(sy, -(double)y0), tx = dadd(sx, -(double)x0);
            const double uy = dadd(1.0, -ty), ux = dadd(1.0, -tx);
            const double top = dadd(dmul(ux, (double)p[(int64_t)y0 * w + x0]), dmul(tx, (double)p[(int64_t)y0 * w + x1]));
            const double bot = dadd(dmul(ux, (double)p[(int64_t)y1 * w + x0]), dmul(tx, (double)p[(int64_t)y1 * w + x1]));
            v = (uint8_t)(int)floor(dadd(dadd(dmul(uy, top), dmul(ty, bot)), 0.5));
        }
        out[e] = v;
    }
}

}  // namespace ta

using namespace ta;

extern "C" int64_t ta_line_distort_workspace_bytes(int32_t nlines, int64_t total_pixels) {
    if (nlines < 0 || total_pixels < 0) return -1;
    return 24 * (int64_t)nlines + 32 * total_pixels;        // max |F| bits [n][2], strip maxima [n] (8 bytes each), V, F
}

extern "C" int ta_line_distort(const uint8_t* pix, const int64_t* pix_off, const int32_t* hh, const int32_t* ww,
                               const uint64_t* counters, int32_t nlines, const int32_t* hh_host,
                               const int32_t* ww_host, double distort, double dsigma, uint64_t seed,
                               const double* gw, void* workspace, int64_t workspace_bytes, uint8_t* out,
                               double* fields, void* stream) {
    if (nlines < 0) return ta_fail(TA_EINVAL, "negative line count");
    if (!(distort > 0.0) || !(dsigma > 0.0) || !(distort < 1e9)) return ta_fail(TA_EINVAL, "distort and dsigma must be positive");
    if (!(dsigma <= (double)TA_DISTORT_MAX_RADIUS)) return ta_fail(TA_ELIMIT, "dsigma: the gaussian's radius exceeds TA_DISTORT_MAX_RADIUS");
    const int rad = (int)(4.0 * dsigma + 0.5);
    if (rad > TA_DISTORT_MAX_RADIUS) return ta_fail(TA_ELIMIT, "dsigma: the gaussian's radius exceeds TA_DISTORT_MAX_RADIUS");
    if (nlines == 0) return TA_OK;
    if (!pix || !pix_off || !hh || !ww || !counters || !hh_host || !ww_host || !gw || !workspace || !out)
        return ta_fail(TA_EINVAL, "null pointer argument");
    int64_t total = 0;
    int max_h = 1, max_tiles = 1;
    for (int b = 0; b < nlines; ++b) {
        const int h = hh_host[b], w = ww_host[b];
        if (h < 1 || w < 1) return ta_fail(TA_EINVAL, "empty strip");
        if (h > TA_DISTORT_MAX_H) return ta_fail(TA_ELIMIT, "a strip is taller than TA_DISTORT_MAX_H");
        if ((int64_t)h * w > 0x7fffffff) return ta_fail(TA_ELIMIT, "a strip has more than 2^31 - 1 pixels");
        total += (int64_t)h * w;
        const int ct = ds_col_tile(h, rad);
        const int tiles = (w + ct - 1) / ct;
        if (tiles > max_tiles) max_tiles = tiles;
        if (h > max_h) max_h = h;
    }
    if (workspace_bytes < ta_line_distort_workspace_bytes(nlines, total))
        return ta_fail(TA_EINVAL, "workspace smaller than ta_line_distort_workspace_bytes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* wsb = static_cast<char*>(workspace);
    DsArgs a{pix, pix_off, hh, ww, counters, nlines, (uint32_t)seed, (uint32_t)(seed >> 32), gw + rad, rad, distort,
             reinterpret_cast<double*>(wsb + 24 * (int64_t)nlines),
             reinterpret_cast<double*>(wsb + 24 * (int64_t)nlines) + 2 * total,
             reinterpret_cast<unsigned long long*>(wsb), reinterpret_cast<uint32_t*>(wsb + 16 * (int64_t)nlines),
             out, fields};
    hipError_t e = hipMemsetAsync(workspace, 0, 24 * (size_t)nlines, st);
    if (e != hipSuccess) return ta_fail_hip(e, "line distortion memset");
    const unsigned tiles_y = (unsigned)(max_tiles < kDsGridTiles ? max_tiles : kDsGridTiles);
    hipLaunchKernelGGL(ds_imax_kernel, dim3(nlines), dim3(kDsThreads), 0, st, a);
    hipLaunchKernelGGL(ds_noise_col_kernel, dim3(nlines, tiles_y, 2), dim3(kDsThreads), 0, st, a);
    hipLaunchKernelGGL(ds_row_kernel, dim3(nlines, max_h, 2), dim3(kDsThreads), 0, st, a);
    hipLaunchKernelGGL(ds_resample_kernel, dim3(nlines, 32), dim3(kDsThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "line distortion launch");
    return TA_OK;
}
