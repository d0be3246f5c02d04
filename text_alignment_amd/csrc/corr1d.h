// corr1d.h -- what the gaussians of the line normaliser (ta_lineest.hip) and of the line distortion (ta_distort.hip)
// share: scipy's float64 correlate1d with a symmetric kernel, NO adjacent outputs at a time, and the workgroup's
// tree reduction.  The tap loop also compiles for the host with a plain C++ compiler (tests/native/sim_corr1d.cpp
// holds it against scipy bit for bit without a GPU); there dmul / dadd are the plain operators, to be built with
// -ffp-contract=off.  The distortion's two gaussians call ring_taps; the normaliser's four carry the same loop
// spelled out (the compiler schedules each of them differently around a call of the helper).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TA_C1D __device__ __forceinline__
#else
#define TA_C1D inline
#endif

namespace ta {

// explicit non-fused multiply and add
#if defined(__HIPCC__)
TA_C1D double dmul(double a, double b) { return __dmul_rn(a, b); }
TA_C1D double dadd(double a, double b) { return __dadd_rn(a, b); }
#else
TA_C1D double dmul(double a, double b) { return a * b; }
TA_C1D double dadd(double a, double b) { return a + b; }
#endif

// NO adjacent outputs t[0 .. NO) of one line.  X(k) is element k of the EXTENDED line (zeros or reflections outside,
// the caller's border rule) relative to the first output, valid for -reach <= k < NO + reach; wc points at the centre
// tap of the symmetric kernel, of which the taps -reach .. reach are used (with zeros outside, beyond the line's
// length - 1 both taps of a pair are zeros: reach = min(radius, length - 1)).
// Every output sums its own products in scipy's order: centre tap first, then the tap pairs from the outermost
// inwards, (x[j + jj] + x[j - jj]) * w[jj] for jj = -reach .. -1.
// The two tap windows x[jj .. jj + NO) and x[-jj .. -jj + NO) slide by one element per tap pair, so each pair costs
// two new elements for NO outputs.  The windows are RINGS: at the u-th tap of a round of NO, element q of the low
// window sits in lo[(q + u) % NO] and of the high window in hi[(q - u) mod NO] -- a slide costs one load each and no
// register moves (shifting 2 x NO doubles per tap pair cost as much as the arithmetic).
template <int NO, class Line>
TA_C1D void ring_taps(Line X, const double* wc, int reach, double* t) {
    double lo[NO], hi[NO];
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        t[q] = dmul(X(q), wc[0]);
        lo[q] = X(q - reach);
        hi[q] = X(q + reach);
    }
    for (int jb = -reach; jb < 0; jb += NO) {
#pragma unroll
        for (int u = 0; u < NO; ++u) {
            const int jj = jb + u;
            if (jj < 0) {
                const double wj = wc[jj];
#pragma unroll
                for (int q = 0; q < NO; ++q)
                    t[q] = dadd(t[q], dmul(dadd(lo[(q + u) % NO], hi[(q - u + NO) % NO]), wj));
                lo[u % NO] = X(jj + NO);                    // enters as element NO - 1 of tap jj + 1's window
                hi[(NO - 1 - u) % NO] = X(-jj - 1);         // enters as element 0
            }
        }
    }
}

// the same over C[k * stride] = element k
template <int NO>
TA_C1D void ring_taps(const double* C, int stride, const double* wc, int reach, double* t) {
    ring_taps<NO>([&](int k) -> double { return C[k * stride]; }, wc, reach, t);
}

#if defined(__HIPCC__)
// Tree reduction over the kThreads entries that a workgroup of kThreads threads has written to its LDS arrays:
// combine(i, j) folds entry j into entry i (of one array or of several at once); the result is entry 0.
template <int kThreads, class Combine>
TA_C1D void block_reduce(int tid, Combine combine) {
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) combine(tid, tid + s);
        __syncthreads();
    }
}
#endif

}  // namespace ta
