// pp_cc.h -- what the two connected-component labellers and the two skew-search kernels of ta_preproc.hip share: the
// run masks of a 64-pixel segment, the join of a run to the row above, the lock-free union, and the row a point of the
// decimated page lands on.  Compiles for the host with a plain C++ compiler too (tests/native/sim_pp.cpp labels pages
// with these blocks against scipy.ndimage.label and holds the rows against numpy without a GPU); there the atomic
// minimum is a plain one and dmul / dadd are the plain operators, to be built with -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <math.h>

#include "corr1d.h"                          // dmul / dadd: explicit non-fused multiply and add

#if defined(__HIPCC__)
#define TA_PP __device__ __forceinline__
#else
#define TA_PP inline
#endif

namespace ta {

// ---- runs.  m: the ballot of a 64-pixel segment of a row (bit k = pixel k has the wanted value), carry: the last bit
// of the segment before it, next: the ballot of the segment after it.  A run starts at a set bit whose left neighbour
// is clear and ends at one whose right neighbour is clear.  Counting and writing the runs must use the SAME start mask,
// or every table index is off.
TA_PP unsigned long long run_starts(unsigned long long m, unsigned long long carry) { return m & ~((m << 1) | carry); }
TA_PP unsigned long long run_ends(unsigned long long m, unsigned long long next) { return m & ~((m >> 1) | ((next & 1ull) << 63)); }

constexpr int kRunBand = 32;                 // rows of a band: runs are joined inside the bands first, then across their borders

// ---- join to the row above (8-connectivity): the run [rx0, rx1] touches the runs of the row above -- x0 / x1 of the
// runs a .. end - 1, in raster order -- whose columns reach [rx0 - 1, rx1 + 1].  The first of them is the first that
// ends at rx0 - 1 or beyond (binary search), and they are consecutive: the walk stops at the first that starts past
// rx1 + 1.
TA_PP int first_touching_run(const int32_t* x1, int a, int b, int lo) {
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (x1[mid] < lo) a = mid + 1; else b = mid;
    }
    return a;
}
template <class Link>
TA_PP void join_up(const int32_t* x0, const int32_t* x1, int a, int end, int rx0, int rx1, Link link) {
    const int lo = rx0 - 1, hi = rx1 + 1;
    for (int j = first_touching_run(x1, a, end, lo); j < end && x0[j] <= hi; ++j) link(j);
}

// ---- union-find on an array of parents: a root is an entry that points to itself, the smaller index wins a union, so
// a component's root ends up its raster-first element whatever the order of the unions.
TA_PP int32_t uf_root(const int32_t* parent, int32_t a) {
    while (true) { const int32_t p = parent[a]; if (p == a) return a; a = p; }
}
TA_PP int32_t uf_atomic_min(int32_t* p, int32_t v) {
#if defined(__HIPCC__)
    return atomicMin(p, v);
#else
    const int32_t old = *p;
    if (v < old) *p = v;
    return old;
#endif
}
// lock-free: find(x) = some ancestor of x that was a root when looked at (the plain chase over LDS, the path-halving
// uf_find of ta_preproc.hip over memory)
template <class Find>
TA_PP void uf_unite_by(int32_t* parent, Find find, int32_t a, int32_t b) {
    while (true) {
        a = find(a); b = find(b);
        if (a == b) return;
        if (a > b) { const int32_t t = a; a = b; b = t; }          // the larger root goes under the smaller
        const int32_t old = uf_atomic_min(&parent[b], a);
        if (old == b) return;                                       // b was still a root: linked
        b = old;                                                    // b had been linked elsewhere meanwhile: unite with that
    }
}

// ---- skew search: pixel (ys, xs) of the decimated page (centre cy, cx) lands on row rint(cy + dy cos a - dx sin a) of
// the page turned by a.  Float64, one rounding per operation, in numpy's order: t0 belongs to the row, the rest to the point.
TA_PP double skew_t0(int ys, double cy, double ca) { return dadd(cy, dmul(dadd((double)ys, -cy), ca)); }
TA_PP long long skew_row(double t0, int xs, double cx, double sa) {
    return (long long)rint(dadd(t0, -dmul(dadd((double)xs, -cx), sa)));
}

}  // namespace ta
