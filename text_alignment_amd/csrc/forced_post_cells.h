// forced_post_cells.h -- the sum-product arithmetic that ta_forced_post.hip (a lattice per line)
// and ta_forced_page_post.hip (one lattice through all lines of a page, section 14.15) share: a value as a pair
// (double m, int x) = m 2^x that is not kept normalised, its add, its renormalisation, the moves to the neighbouring lanes,
// the clamped float32 emission, and PostCells: a frame of the forward and of the backward fill for a lane's K states, the
// row a query frame keeps and the candidates of a combine.  The rule and why the results do not depend on where the
// renormalisation happens: ta_forced_post.hip's opening comment.  Both files are built with -ffp-contract=off.
#pragma once
#include "forced_two_fill.h"

namespace {

constexpr int kZeroX = -(1 << 29);                     // zero's exponent: two of them still add inside an int
constexpr int kShift = 256;
constexpr int kKeyNone = INT32_MIN;                    // a lane without a candidate
constexpr int kKeyZero = INT32_MIN + 1;                // a candidate whose g is zero: below every real exponent

struct Val { double m; int x; };                       // m 2^x, m >= 0

__device__ __forceinline__ Val add(Val a, Val b) {
    const int x = a.x > b.x ? a.x : b.x;
    const int da = a.x - x > -kShift ? a.x - x : -kShift, db = b.x - x > -kShift ? b.x - x : -kShift;
    return Val{ldexp(a.m, da) + ldexp(b.m, db), x};
}
__device__ __forceinline__ Val normal(Val a) {         // m in [0.5, 1); zero keeps kZeroX (frexp gives it exponent 0)
    int e;
    const double m = frexp(a.m, &e);
    return Val{m, a.x + e};
}
__device__ __forceinline__ long long bits_of(double d) { long long u; __builtin_memcpy(&u, &d, 8); return u; }
__device__ __forceinline__ double double_of(long long u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
__device__ __forceinline__ Val left_of(Val v) {        // lane l takes lane l - 1's, lane 0 zero
    return Val{double_of(from_left(bits_of(v.m), 0)), __builtin_amdgcn_update_dpp(kZeroX, v.x, 0x138, 0xf, 0xf, false)};
}
__device__ __forceinline__ Val right_of(Val v) {       // lane l takes lane l + 1's, lane 63 zero
    return Val{double_of(from_right(bits_of(v.m), 0)), __builtin_amdgcn_update_dpp(kZeroX, v.x, 0x130, 0xf, 0xf, false)};
}
__device__ __forceinline__ float emission_f(float p) {
    const float a = p > 0x1p-17f ? p : 0x1p-17f;       // emission_q's two comparisons: NaN, 0 and negatives give the floor
    return a < 1.0f ? a : 1.0f;
}

struct PostLine : TwoFillLine {
    double* own_m; int32_t* own_x; double* rival_m; int32_t* rival_x; int32_t* rival_state;     // its rows of the outputs
    double* z_m; int32_t* z_x; // its entry of the two per line
};

// the LDS of a combine: 64 lanes' candidates, 8 partial bests, the own state's value ([72]); Z's two terms pass through too
struct PostRed { double m[73]; int x[73]; int s[73]; };

struct PostCand { int x; double m; int s; };           // a candidate: exponent, then significand, then the smaller state

// two_fill's arithmetic: sum-product on (double, int) pairs; a forward row is 64 K doubles, then 64 K exponents, per
// character
struct PostCells {
    using V = Val;
    using E = float;           // the emissions stay float32
    using Line = PostLine;
    using Red = PostRed;
    using Cand = PostCand;
    static constexpr int64_t kRowBytes = 768;
    __device__ static __forceinline__ void put(Red* red, int i, Cand c) { red->x[i] = c.x; red->m[i] = c.m; red->s[i] = c.s; }
    __device__ static __forceinline__ Cand get(const Red* red, int i) { return Cand{red->x[i], red->m[i], red->s[i]}; }
    __device__ static __forceinline__ bool better(Cand a, Cand b) {
        return a.x > b.x || (a.x == b.x && (a.m > b.m || (a.m == b.m && a.s < b.s)));
    }
    __device__ static __forceinline__ V zero() { return Val{0.0, kZeroX}; }
    __device__ static __forceinline__ V one() { return Val{1.0, 0}; }
    __device__ static __forceinline__ E emit(float p) { return emission_f(p); }
    __device__ static __forceinline__ V first(E e) { return Val{(double)e, 0}; }
    __device__ static __forceinline__ V left(V v) { return left_of(v); }
    template <int K> __device__ static __forceinline__ void chunk_begin(V (&v)[K]) {         // renormalise
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = normal(v[k]);
    }
    template <int K> __device__ static __forceinline__ double* row_m(const Line& ln, int i) {
        return reinterpret_cast<double*>(ln.fwd + (int64_t)i * (768 * K));
    }
    template <int K> __device__ static __forceinline__ int* row_x(const Line& ln, int i) {
        return reinterpret_cast<int*>(ln.fwd + (int64_t)i * (768 * K) + 512 * K);
    }

    // kFirst (a page alone): the first frame of a line behind the page's first, in which a label state has no stay term
    template <int K, bool kFirst = false>
    __device__ static __forceinline__ void forward(V (&v)[K], V left, unsigned skip, const int (&lab)[K / 2], const E* e) {
        const Val zero{0.0, kZeroX};
        const double eb = (double)e[0];
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {             // downwards: v[k - 1] and v[k - 2] are still the old row's
            Val y = add((kFirst && (k & 1)) ? zero : v[k], k >= 1 ? v[k - 1] : left);
            if (k & 1) {
                const Val sk = k >= 2 ? v[k - 2] : left;
                y = add(y, ((skip >> (k >> 1)) & 1u) ? sk : zero);
                v[k] = Val{y.m * (double)e[lab[k >> 1]], y.x};
            } else {
                v[k] = Val{y.m * eb, y.x};
            }
        }
    }

    template <int K>
    __device__ static __forceinline__ void backward(V (&v)[K], unsigned skipf, const int (&lab)[K / 2], const E* e) {
        const Val zero{0.0, kZeroX};
        const double eb = (double)e[0];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k].m *= (k & 1) ? (double)e[lab[k >> 1]] : eb;
        const Val r0 = right_of(v[0]), r1 = right_of(v[1]);
#pragma unroll
        for (int k = 0; k < K; ++k) {                  // upwards: v[k + 1] and v[k + 2] still carry frame t
            Val y = add(v[k], k + 1 < K ? v[(k + 1) % K] : r0);
            if (k & 1) {
                const Val sk = k + 2 < K ? v[(k + 2) % K] : r1;
                y = add(y, ((skipf >> (k >> 1)) & 1u) ? sk : zero);
            }
            v[k] = y;
        }
    }

    template <int K>
    __device__ static __forceinline__ void store_row(const Line& ln, int cur, int lane, const V (&v)[K]) {
        double* rm = row_m<K>(ln, cur);
        int* rx = row_x<K>(ln, cur);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rm[k * 64 + lane] = v[k].m;
            rx[k * 64 + lane] = v[k].x;
        }
    }

    // Z = a[S - 1] + a[S - 2]
    template <int K>
    __device__ static __forceinline__ void forward_done(const Line& ln, int lane, int S, const V (&v)[K], Red* redp) {
        Red& red = *redp;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane * K + k;
            if (s == S - 1) { red.m[0] = v[k].m; red.x[0] = v[k].x; }
            if (s == S - 2) { red.m[1] = v[k].m; red.x[1] = v[k].x; }
        }
        wave_lds_sync();
        if (lane == 0) {
            const Val z = normal(add(Val{red.m[0], red.x[0]}, Val{red.m[1], red.x[1]}));
            *ln.z_m = z.m;
            *ln.z_x = z.m == 0.0 ? 0 : z.x;
        }
        wave_lds_sync();                               // red is free again
    }

    // character `cur` at the frame v holds b of
    template <int K>
    __device__ static __forceinline__ void combine(const Line& ln, int cur, int lane, int S, const V (&v)[K], Red* redp) {
        Red& red = *redp;
        const double* rm = row_m<K>(ln, cur);
        const int* rx = row_x<K>(ln, cur);
        const int own = 2 * cur + 1;
        Cand best{kKeyNone, 0.0, 0};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane * K + k;
            // what this very lane stored in the forward fill
            const Val g = normal(Val{rm[k * 64 + lane] * v[k].m, rx[k * 64 + lane] + v[k].x});
            const int gx = g.m == 0.0 ? kKeyZero : g.x;
            if (s == own) { red.m[72] = g.m; red.x[72] = gx; }
            else if (s < S && better(Cand{gx, g.m, s}, best)) best = Cand{gx, g.m, s};
        }
        best = two_fill_best<PostCells>(redp, lane, best);
        if (lane == 0) {
            ln.own_m[cur] = red.m[72];
            ln.own_x[cur] = red.x[72] == kKeyZero ? 0 : red.x[72];
            ln.rival_m[cur] = best.m;
            ln.rival_x[cur] = best.x == kKeyZero ? 0 : best.x;
            ln.rival_state[cur] = best.s;
        }
        wave_lds_sync();                               // red is free again
    }
};

}  // namespace
