// Host run of the gaussians' tap loop (text_alignment_amd/csrc/corr1d.h, the header the HIP kernels compile):
// ring_taps<NO> along one line of doubles, group after group of NO outputs, under the two border rules the kernels
// use.  tests/test_corr1d.py holds the result against scipy.ndimage.correlate1d bit for bit.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC (no contraction: the header's dmul / dadd are the plain
// operators here).
#include "../../text_alignment_amd/csrc/corr1d.h"

namespace {

// (d c b a | a b c d | d c b a): period 2 n
int reflect(long k, int n) {
    long m = k % (2L * n);
    if (m < 0) m += 2L * n;
    return (int)(m < n ? m : 2L * n - 1 - m);
}

template <int NO>
void run(const double* x, int n, const double* wc, int rad, int mode, double* out) {
    // zeros outside: beyond n - 1 both taps of a pair are zeros (ta_lineest.hip); reflect: every tap (ta_distort.hip)
    const int reach = mode == 0 ? (rad < n - 1 ? rad : n - 1) : rad;
    for (int j0 = 0; j0 < n; j0 += NO) {
        double t[NO];
        if (mode == 0)
            ta::ring_taps<NO>([&](int k) -> double { return (j0 + k >= 0 && j0 + k < n) ? x[j0 + k] : 0.0; }, wc, reach, t);
        else
            ta::ring_taps<NO>([&](int k) -> double { return x[reflect((long)j0 + k, n)]; }, wc, reach, t);
        for (int q = 0; q < NO && j0 + q < n; ++q) out[j0 + q] = t[q];
    }
}

}  // namespace

// w: the 2 rad + 1 weights; mode 0: zeros outside ('constant'), 1: 'reflect'.  Returns 0, or -1 for an NO that is not built.
extern "C" int sim_corr1d(int no, const double* x, int n, const double* w, int rad, int mode, double* out) {
    const double* wc = w + rad;
    switch (no) {
        case 1: run<1>(x, n, wc, rad, mode, out); return 0;
        case 4: run<4>(x, n, wc, rad, mode, out); return 0;
        case 5: run<5>(x, n, wc, rad, mode, out); return 0;
        case 7: run<7>(x, n, wc, rad, mode, out); return 0;
        case 8: run<8>(x, n, wc, rad, mode, out); return 0;
        case 9: run<9>(x, n, wc, rad, mode, out); return 0;
    }
    return -1;
}
