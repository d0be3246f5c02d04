// tests/native/sim_lineest.cpp -- host build of the line normaliser's kernels (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_lineest.hip ITSELF -- not a restatement -- against tests/native/hipshim_wg, where a
// workgroup is 256 lanes that meet at every barrier.  The library this makes exports the same ta_linenorm_measure /
// ta_linenorm_resample, taking host pointers where the real ones take device pointers, so the four spelled-out tap loops,
// the row kernel's tiles and halo, the column kernel's zero row, the box filter's chunks, the reflect loop and the
// dewarp's bounds are run against oracle/lineest_ref.py without a GPU (tests/test_lineest_sim.py).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim_wg (no contraction: the
// explicit multiplies and adds are the plain operators here).
// With -DSIM_LINEEST_MAIN the same source is a program -- for a build with -fsanitize=address,undefined: every buffer it
// hands the kernels is a heap block of exactly the size the caller owes them.
//   sim_lineest IN OUT
// IN:  int64 nlines, npix, ngw; int32 hh[n], ww[n]; int64 gw_off[3 n]; int32 gr[3 n]; double gw[ngw]; uint8 pix[npix]
//      (strip k's pixels follow strip k - 1's)
// OUT: int32 r[n], wout[n], arg[sum w], center[sum w]; float x[sum (wout + 32)][48]
#define __HIPCC__ 1             // corr1d.h: the kernels' side of it (block_reduce, the explicit operations)
#include <hip/hip_runtime.h>

#include <string>

dim3 threadIdx, blockIdx, gridDim, blockDim;
sim_group sim_g;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_lineest_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_lineest.hip"

#ifdef SIM_LINEEST_MAIN
#include <stdio.h>

#include <memory>

namespace {

template <class T>
std::unique_ptr<T[]> take(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "sim_lineest: short input\n"); exit(2); }
    return p;
}
template <class T>
void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "sim_lineest: short output\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sim_lineest IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const auto head = take<int64_t>(f, 3);
    const size_t n = (size_t)head[0], npix = (size_t)head[1], ngw = (size_t)head[2];
    const auto hh = take<int32_t>(f, n), ww = take<int32_t>(f, n);
    const auto gw_off = take<int64_t>(f, 3 * n);
    const auto gr = take<int32_t>(f, 3 * n);
    const auto gw = take<double>(f, ngw);
    const auto pix = take<uint8_t>(f, npix);
    fclose(f);
    std::unique_ptr<int64_t[]> pix_off(new int64_t[n]), ws_off(new int64_t[n]), col_off(new int64_t[n]);
    size_t at = 0, cols = 0;
    for (size_t k = 0; k < n; ++k) {
        pix_off[k] = (int64_t)at; ws_off[k] = 3 * (int64_t)at; col_off[k] = (int64_t)cols;
        at += (size_t)hh[k] * ww[k]; cols += ww[k];
    }
    if (at != npix) { fprintf(stderr, "sim_lineest: sizes and pixels disagree\n"); return 2; }
    std::unique_ptr<double[]> ws(new double[3 * npix]);
    std::unique_ptr<int32_t[]> arg(new int32_t[cols]), center(new int32_t[cols]), minmax(new int32_t[2 * n]),
        r(new int32_t[n]), wout(new int32_t[n]);
    if (ta_linenorm_measure(pix.get(), pix_off.get(), hh.get(), ww.get(), (int32_t)n, gw.get(), gw_off.get(), gr.get(),
                            ws.get(), ws_off.get(), arg.get(), center.get(), col_off.get(), minmax.get(), r.get(),
                            wout.get(), nullptr) != TA_OK) {
        fprintf(stderr, "sim_lineest: measure: %s\n", last_error.c_str());
        return 1;
    }
    std::unique_ptr<int64_t[]> tmp_off(new int64_t[n]), row_off(new int64_t[n]);
    size_t ntmp = 0, rows = 0;
    for (size_t k = 0; k < n; ++k) {
        if (wout[k] < 1) { fprintf(stderr, "sim_lineest: strip %zu has output width %d\n", k, wout[k]); return 1; }
        tmp_off[k] = (int64_t)ntmp; row_off[k] = (int64_t)rows;
        ntmp += (size_t)wout[k] * 48; rows += (size_t)wout[k] + 32;
    }
    std::unique_ptr<float[]> tmp(new float[ntmp]), x(new float[rows * 48]);
    std::unique_ptr<uint32_t[]> omax(new uint32_t[n]);
    if (ta_linenorm_resample(pix.get(), pix_off.get(), hh.get(), ww.get(), (int32_t)n, center.get(), col_off.get(),
                             minmax.get(), r.get(), wout.get(), tmp.get(), tmp_off.get(), omax.get(), x.get(),
                             row_off.get(), nullptr) != TA_OK) {
        fprintf(stderr, "sim_lineest: resample: %s\n", last_error.c_str());
        return 1;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    put(f, r.get(), n); put(f, wout.get(), n); put(f, arg.get(), cols); put(f, center.get(), cols);
    put(f, x.get(), rows * 48);
    if (fclose(f) != 0) { perror(argv[2]); return 2; }
    return 0;
}
#endif
