// tests/native/sim_distort.cpp -- host build of the line distortion's kernels (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_distort.hip ITSELF -- not a restatement -- against tests/native/hipshim_wg, where a
// workgroup is 256 lanes that meet at every barrier and the grid has its z dimension (the field).  The library this makes
// exports the same ta_line_distort / ta_line_distort_workspace_bytes, taking host pointers where the real ones take device
// pointers, so the column kernel's tile choice, its LDS array filled to the last element and its grid-stride sweep, the
// row kernel's tiles and halo, the strip maximum and the resampling's bounds are run against tests/distort_ref.py without
// a GPU (tests/test_distort_sim.py).  sim_distort_constants and sim_distort_col_tile hand out the source's own constants
// and its choice of the column tile, so that tests/distort_cases.py derives the branch a case is there for from them and
// not from a copy.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim_wg (no contraction: the
// explicit multiplies and adds are the plain operators here).
// With -DSIM_DISTORT_MAIN the same source is a program -- for a build with -fsanitize=address,undefined: every buffer it
// hands the kernels is a heap block of exactly the size the caller owes them.
//   sim_distort IN OUT
// IN:  int64 nlines, npix, rad; double distort, dsigma; uint64 seed; int32 hh[n], ww[n]; uint64 counters[n];
//      double gw[2 rad + 1]; uint8 pix[npix]  (strip k's pixels follow strip k - 1's)
// OUT: uint8 out[npix]; double fields[2 npix]
#define __HIPCC__ 1             // corr1d.h: the kernels' side of it (block_reduce, the explicit operations)
#include <hip/hip_runtime.h>

#include <string>

dim3 threadIdx, blockIdx, gridDim, blockDim;
sim_group sim_g;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_distort_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_distort.hip"

// the constants of ta_distort.hip, in this order (tests/distort_cases.py names them)
extern "C" int sim_distort_constants(int32_t* out, int32_t room) {
    const int32_t v[] = {kDsThreads, kDsColCells, kDsColTile, kDsRowW5, kDsRowW7, kDsRowMaxNO, kDsRowCells, kDsGridTiles,
                         TA_DISTORT_MAX_H, TA_DISTORT_MAX_RADIUS};
    const int32_t n = (int32_t)(sizeof v / sizeof v[0]);
    for (int32_t k = 0; k < n && k < room; ++k) out[k] = v[k];
    return n;
}

// the source's choice of the column tile
extern "C" int sim_distort_col_tile(int32_t h, int32_t rad) { return ds_col_tile(h, rad); }

#ifdef SIM_DISTORT_MAIN
#include <stdio.h>

#include <memory>

namespace {

template <class T>
std::unique_ptr<T[]> take(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "sim_distort: short input\n"); exit(2); }
    return p;
}
template <class T>
void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "sim_distort: short output\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sim_distort IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const auto head = take<int64_t>(f, 3);
    const size_t n = (size_t)head[0], npix = (size_t)head[1], rad = (size_t)head[2];
    const auto par = take<double>(f, 2);
    const auto seed = take<uint64_t>(f, 1);
    const auto hh = take<int32_t>(f, n), ww = take<int32_t>(f, n);
    const auto counters = take<uint64_t>(f, n);
    const auto gw = take<double>(f, 2 * rad + 1);
    const auto pix = take<uint8_t>(f, npix);
    fclose(f);
    std::unique_ptr<int64_t[]> pix_off(new int64_t[n]);
    size_t at = 0;
    for (size_t k = 0; k < n; ++k) { pix_off[k] = (int64_t)at; at += (size_t)hh[k] * ww[k]; }
    if (at != npix) { fprintf(stderr, "sim_distort: sizes and pixels disagree\n"); return 2; }
    const int64_t ws_bytes = ta_line_distort_workspace_bytes((int32_t)n, (int64_t)npix);
    if (ws_bytes < 0) { fprintf(stderr, "sim_distort: workspace size refused\n"); return 1; }
    // (filled, so that a read of what no kernel wrote would show in the output, not as an uninitialised read)
    std::unique_ptr<unsigned char[]> ws(new unsigned char[(size_t)ws_bytes]);
    memset(ws.get(), 0xA5, (size_t)ws_bytes);
    std::unique_ptr<uint8_t[]> out(new uint8_t[npix]);
    std::unique_ptr<double[]> fields(new double[2 * npix]);
    memset(out.get(), 0xA5, npix);
    memset(fields.get(), 0xFF, 2 * npix * sizeof(double));
    if (ta_line_distort(pix.get(), pix_off.get(), hh.get(), ww.get(), counters.get(), (int32_t)n, hh.get(), ww.get(),
                        par[0], par[1], seed[0], gw.get(), ws.get(), ws_bytes, out.get(), fields.get(), nullptr) != TA_OK) {
        fprintf(stderr, "sim_distort: %s\n", last_error.c_str());
        return 1;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    put(f, out.get(), npix); put(f, fields.get(), 2 * npix);
    if (fclose(f) != 0) { perror(argv[2]); return 2; }
    return 0;
}
#endif
