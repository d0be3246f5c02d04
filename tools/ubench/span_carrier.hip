// span_carrier.hip -- what it costs to carry an ORIGIN with every score of the carried score-only cell
// (csrc/ta_nw_span.hip).  Same method as valu_rate.hip: 8 waves per SIMD, independent copies.
// Build: hipcc -O3 --offload-arch=gfx950 span_carrier.hip -o span_carrier ; run on the GPU box.
//
// Candidates for a (score, origin) value whose maximum is lexicographic:
//   double    score * 2^28 + origin (exact: 24 + 28 bits < 53): add = v_add_f64, max = v_max_f64
//   int64     score << 32 | origin: add = v_add_co + v_addc, max = v_cmp_gt_i64 + 2 v_cndmask
// against the plain int cell (no origin).  The cell kernels run the lane step of the fill: 4 rows chained.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <stdint.h>

#define REP8(X) X X X X X X X X

template <int OP>
__global__ __launch_bounds__(512) void k(double* out, int iters, int seed) {
    double a0 = threadIdx.x + seed, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7;
    double b0 = a0 + 0.5;
    long long i0 = threadIdx.x + seed, i1 = i0 * 3, i2 = i0 * 5, i3 = i0 * 7, j0 = i0 ^ 0x55;
    for (int it = 0; it < iters; ++it) {
        if (OP == 0) { REP8(asm volatile("v_add_f64 %0, %0, %4\n v_add_f64 %1, %1, %4\n v_add_f64 %2, %2, %4\n v_add_f64 %3, %3, %4" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0));) }
        if (OP == 1) { REP8(asm volatile("v_max_f64 %0, %0, %4\n v_max_f64 %1, %1, %4\n v_max_f64 %2, %2, %4\n v_max_f64 %3, %3, %4" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0));) }
        if (OP == 2) { REP8(asm volatile("v_add_f64 %0, %0, %4\n v_max_f64 %1, %1, %4\n v_add_f64 %2, %2, %4\n v_max_f64 %3, %3, %4" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b0));) }
        if (OP == 3) { REP8(asm volatile("v_cmp_gt_i64 vcc, %0, %4\n v_cmp_gt_i64 vcc, %1, %4\n v_cmp_gt_i64 vcc, %2, %4\n v_cmp_gt_i64 vcc, %3, %4" : "+v"(i0), "+v"(i1), "+v"(i2), "+v"(i3) : "v"(j0) : "vcc");) }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + (double)(i0 + i1 + i2 + i3);
}

template <class T> __device__ __forceinline__ T vmax(T a, T b) { return a > b ? a : b; }
template <> __device__ __forceinline__ double vmax<double>(double a, double b) { return __builtin_fmax(a, b); }
template <class T> __device__ __forceinline__ T pick(bool hit, T mat, T mis) { return hit ? mat : mis; }
// the two constants of the double carrier differ in the high dword only
template <> __device__ __forceinline__ double pick<double>(bool hit, double mat, double mis) {
    return __hiloint2double(hit ? __double2hiint(mat) : __double2hiint(mis), 0);
}
template <> __device__ __forceinline__ long long pick<long long>(bool hit, long long mat, long long mis) {
    const int hi = hit ? (int)(mat >> 32) : (int)(mis >> 32);
    return (long long)(((unsigned long long)(unsigned)hi) << 32);
}

template <class T>
__global__ __launch_bounds__(512) void cellk(T* out, int iters, int seed, T cmat, T cmis, T gox, T goy) {
    constexpr int R = 4;
    T D[R], X[R], H[R];
    int tc[R];
    for (int r = 0; r < R; ++r) { D[r] = (T)(threadIdx.x + r); X[r] = (T)(seed + r); H[r] = (T)(seed - r); tc[r] = (threadIdx.x + r) & 3; }
    T dsave = (T)seed, x_up = (T)(seed + 7);
    int o = seed;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            o = (o * 5 + 1) & 3;
            T d_ul = dsave, x_u = x_up;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const T d_old = D[r];
                const T mr = d_ul + pick<T>(tc[r] == o, cmat, cmis);
                const T d = vmax(vmax(mr, x_u), H[r]);
                x_u = vmax(d + gox, x_u);
                H[r] = vmax(d + goy, H[r]);
                X[r] = x_u; D[r] = d; d_ul = d_old;
            }
            dsave = D[R - 1]; x_up = X[R - 1];
        }
    }
    T acc = dsave;
    for (int r = 0; r < R; ++r) acc += D[r] + X[r] + H[r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

static double time_ms(void (*launch)(int), int iters) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    launch(10); hipDeviceSynchronize();
    hipEventRecord(e0); launch(iters); hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    return ms;
}
static void* g_out;
constexpr int kBlocks = 256 * 4;        // 4 blocks of 512 per CU = 8 waves per SIMD
template <int OP> static void launch_op(int iters) { hipLaunchKernelGGL(k<OP>, dim3(kBlocks), dim3(512), 0, 0, (double*)g_out, iters, 1); }
template <class T> static void launch_cell(int iters) {
    hipLaunchKernelGGL(cellk<T>, dim3(kBlocks), dim3(512), 0, 0, (T*)g_out, iters, 1, (T)8, (T)-4, (T)-7, (T)-7);
}
static void launch_cell_f64(int iters) {
    const double s = 268435456.0;
    hipLaunchKernelGGL(cellk<double>, dim3(kBlocks), dim3(512), 0, 0, (double*)g_out, iters, 1, 11 * s, -1 * s, -7 * s, -7 * s);
}
static void launch_cell_i64(int iters) {
    hipLaunchKernelGGL(cellk<long long>, dim3(kBlocks), dim3(512), 0, 0, (long long*)g_out, iters, 1, 11ll << 32, -(1ll << 32),
                       -(7ll << 32), -(7ll << 32));
}

int main() {
    hipMalloc(&g_out, (size_t)kBlocks * 512 * 8);
    const int iters = 2000;
    auto op = [&](const char* name, void (*l)(int), int per_iter) {
        const double ms = time_ms(l, iters);
        const double ns = ms * 1e6 / ((double)iters * per_iter * 8.0);
        printf("%-34s %8.3f ms  %6.3f ns per wave-instr per SIMD  (= %.2f cycles @2.4GHz)\n", name, ms, ns, ns * 2.4);
    };
    op("v_add_f64", launch_op<0>, 32); op("v_max_f64", launch_op<1>, 32); op("add_f64,max_f64 alternating", launch_op<2>, 32);
    op("v_cmp_gt_i64 alone", launch_op<3>, 32);
    auto cell = [&](const char* name, void (*l)(int)) {
        const double ms = time_ms(l, 500);
        const double ns = ms * 1e6 / (500.0 * 8 * 4 * 8.0);          // cells per wave per SIMD: iters x 8 steps x 4 rows x 8 waves
        printf("%-34s %8.3f ms  %6.3f ns per wave-cell per SIMD  (= %.1f cycles @2.4GHz)\n", name, ms, ns, ns * 2.4);
        return ns;
    };
    const double ci = cell("carried cell, int (no origin)", launch_cell<int>);
    const double cd = cell("carried cell, double carrier", launch_cell_f64);
    const double cl = cell("carried cell, int64 carrier", launch_cell_i64);
    printf("ratio to the int cell: double %.2f, int64 %.2f\n", cd / ci, cl / ci);
    hipFree(g_out);
    return 0;
}
