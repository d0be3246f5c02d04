// ta_train.hip -- training of the line recogniser in float64: the state-saving forward pass,
// the CTC alignment of the outputs with the target text, and back-propagation through time.
//
// The arithmetic is ocropy 1.3.3's `SeqRecognizer.trainSequence` as restated in DESIGN.md section 14 (parity unpinned,
// like SURVEY.md Appendix B: ocropy is a third-party package the reference only calls, reference README "Training a
// New OCRopus model").  The checker of record is tests/train_ref.py.
//
// Three kernels carry the sequential parts, one workgroup per line (CTC) or per (line, direction) (LSTM):
//   train_forward_kernel   h_t from h_{t-1}: the 400 x 100 recurrent weights of a direction live in the registers of 400
//                          lanes (a row of 100 doubles each: 200 VGPRs at two waves per SIMD), h_{t-1} is broadcast from
//                          LDS; 100 lanes then apply the gates and store gi, gf, go, ci, c and h_{t-1} for BPTT
//   train_backward_kernel  the same shape with the weights TRANSPOSED in the registers (lane (gate, j) holds column j of
//                          its gate's recurrent block), so the error that flows back into h_{t-1} is four partial sums
//                          per unit, reduced through LDS
//   ctc_align_kernel       lanes over the 2 L + 1 states, the two lattice recursions over time with the running row in LDS
// The products that have no dependence between steps (input projection, output layer's error, the time-summed outer
// products) are matrix products and left to the caller (text_alignment_amd/train.py: torch, float64).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ta_common.h"

namespace {

constexpr int kNi = TA_TRAIN_NI;
constexpr int kNs = TA_TRAIN_NS;
constexpr int kNa = 1 + kNi + kNs;             // 149: bias, x, h
constexpr int kPre = 4 * kNs;                  // pre-activations of a step: gi, gf, go, ci
constexpr int kFields = TA_TRAIN_STATE_FIELDS; // gi gf go ci c h_prev
constexpr int kMaxT = TA_TRAIN_MAX_T;
constexpr int kMaxClasses = TA_TRAIN_MAX_CLASSES;
constexpr int kMaxStates = TA_CTC_MAX_STATES;
constexpr int kSeqThreads = 512;               // 8 waves, two per SIMD: 256 registers a lane
constexpr int kCtcThreads = 256;
constexpr int kOutRows = 8;                    // rows of the output layer per workgroup
constexpr int kOutThreads = 128;

__device__ __forceinline__ double sigmoid64(double x) {
    return 1.0 / (1.0 + exp(fmin(fmax(-x, -20.0), 20.0)));
}

// row of line b's step s in direction d (the reversed LSTM walks the line from its end)
__device__ __forceinline__ int64_t step_row(int64_t r0, int T, int d, int s) { return r0 + (d == 0 ? s : T - 1 - s); }

__device__ __forceinline__ bool line_ok(int T, int64_t r0, int64_t rows) {
    return T > 0 && T <= kMaxT && r0 >= 0 && r0 + T <= rows;
}

// sum_k w[k] v[k] over the 100 entries of an LDS vector (every lane reads the same address: a broadcast), four chains
__device__ __forceinline__ double dot100(const double (&w)[kNs], const double* v, double seed) {
    double a0 = seed, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int k = 0; k < kNs; k += 4) {
        a0 = fma(w[k], v[k], a0);
        a1 = fma(w[k + 1], v[k + 1], a1);
        a2 = fma(w[k + 2], v[k + 2], a2);
        a3 = fma(w[k + 3], v[k + 3], a3);
    }
    return (a0 + a1) + (a2 + a3);
}

struct SeqArgs {
    const int64_t* row_off;     // [nlines] first row of line b
    const int32_t* T;           // [nlines]
    int64_t rows;               // rows of every per-row array
    const double* W;            // [dir 2][gate 4][unit 100][149]
    const double* peep;         // [dir 2][WIP, WFP, WOP][100]
    double* states;             // [rows][dir 2][field 6][100]
    // forward
    const double* gx;           // [rows][dir 2][400]: W_gate[unit][0 .. 48] . [1; x[row]]
    double* hout;               // [rows][200]
    // backward
    const double* dy;           // [rows][200]
    double* gate_err;           // [rows][dir 2][gate 4][100]
    double* dpeep;              // [nlines][dir 2][3][100]
};

__global__ __launch_bounds__(kSeqThreads) void train_forward_kernel(SeqArgs a) {
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int T = a.T[b];
    const int64_t r0 = a.row_off[b];
    if (!line_ok(T, r0, a.rows)) return;
    __shared__ double h_s[kNs];
    __shared__ double pre_s[kPre];
    const bool mv = tid < kPre;
    double w[kNs];
    {
        const int g = mv ? tid / kNs : 0, u = mv ? tid % kNs : 0;
        const double* src = a.W + ((size_t)(d * 4 + g) * kNs + u) * kNa + 1 + kNi;
#pragma unroll
        for (int k = 0; k < kNs; ++k) w[k] = mv ? src[k] : 0.0;
    }
    const bool unit = tid < kNs;
    double wip = 0.0, wfp = 0.0, wop = 0.0, c = 0.0;
    if (unit) {
        wip = a.peep[(d * 3 + 0) * kNs + tid];
        wfp = a.peep[(d * 3 + 1) * kNs + tid];
        wop = a.peep[(d * 3 + 2) * kNs + tid];
        h_s[tid] = 0.0;
    }
    __syncthreads();
    for (int s = 0; s < T; ++s) {
        const int64_t row = step_row(r0, T, d, s);
        if (mv) pre_s[tid] = dot100(w, h_s, a.gx[(row * 2 + d) * kPre + tid]);
        __syncthreads();
        if (unit) {
            double* st = a.states + (row * 2 + d) * (kFields * kNs);
            st[5 * kNs + tid] = h_s[tid];
            double gi = pre_s[tid], gf = pre_s[kNs + tid], go = pre_s[2 * kNs + tid];
            const double ci = tanh(pre_s[3 * kNs + tid]);
            if (s > 0) {
                gi += wip * c;
                gf += wfp * c;
            }
            gi = sigmoid64(gi);
            gf = sigmoid64(gf);
            double cn = ci * gi;
            if (s > 0) {
                cn += gf * c;
                go += wop * cn;
            }
            go = sigmoid64(go);
            c = cn;
            const double h = tanh(c) * go;
            st[tid] = gi;
            st[kNs + tid] = gf;
            st[2 * kNs + tid] = go;
            st[3 * kNs + tid] = ci;
            st[4 * kNs + tid] = c;
            h_s[tid] = h;
            a.hout[row * (2 * kNs) + d * kNs + tid] = h;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSeqThreads) void train_backward_kernel(SeqArgs a) {
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int T = a.T[b];
    const int64_t r0 = a.row_off[b];
    if (!line_ok(T, r0, a.rows)) return;
    __shared__ double e_s[kPre];        // gate errors of the step: gi, gf, go, ci
    __shared__ double part_s[kPre];     // per gate, the error its recurrent block sends back into h_{t-1}
    const bool mv = tid < kPre;
    const int g = mv ? tid / kNs : 0, j = mv ? tid % kNs : 0;
    double w[kNs];                      // column j of gate g's recurrent block
    {
        const double* src = a.W + (size_t)(d * 4 + g) * kNs * kNa + 1 + kNi + j;
#pragma unroll
        for (int u = 0; u < kNs; ++u) w[u] = mv ? src[(size_t)u * kNa] : 0.0;
    }
    const bool unit = tid < kNs;
    double wip = 0.0, wfp = 0.0, wop = 0.0;
    if (unit) {
        wip = a.peep[(d * 3 + 0) * kNs + tid];
        wfp = a.peep[(d * 3 + 1) * kNs + tid];
        wop = a.peep[(d * 3 + 2) * kNs + tid];
    }
    double carry = 0.0;                 // what step s + 1 sends into this step's cell error
    double dip = 0.0, dfp = 0.0, dop = 0.0;
    for (int s = T - 1; s >= 0; --s) {
        const int64_t row = step_row(r0, T, d, s);
        if (unit) {
            double oe = a.dy[row * (2 * kNs) + d * kNs + tid];
            if (s < T - 1) oe += ((part_s[tid] + part_s[kNs + tid]) + part_s[2 * kNs + tid]) + part_s[3 * kNs + tid];
            const double* st = a.states + (row * 2 + d) * (kFields * kNs);
            const double gi = st[tid], gf = st[kNs + tid], go = st[2 * kNs + tid], ci = st[3 * kNs + tid];
            const double c = st[4 * kNs + tid];
            double cprev = 0.0;
            if (s > 0) cprev = a.states[(step_row(r0, T, d, s - 1) * 2 + d) * (kFields * kNs) + 4 * kNs + tid];
            const double tc = tanh(c);
            const double ego = go * (1.0 - go) * tc * oe;
            double ec = (1.0 - tc * tc) * go * oe;
            if (s > 0) ec += ego * wop;
            if (s < T - 1) ec += carry;
            const double egf = s > 0 ? gf * (1.0 - gf) * ec * cprev : 0.0;
            const double egi = gi * (1.0 - gi) * ec * ci;
            const double eci = (1.0 - ci * ci) * ec * gi;
            carry = egf * wfp + egi * wip + ec * gf;
            if (s > 0) {
                dip += egi * cprev;
                dfp += egf * cprev;
                dop += ego * c;
            }
            double* ge = a.gate_err + (row * 2 + d) * kPre;
            ge[tid] = egi;
            ge[kNs + tid] = egf;
            ge[2 * kNs + tid] = ego;
            ge[3 * kNs + tid] = eci;
            e_s[tid] = egi;
            e_s[kNs + tid] = egf;
            e_s[2 * kNs + tid] = ego;
            e_s[3 * kNs + tid] = eci;
        }
        __syncthreads();
        if (mv && s > 0) part_s[tid] = dot100(w, e_s + g * kNs, 0.0);
        __syncthreads();
    }
    if (unit) {
        double* dp = a.dpeep + ((size_t)b * 2 + d) * 3 * kNs;
        dp[tid] = dip;
        dp[kNs + tid] = dfp;
        dp[2 * kNs + tid] = dop;
    }
}

// probs[row] = softmax(W2 . [1; hout[row]]) with ocropy's clip of the logits to +-100
__global__ __launch_bounds__(kOutThreads) void train_output_kernel(const double* hout, int64_t rows, const double* W2,
                                                                   int no, double* probs) {
    __shared__ double y_s[kOutRows][2 * kNs];
    __shared__ double e_s[kOutRows][kMaxClasses];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kOutRows;
    const int n = (int)(rows - row0 < kOutRows ? rows - row0 : kOutRows);
    for (int i = tid; i < kOutRows * 2 * kNs; i += kOutThreads)
        y_s[i / (2 * kNs)][i % (2 * kNs)] = i < n * 2 * kNs ? hout[row0 * (2 * kNs) + i] : 0.0;
    __syncthreads();
    if (tid < no) {
        const double* wr = W2 + (size_t)tid * (1 + 2 * kNs);
        double acc[kOutRows];
#pragma unroll
        for (int i = 0; i < kOutRows; ++i) acc[i] = wr[0];
        for (int k = 0; k < 2 * kNs; ++k) {
            const double wk = wr[1 + k];
#pragma unroll
            for (int i = 0; i < kOutRows; ++i) acc[i] = fma(wk, y_s[i][k], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < kOutRows; ++i) e_s[i][tid] = exp(fmin(fmax(acc[i], -100.0), 100.0));
    }
    __syncthreads();
    if (tid < no)
        for (int i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int c = 0; c < no; ++c) sum += e_s[i][c];
            probs[(row0 + i) * no + tid] = e_s[i][tid] / sum;
        }
}

struct CtcArgs {
    const double* probs;        // [rows][no]
    const int64_t* row_off;     // [nlines]
    const int32_t* T;           // [nlines]
    const int32_t* labels;      // [nlabels] target class codes of all lines
    const int64_t* lab_off;     // [nlines] first code of line b
    const int32_t* L;           // [nlines] codes of line b
    const int64_t* ws_off;      // [nlines] line b's piece of the workspace, in doubles
    int64_t rows, nlabels, ws_doubles;
    int no;
    double* ws;
    double* aligned;            // [rows][no]
    double* deltas;             // [rows][no]
    double* err;                // [nlines] sum of deltas^2; NaN = the line was refused
};

__device__ __forceinline__ double logadd64(double x, double y) {
    return fabs(x - y) > 10.0 ? fmax(x, y) : log(exp(x - y) + 1.0) + y;
}

// deterministic block reductions through LDS (kCtcThreads is a power of two)
__device__ __forceinline__ double block_reduce(double v, double* red, bool take_max) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int k = kCtcThreads / 2; k > 0; k >>= 1) {
        if (tid < k) red[tid] = take_max ? fmax(red[tid], red[tid + k]) : red[tid] + red[tid + k];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kCtcThreads) void ctc_align_kernel(CtcArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[b], L = a.L[b], no = a.no;
    const int64_t r0 = a.row_off[b], l0 = a.lab_off[b], w0 = a.ws_off[b];
    const int S = 2 * L + 1;
    __shared__ double v_s[2][kMaxStates];
    __shared__ int lab_s[kMaxStates];
    __shared__ double red_s[kCtcThreads];
    __shared__ int bad_s;
    // every bound the kernel relies on, checked on the line's own numbers (the host checks them as well)
    const bool ok = line_ok(T, r0, a.rows) && L >= 0 && L <= (kMaxStates - 1) / 2 && S <= T && l0 >= 0 &&
                    l0 + L <= a.nlabels && w0 >= 0 && w0 + (int64_t)T * (S + no) <= a.ws_doubles;
    if (!ok) {
        if (tid == 0) a.err[b] = nan("");
        return;
    }
    if (tid == 0) bad_s = 0;
    __syncthreads();
    for (int s = tid; s < S; s += kCtcThreads) {
        const int c = (s & 1) ? a.labels[l0 + s / 2] : 0;
        if (c < 0 || c >= no) bad_s = 1;
        lab_s[s] = (c < 0 || c >= no) ? 0 : c;
        v_s[0][s] = -5.0 * s;
    }
    __syncthreads();
    if (bad_s) {
        if (tid == 0) a.err[b] = nan("");
        return;
    }
    double* both = a.ws + w0;                       // [T][S]: A, then A + B, then the normalised path weights
    double* lq = both + (size_t)T * S;              // [T][no]: log of the clamped, renormalised outputs
    const double* P = a.probs + r0 * no;
    for (int t = tid; t < T; t += kCtcThreads) {
        double sum = 0.0;
        for (int c = 0; c < no; ++c) sum += fmax(P[(size_t)t * no + c], 1e-5);
        for (int c = 0; c < no; ++c) lq[(size_t)t * no + c] = log(fmax(P[(size_t)t * no + c], 1e-5) / sum);
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        for (int s = tid; s < S; s += kCtcThreads) {
            const double x = v_s[cur][s];
            const double w = s > 0 ? v_s[cur][s - 1] : -5.0 * t;
            const double nv = logadd64(x, w) + lq[(size_t)t * no + lab_s[s]];
            v_s[cur ^ 1][s] = nv;
            both[(size_t)t * S + s] = nv;
        }
        __syncthreads();
        cur ^= 1;
    }
    // the same recursion on the match matrix reversed along both axes, added in place at the mirrored cell
    for (int s = tid; s < S; s += kCtcThreads) v_s[cur][s] = -5.0 * s;
    __syncthreads();
    double mx = -INFINITY;
    for (int tp = 0; tp < T; ++tp) {
        const int t = T - 1 - tp;
        for (int sp = tid; sp < S; sp += kCtcThreads) {
            const int s = S - 1 - sp;
            const double x = v_s[cur][sp];
            const double w = sp > 0 ? v_s[cur][sp - 1] : -5.0 * tp;
            const double nv = logadd64(x, w) + lq[(size_t)t * no + lab_s[s]];
            v_s[cur ^ 1][sp] = nv;
            const double bb = both[(size_t)t * S + s] + nv;
            both[(size_t)t * S + s] = bb;
            mx = fmax(mx, bb);
        }
        __syncthreads();
        cur ^= 1;
    }
    mx = block_reduce(mx, red_s, true);
    // E = exp(both - max), every state's column divided by its sum over time
    for (int s = tid; s < S; s += kCtcThreads) {
        double sum = 0.0;
        for (int t = 0; t < T; ++t) {
            const double e = exp(both[(size_t)t * S + s] - mx);
            both[(size_t)t * S + s] = e;
            sum += e;
        }
        const double l = sum == 0.0 ? 1e-9 : sum;
        for (int t = 0; t < T; ++t) both[(size_t)t * S + s] /= l;
    }
    __syncthreads();
    // a row per lane: states into classes in state order (the checker's order of additions), clamp, renormalise
    double esum = 0.0;
    for (int t = tid; t < T; t += kCtcThreads) {
        double* al = a.aligned + (r0 + t) * no;
        double* de = a.deltas + (r0 + t) * no;
        for (int c = 0; c < no; ++c) al[c] = 0.0;
        double blank = 0.0;
        for (int s = 0; s < S; ++s) {
            const double e = both[(size_t)t * S + s];
            const int c = lab_s[s];
            if (c == 0) blank += e;
            else al[c] += e;
        }
        al[0] = blank;
        double sum = 0.0;
        for (int c = 0; c < no; ++c) {
            const double v = fmax(al[c], 1e-5);
            al[c] = v;
            sum += v;
        }
        const double l = sum == 0.0 ? 1e-9 : sum;
        for (int c = 0; c < no; ++c) {
            const double v = al[c] / l;
            const double dl = v - P[(size_t)t * no + c];
            al[c] = v;
            de[c] = dl;
            esum += dl * dl;
        }
    }
    esum = block_reduce(esum, red_s, false);
    if (tid == 0) a.err[b] = esum;
}

int check_lines(int32_t nlines, int32_t max_T, int64_t rows) {
    if (nlines < 0 || max_T < 0 || rows < 0) return ta_fail(TA_EINVAL, "negative count");
    if (max_T > kMaxT) return ta_fail(TA_EINVAL, "a line is longer than TA_TRAIN_MAX_T timesteps");
    return TA_OK;
}

}  // namespace

extern "C" int64_t ta_ctc_workspace_bytes(int32_t T, int32_t L, int32_t no) {
    if (T <= 0 || T > kMaxT || L < 0 || L > (kMaxStates - 1) / 2 || 2 * L + 1 > T || no < 2 || no > kMaxClasses)
        return -1;
    return (int64_t)T * (2 * L + 1 + no) * (int64_t)sizeof(double);
}

extern "C" int ta_lstm_train_forward(const double* gx, const int64_t* row_off, const int32_t* T, int32_t nlines,
                                     int32_t max_T, int64_t rows, const double* W, const double* peep,
                                     const double* W2, int32_t no, double* states, double* hout, double* probs,
                                     void* stream) {
    if (int rc = check_lines(nlines, max_T, rows)) return rc;
    if (no < 2 || no > kMaxClasses) return ta_fail(TA_EINVAL, "a line model has 2 .. TA_TRAIN_MAX_CLASSES output classes");
    if (nlines == 0 || rows == 0) return TA_OK;
    if (!gx || !row_off || !T || !W || !peep || !W2 || !states || !hout || !probs)
        return ta_fail(TA_EINVAL, "null pointer argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    SeqArgs a{};
    a.row_off = row_off, a.T = T, a.rows = rows, a.W = W, a.peep = peep, a.states = states, a.gx = gx, a.hout = hout;
    hipLaunchKernelGGL(train_forward_kernel, dim3((unsigned)nlines, 2), dim3(kSeqThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "train_forward_kernel launch");
    const unsigned nblk = (unsigned)((rows + kOutRows - 1) / kOutRows);
    hipLaunchKernelGGL(train_output_kernel, dim3(nblk), dim3(kOutThreads), 0, st, hout, rows, W2, (int)no, probs);
    e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "train_output_kernel launch");
    return TA_OK;
}

extern "C" int ta_lstm_train_backward(const double* dy, const double* states, const int64_t* row_off, const int32_t* T,
                                      int32_t nlines, int32_t max_T, int64_t rows, const double* W, const double* peep,
                                      double* gate_err, double* dpeep, void* stream) {
    if (int rc = check_lines(nlines, max_T, rows)) return rc;
    if (nlines == 0 || rows == 0) return TA_OK;
    if (!dy || !states || !row_off || !T || !W || !peep || !gate_err || !dpeep)
        return ta_fail(TA_EINVAL, "null pointer argument");
    SeqArgs a{};
    a.row_off = row_off, a.T = T, a.rows = rows, a.W = W, a.peep = peep, a.states = const_cast<double*>(states);
    a.dy = dy, a.gate_err = gate_err, a.dpeep = dpeep;
    hipLaunchKernelGGL(train_backward_kernel, dim3((unsigned)nlines, 2), dim3(kSeqThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "train_backward_kernel launch");
    return TA_OK;
}

extern "C" int ta_ctc_align(const double* probs, const int64_t* row_off, const int32_t* T, const int32_t* labels,
                            const int64_t* lab_off, const int32_t* L, const int64_t* ws_off, int32_t nlines,
                            int32_t no, int64_t rows, int64_t nlabels, const int32_t* T_host, const int32_t* L_host,
                            double* workspace, int64_t workspace_bytes, double* aligned, double* deltas, double* err,
                            void* stream) {
    if (nlines < 0 || rows < 0 || nlabels < 0 || workspace_bytes < 0) return ta_fail(TA_EINVAL, "negative count");
    if (no < 2 || no > kMaxClasses) return ta_fail(TA_EINVAL, "a line model has 2 .. TA_TRAIN_MAX_CLASSES output classes");
    if (nlines == 0) return TA_OK;
    if (!T_host || !L_host) return ta_fail(TA_EINVAL, "null pointer argument");
    int64_t need = 0;
    for (int32_t b = 0; b < nlines; ++b) {
        if (T_host[b] <= 0 || T_host[b] > kMaxT) return ta_fail(TA_EINVAL, "a line has no timesteps or more than TA_TRAIN_MAX_T");
        if (L_host[b] < 0) return ta_fail(TA_EINVAL, "negative target length");
        if (2 * (int64_t)L_host[b] + 1 > T_host[b])
            return ta_fail(TA_EINVAL, "a target's 2 L + 1 states do not fit its line's timesteps");
        if (2 * L_host[b] + 1 > kMaxStates) return ta_fail(TA_EINVAL, "a target has more than TA_CTC_MAX_STATES states");
        need += ta_ctc_workspace_bytes(T_host[b], L_host[b], no);
    }
    if (workspace_bytes < need) return ta_fail(TA_EINVAL, "workspace smaller than the lines' ta_ctc_workspace_bytes");
    if (!probs || !row_off || !T || !labels || !lab_off || !L || !ws_off || !workspace || !aligned || !deltas || !err)
        return ta_fail(TA_EINVAL, "null pointer argument");
    CtcArgs a{probs, row_off, T, labels, lab_off, L, ws_off, rows, nlabels, workspace_bytes / (int64_t)sizeof(double),
              (int)no, workspace, aligned, deltas, err};
    hipLaunchKernelGGL(ctc_align_kernel, dim3((unsigned)nlines), dim3(kCtcThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ta_fail_hip(e, "ctc_align_kernel launch");
    return TA_OK;
}
