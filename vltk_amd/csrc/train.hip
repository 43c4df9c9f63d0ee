// What a training step of an answer head over a frozen encoder needs on gfx950 (vltk/legacy/legacy_train.py: cross-entropy on
// `question_answering_score`, AdamW, StepLR): an fp32 GEMM in the three transposition forms, column sums, the backward of
// cross-entropy, GELU / tanh and LayerNorm, and a fused AdamW step.  Everything is fp32 in memory and runs on the caller's
// stream.  No atomics and no split-K: every output has one writer and a fixed summation order, so the same input gives the
// same bits on every run.  Nothing is written outside the M x N (or n) elements an entry names.
//
//   gemm_f32_kernel<F, BK> C = op(A) . op(B) (+ bias) (+ C) on v_mfma_f32_32x32x2_f32.  256 threads = 2 x 2 waves, a wave owns
//                          F x F blocks of 32 x 32, so the tile is 64F x 64F: F = 2 (128 x 128, the shape the instruction's
//                          122 TFLOP/s figure was taken at) where such tiles fill half the CUs, F = 1 (64 x 64) elsewhere (a head's
//                          M is often 64).  K goes through LDS in steps of BK (32 at F = 1; 16 at F = 2, which keeps the kernel
//                          under 256 registers so that two workgroups share a CU and one's MFMAs run under the other's loads):
//                          each operand tile lies k-major, [BK][LD], which is what the instruction reads (lane l takes row /
//                          column l & 31 at k = l >> 5): a half-wave reads 32 consecutive words, and LD = 64F + 1 (BK = 32) or
//                          64F + 2 (BK = 16) spreads a half-wave's transposed WRITE (an operand whose memory runs along k) over
//                          the 32 banks.  The next step's global loads are issued before the MFMAs of the current one and land
//                          in LDS after them.  Edges are masked to zero at the load and skipped at the store.
//   col_sums_kernel        256 threads = 4 row lanes x 64 columns, fp64; slices of 256 rows and a second launch over the slices
//                          when M > 256
//   ce_grad_kernel         a workgroup per row: max, sum, write
//   act_kernel / act_grad_kernel     elementwise
//   ln_grad_rows_kernel    a wave per row: statistics recomputed from x, dx; ln_grad_cols_kernel: dgamma, dbeta as col_sums
//   adamw_kernel           grid (blocks, tensors) over a device table of tensors
//   scatter_rows_kernel    the backward of a row gather (after fill_zero_kernel); clip_*_kernel: clip_grad_norm_ over that table
//
// Rounding points (tests/train_util.py derives its bounds from them; u = 2^-24):
//   gemm        acc = (accumulate ? C : 0) + bias, one rounding where both are given; then per output element ONE chain
//               acc = fmaf(a_k, b_k, acc) in ascending k (the instruction is that chain; a masked k adds fmaf(0, 0, acc) = acc).
//               Integer data below 2^24 is exact.
//   col_sums    fp64 adds in the order rows q, q + 4, .. of a slice per lane q, lanes 0..3, slices ascending; one rounding to f32.
//   ce_grad     m = max (exact); a = x - m rounded; e = expf(a) (1 ulp); s = the fp64 sum of e (lane order, a fixed tree);
//               p = (float)((double)e / s); p - 1 at the label, rounded; times scale, rounded.
//   act, act_grad, ln_grad, adamw     fp64 arithmetic on the fp32 inputs (erfc, exp, cosh, sqrt of the device library: below
//               1e-15 relative), and ONE rounding to f32 at each store.  adamw forms p from the unrounded m and v.
#include "vk_common.h"

namespace vk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int COLS_SLICE = 256;        // rows per first-stage slice of a column reduction

struct GemmArgs {
    const float *A, *B, *bias;
    float *C;
    int M, N, K;
    long lda, ldb, ldc;
    int transA, transB, accumulate;
};

// One operand's 64F x BK piece of a K step, global -> registers -> LDS image [k][LD].  `kcontig`: memory runs along k (A as
// [M, K]; B as [N, K]), BK consecutive lanes then load consecutive k of one row; else along the row index (A as [K, M]; B as
// [K, N]) and a wave loads 64 consecutive rows at one k.  Element i of a thread is the same (row, k) in fetch and stash.
// LD = T + 1 at BK = 32 and T + 2 at BK = 16: a half-wave's transposed write (32 k of one row; 16 k of two rows) then covers
// 32 different banks.
// The address arithmetic is done once: a thread keeps one pointer per element and advances it by a K step.  A row outside the
// matrix is read from the last row instead and not masked: row i of op(A) reaches row i of C only, column j of op(B) column j
// only, and those are not stored.  A k outside the matrix (the last step of a K that is no multiple of BK) is read from the last
// k and cleared with a bit mask in both operands on its way into LDS, so it adds fmaf(0, 0, acc).  (Written as a select, the
// compiler puts the load under a branch and waits for it there.)
template <int T, int BK>
struct GemmTile {
    static constexpr int PER = T * BK / 256, LD = T + (BK == 32 ? 1 : 2);
    const float *p[PER];        // element i at the current step
    long kstride;               // elements between k and k + 1
    int s_off[PER], k_of[PER];  // its word of the LDS image; its k within a step

    __device__ __forceinline__ void init(const float *src, long ld, bool kcontig, int r0, int R, int tid) {
        kstride = kcontig ? 1 : ld;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int rr = kcontig ? tid / BK + (256 / BK) * i : tid % T;
            k_of[i] = kcontig ? tid % BK : tid / T + (256 / T) * i;
            s_off[i] = k_of[i] * LD + rr;
            const long gr = min(r0 + rr, R - 1);
            p[i] = kcontig ? src + gr * ld + k_of[i] : src + k_of[i] * ld + gr;
        }
    }
    // the loads of the step that starts at k0, and the pointers on to the next step
    __device__ __forceinline__ void fetch(int k0, int K, float (&r)[PER]) {
        if (k0 + BK <= K) {
#pragma unroll
            for (int i = 0; i < PER; ++i) r[i] = *p[i];
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) r[i] = p[i][(long)min(0, K - 1 - k0 - k_of[i]) * kstride];
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) p[i] += BK * kstride;
    }
    __device__ __forceinline__ void stash(float *__restrict__ s, int k0, int K, const float (&r)[PER]) const {
        if (k0 + BK <= K) {
#pragma unroll
            for (int i = 0; i < PER; ++i) s[s_off[i]] = r[i];
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) s[s_off[i]] = __uint_as_float(__float_as_uint(r[i]) & (unsigned)-(int)(k0 + k_of[i] < K));
        }
    }
};

template <int F, int BK>
__global__ __launch_bounds__(256, F) void gemm_f32_kernel(GemmArgs g) {
    constexpr int T = 64 * F, LD = GemmTile<T, BK>::LD;
    extern __shared__ float gemm_lds[];
    float *sa = gemm_lds, *sb = gemm_lds + BK * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * T, n0 = blockIdx.x * T;
    const int wm = (wave >> 1) * 32 * F, wn = (wave & 1) * 32 * F;
    const bool ka = g.transA == 0, kb = g.transB != 0;
    const int col = lane & 31, half = lane >> 5;

    // C / D of the instruction: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    f32x16 acc[F][F];
#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < F; ++j) {
            const int gc = n0 + wn + 32 * j + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gr = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = 0.0f;
                if (gr < g.M && gc < g.N) {
                    if (g.accumulate) v = g.C[(long)gr * g.ldc + gc];
                    if (g.bias) v += g.bias[gc];
                }
                acc[i][j][r] = v;
            }
        }

    GemmTile<T, BK> ta, tb;
    float ra[GemmTile<T, BK>::PER], rb[GemmTile<T, BK>::PER];
    ta.init(g.A, g.lda, ka, m0, g.M, tid);
    tb.init(g.B, g.ldb, kb, n0, g.N, tid);
    ta.fetch(0, g.K, ra);
    tb.fetch(0, g.K, rb);
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        ta.stash(sa, k0, g.K, ra);
        tb.stash(sb, k0, g.K, rb);
        __syncthreads();
        if (k0 + BK < g.K) {
            ta.fetch(k0 + BK, g.K, ra);
            tb.fetch(k0 + BK, g.K, rb);
        }
        // the step's fragments first, all of them (32 registers), then the MFMAs: one LDS latency per step, not one per pair
        float a[BK / 2][F], b[BK / 2][F];
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
#pragma unroll
            for (int i = 0; i < F; ++i) a[kk][i] = sa[(2 * kk + half) * LD + wm + 32 * i + col];
#pragma unroll
            for (int j = 0; j < F; ++j) b[kk][j] = sb[(2 * kk + half) * LD + wn + 32 * j + col];
        }
        __builtin_amdgcn_sched_barrier(0);      // or the scheduler sinks each read to just above its MFMA again
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk)
#pragma unroll
            for (int i = 0; i < F; ++i)
#pragma unroll
                for (int j = 0; j < F; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < F; ++j) {
            const int gc = n0 + wn + 32 * j + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gr = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (gr < g.M && gc < g.N) g.C[(long)gr * g.ldc + gc] = acc[i][j][r];
            }
        }
}

// ---- column sums ----------------------------------------------------------------------------------------------------------------
// Slice blockIdx.y (rows [y * rows, min(M, (y + 1) * rows))) of columns blockIdx.x * 64 ..: lane q adds rows q, q + 4, .. in fp64,
// the four lanes of a column are added in order.  part != null: the slice's sum goes to part[y][N] (fp64); else to out (f32).
__global__ __launch_bounds__(256) void col_sums_kernel(const float *__restrict__ x, long ld, int M, int N, int rows, double *__restrict__ part,
                                                       float *__restrict__ out) {
    __shared__ double s[4][64];
    const int tid = threadIdx.x, q = tid >> 6, c = blockIdx.x * 64 + (tid & 63);
    const int r1 = min(M, ((int)blockIdx.y + 1) * rows);
    double acc = 0.0;
    if (c < N)
        for (int r = blockIdx.y * rows + q; r < r1; r += 4) acc += (double)x[(long)r * ld + c];
    s[q][tid & 63] = acc;
    __syncthreads();
    if (q == 0 && c < N) {
        const double t = ((s[0][tid] + s[1][tid]) + s[2][tid]) + s[3][tid];
        if (part)
            part[(long)blockIdx.y * N + c] = t;
        else
            out[c] = (float)t;
    }
}

// out[v][c] = (float) sum over the slices, ascending, of part[v][slice][c]; v < nvec vectors share the launch (dgamma and dbeta)
__global__ __launch_bounds__(256) void col_finish_kernel(const double *__restrict__ part, int S, int N, int nvec,
                                                         float *__restrict__ out0, float *__restrict__ out1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    for (int v = 0; v < nvec; ++v) {
        double t = 0.0;
        for (int sl = 0; sl < S; ++sl) t += part[((long)v * S + sl) * N + c];
        (v == 0 ? out0 : out1)[c] = (float)t;
    }
}

// ---- cross-entropy backward ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[row, :C] = (softmax(logits[row, :C]) - onehot(label)) * scale; zeros where the label is ignore_index; NaN where it is
// neither that nor a class (nothing is read through it).
__global__ __launch_bounds__(256) void ce_grad_kernel(const float *__restrict__ logits, long ld, int C, const int64_t *__restrict__ labels,
                                                      int ignore_index, float scale, float *__restrict__ out, long ldo) {
    __shared__ float smax[4];
    __shared__ double ssum[4];
    const long row = blockIdx.x;
    const int tid = threadIdx.x;
    const long label = labels[row];
    float *o = out + row * ldo;
    if (label == (long)ignore_index || label < 0 || label >= C) {      // uniform over the workgroup
        const float v = label == (long)ignore_index ? 0.0f : __builtin_nanf("");
        for (int c = tid; c < C; c += 256) o[c] = v;
        return;
    }
    const float *x = logits + row * ld;
    float m = -INFINITY;
    for (int c = tid; c < C; c += 256) m = fmaxf(m, x[c]);
    m = wave_max(m);
    if ((tid & 63) == 0) smax[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    double s = 0.0;
    for (int c = tid; c < C; c += 256) s += (double)expf(x[c] - m);
    s = wave_sum_d(s);
    if ((tid & 63) == 0) ssum[tid >> 6] = s;
    __syncthreads();
    s = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
    for (int c = tid; c < C; c += 256) {
        float p = (float)((double)expf(x[c] - m) / s);
        if (c == label) p -= 1.0f;
        o[c] = p * scale;
    }
}

// ---- activations -------------------------------------------------------------------------------------------------------------------
// Phi(x) as erfc: 0.5 (1 + erf) would cancel on the left tail
__device__ __forceinline__ double norm_cdf(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }
__device__ __forceinline__ double act_f64(double x, int act) { return act == VK_ACT_GELU ? x * norm_cdf(x) : tanh(x); }
__device__ __forceinline__ double act_grad_f64(double x, int act) {
    if (act == VK_ACT_GELU) return norm_cdf(x) + x * exp(-0.5 * x * x) * 0.39894228040143267794;      // Phi + x phi
    const double ch = cosh(x);                                                                         // sech^2: 1 - tanh^2 would cancel
    return 1.0 / (ch * ch);
}
__global__ __launch_bounds__(256) void act_kernel(const float *__restrict__ x, float *__restrict__ y, long n, int act) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = (float)act_f64((double)x[i], act);
}
__global__ __launch_bounds__(256) void act_grad_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ dx, long n,
                                                       int act) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        dx[i] = (float)((double)dy[i] * act_grad_f64((double)x[i], act));
}

// ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
// y = gamma * xhat + beta, xhat = (x - mean) * rstd, rstd = 1 / sqrt(var + eps) (biased variance).  With g = dy * gamma:
// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)).  A wave per row; mean and rstd (fp64) are left in stats[row][2] for the
// column kernel.  A constant row has the exact mean (the fp64 sum of C equal floats is exact), so xhat = 0 and dx =
// (g - mean_c(g)) / sqrt(eps), which is what torch's backward gives in float64.
__global__ __launch_bounds__(256) void ln_grad_rows_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ gamma,
                                                           const float *__restrict__ dy, long lddy, float *__restrict__ dx, long lddx, int M,
                                                           int C, double eps, double *__restrict__ stats) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const float *xr = x + row * ldx, *dyr = dy + row * lddy;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)xr[c];
    const double mean = wave_sum_d(s) / (double)C;
    double q = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)xr[c] - mean;
        q += d * d;
    }
    const double rstd = 1.0 / sqrt(wave_sum_d(q) / (double)C + eps);
    double s1 = 0.0, s2 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double gg = (double)dyr[c] * (double)gamma[c];
        s1 += gg;
        s2 += gg * (((double)xr[c] - mean) * rstd);
    }
    s1 = wave_sum_d(s1) / (double)C;
    s2 = wave_sum_d(s2) / (double)C;
    float *dxr = dx + row * lddx;
    for (int c = lane; c < C; c += 64) {
        const double gg = (double)dyr[c] * (double)gamma[c];
        const double xh = ((double)xr[c] - mean) * rstd;
        dxr[c] = (float)(rstd * (gg - s1 - xh * s2));
    }
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
}

// dgamma[c] = sum_m dy[m, c] * xhat[m, c], dbeta[c] = sum_m dy[m, c], in col_sums_kernel's order
__global__ __launch_bounds__(256) void ln_grad_cols_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ dy, long lddy,
                                                           const double *__restrict__ stats, int M, int N, int rows, int S,
                                                           double *__restrict__ part, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double sg[4][64], sb[4][64];
    const int tid = threadIdx.x, q = tid >> 6, c = blockIdx.x * 64 + (tid & 63);
    const int r1 = min(M, ((int)blockIdx.y + 1) * rows);
    double ag = 0.0, ab = 0.0;
    if (c < N)
        for (int r = blockIdx.y * rows + q; r < r1; r += 4) {
            const double d = (double)dy[(long)r * lddy + c];
            ag += d * (((double)x[(long)r * ldx + c] - stats[2 * r]) * stats[2 * r + 1]);
            ab += d;
        }
    sg[q][tid & 63] = ag;
    sb[q][tid & 63] = ab;
    __syncthreads();
    if (q == 0 && c < N) {
        const double tg = ((sg[0][tid] + sg[1][tid]) + sg[2][tid]) + sg[3][tid];
        const double tb = ((sb[0][tid] + sb[1][tid]) + sb[2][tid]) + sb[3][tid];
        if (part) {
            part[(long)blockIdx.y * N + c] = tg;
            part[((long)S + blockIdx.y) * N + c] = tb;
        } else {
            dgamma[c] = (float)tg;
            dbeta[c] = (float)tb;
        }
    }
}

// ---- AdamW ---------------------------------------------------------------------------------------------------------------------------
// torch.optim.AdamW's rule for tensor blockIdx.y of the table, element by element:
//   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p = p (1 - lr wd) where the record decays;
//   p = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// in fp64 from the fp32 p, g, m, v; m, v and p are each rounded to f32 once, at the store, and p is formed from the unrounded
// m and v.  Scalar loads and stores: a tensor may start at any 4-byte boundary.
struct AdamwArgs {
    double step_size, beta1, beta2, eps, keep, rsqrt_bc2;      // lr / bc1; 1 - lr wd; 1 / sqrt(bc2)
};
__global__ __launch_bounds__(256) void adamw_kernel(const vk_adamw_tensor *__restrict__ table, AdamwArgs a) {
    const vk_adamw_tensor t = table[blockIdx.y];
    const double keep = t.decay ? a.keep : 1.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (long)gridDim.x * 256) {
        const double gr = (double)t.g[i];
        const double m = a.beta1 * (double)t.m[i] + (1.0 - a.beta1) * gr;
        const double v = a.beta2 * (double)t.v[i] + (1.0 - a.beta2) * gr * gr;
        const double p = (double)t.p[i] * keep - a.step_size * m / (sqrt(v) * a.rsqrt_bc2 + a.eps);
        t.m[i] = (float)m;
        t.v[i] = (float)v;
        t.p[i] = (float)p;
    }
}

// ---- a residual add: y = a + b, one rounding (y may be a or b) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_kernel(const float *a, const float *b, float *y, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = a[i] + b[i];
}

// ---- the backward of a row gather ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_zero_kernel(float *__restrict__ x, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] = 0.f;
}
// dst[idx[i]] = src[i], a workgroup per source row; the indices are distinct (the caller's contract), one outside [0, M) is skipped
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float *__restrict__ src, long lds, const int32_t *__restrict__ idx,
                                                           float *__restrict__ dst, long ldd, int M, int C) {
    const long row = idx[blockIdx.x];
    if (row < 0 || row >= M) return;
    for (int c = threadIdx.x; c < C; c += 256) dst[row * ldd + c] = src[(long)blockIdx.x * lds + c];
}

// ---- gradient clipping by global norm ------------------------------------------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_ over the AdamW table.  clip_sumsq_kernel: block x of tensor y adds the squares of elements
// x * 256 + tid, + CLIP_BLOCKS * 256, .. in fp64 per thread, then the 256 threads in a fixed tree; part[y][x].  clip_finish_kernel:
// one workgroup adds the count * CLIP_BLOCKS partial sums (thread t takes t, t + 256, ..; the same tree), norm = sqrt,
// coef = min(1, max_norm / (norm + 1e-6)) with a NaN kept, both rounded to f32 once into out[0], out[1].  clip_scale_kernel:
// g = g * coef, one rounding, coef read from device memory.
constexpr int CLIP_BLOCKS = 32;
__device__ __forceinline__ double block_sum_d(double v, double *s) {      // s[256]; the result in every thread
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    return s[0];
}
__global__ __launch_bounds__(256) void clip_sumsq_kernel(const vk_adamw_tensor *__restrict__ table, double *__restrict__ part) {
    __shared__ double s[256];
    const vk_adamw_tensor t = table[blockIdx.y];
    double acc = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (long)CLIP_BLOCKS * 256) {
        const double g = (double)t.g[i];
        acc += g * g;
    }
    acc = block_sum_d(acc, s);
    if (threadIdx.x == 0) part[(long)blockIdx.y * CLIP_BLOCKS + blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void clip_finish_kernel(const double *__restrict__ part, int n, double max_norm, float *__restrict__ out) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    acc = block_sum_d(acc, s);
    if (threadIdx.x == 0) {
        const double norm = sqrt(acc), c = max_norm / (norm + 1e-6);
        out[0] = (float)norm;
        out[1] = (float)(c < 1.0 ? c : (c != c ? c : 1.0));
    }
}
__global__ __launch_bounds__(256) void clip_scale_kernel(const vk_adamw_tensor *__restrict__ table, const float *__restrict__ norm_coef) {
    const vk_adamw_tensor t = table[blockIdx.y];
    const float coef = norm_coef[1];
    float *g = const_cast<float *>(t.g);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (long)gridDim.x * 256) g[i] = g[i] * coef;
}

static bool train_act(int act) { return act == VK_ACT_GELU || act == VK_ACT_TANH; }
static int elementwise_blocks(long n) { return (int)((n + 1023) / 1024 < 4096 ? (n + 1023) / 1024 : 4096); }
static int col_slices(int M) { return ceil_div(M, COLS_SLICE); }

}  // namespace vk

using namespace vk;

extern "C" {

int vk_gemm_f32_check(int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB) {
    return gemm_shape_check("gemm_f32", M, N, K, lda, ldb, ldc, transA, transB);
}

int vk_gemm_f32(const float *A, long lda, int transA, const float *B, long ldb, int transB, const float *bias, float *C, long ldc, int M,
                int N, int K, int accumulate, void *stream) {
    VK_REQUIRE(A && B && C, VK_EINVAL, "gemm_f32: null argument");
    VK_TRY(gemm_shape_check("gemm_f32", M, N, K, lda, ldb, ldc, transA, transB));
    VK_REQUIRE(accumulate == 0 || accumulate == 1, VK_EINVAL, "gemm_f32: accumulate=%d must be 0 or 1", accumulate);
    DeviceState *ds;
    VK_TRY(device_state(&ds));
    const GemmArgs g = {A, B, bias, C, M, N, K, lda, ldb, ldc, transA, transB, accumulate};
    const int T = large_tile(M, N, ds->n_cu) ? 128 : 64;
    VK_REQUIRE(ceil_div(M, T) <= 65535, VK_EINVAL, "gemm_f32: M=%d is beyond the grid", M);
    const dim3 grid(ceil_div(N, T), ceil_div(M, T));
    if (T == 128) {
        hipLaunchKernelGGL((gemm_f32_kernel<2, 16>), grid, dim3(256), 2 * 16 * (128 + 2) * sizeof(float), (hipStream_t)stream, g);
    } else {
        hipLaunchKernelGGL((gemm_f32_kernel<1, 32>), grid, dim3(256), 2 * 32 * (64 + 1) * sizeof(float), (hipStream_t)stream, g);
    }
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

size_t vk_col_sums_workspace_bytes(int M, int N) {
    if (M < 1 || N < 1) return 0;
    const int S = col_slices(M);
    return S > 1 ? (size_t)S * N * sizeof(double) : 0;
}

int vk_col_sums(const float *x, long ld, int M, int N, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    VK_REQUIRE(x && out, VK_EINVAL, "col_sums: null argument");
    VK_REQUIRE(M >= 1 && N >= 1 && ld >= N, VK_EINVAL, "col_sums: bad shape M=%d N=%d ld=%ld", M, N, ld);
    const int S = col_slices(M);
    VK_REQUIRE(S <= 65535, VK_EINVAL, "col_sums: M=%d is beyond the grid", M);
    const size_t need = vk_col_sums_workspace_bytes(M, N);
    VK_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0), VK_EINVAL,
               "col_sums: M=%d needs an 8-byte aligned workspace of %zu bytes, got %zu", M, need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    double *part = S > 1 ? (double *)workspace : nullptr;
    hipLaunchKernelGGL(col_sums_kernel, dim3(ceil_div(N, 64), S), dim3(256), 0, s, x, ld, M, N, COLS_SLICE, part, out);
    if (part) hipLaunchKernelGGL(col_finish_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, part, S, N, 1, out, nullptr);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_cross_entropy_grad(const float *logits, long ld, int M, int C, const int64_t *labels, int ignore_index, float scale, float *dlogits,
                          long ldd, void *stream) {
    VK_REQUIRE(logits && labels && dlogits, VK_EINVAL, "cross_entropy_grad: null argument");
    VK_REQUIRE(M >= 1 && C >= 1 && ld >= C && ldd >= C, VK_EINVAL, "cross_entropy_grad: bad shape M=%d C=%d ld=%ld ldd=%ld", M, C, ld, ldd);
    VK_REQUIRE(ignore_index < 0, VK_EINVAL, "cross_entropy_grad: ignore_index=%d must be negative (it may not name a class)", ignore_index);
    hipLaunchKernelGGL(ce_grad_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, logits, ld, C, labels, ignore_index, scale, dlogits, ldd);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_act_f32(const float *x, float *y, long n, int act, void *stream) {
    VK_REQUIRE(x && y, VK_EINVAL, "act_f32: null argument");
    VK_REQUIRE(n >= 1, VK_EINVAL, "act_f32: n=%ld must be positive", n);
    VK_REQUIRE(train_act(act), VK_EINVAL, "act_f32: activation %d is neither VK_ACT_GELU nor VK_ACT_TANH", act);
    hipLaunchKernelGGL(act_kernel, dim3(elementwise_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, y, n, act);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_act_grad_f32(const float *x, const float *dy, float *dx, long n, int act, void *stream) {
    VK_REQUIRE(x && dy && dx, VK_EINVAL, "act_grad_f32: null argument");
    VK_REQUIRE(n >= 1, VK_EINVAL, "act_grad_f32: n=%ld must be positive", n);
    VK_REQUIRE(train_act(act), VK_EINVAL, "act_grad_f32: activation %d is neither VK_ACT_GELU nor VK_ACT_TANH", act);
    hipLaunchKernelGGL(act_grad_kernel, dim3(elementwise_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n, act);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

size_t vk_layernorm_grad_workspace_bytes(int M, int C) {
    if (M < 1 || C < 1) return 0;
    const int S = col_slices(M);
    return (size_t)2 * M * sizeof(double) + (S > 1 ? (size_t)2 * S * C * sizeof(double) : 0);
}

int vk_layernorm_grad(const float *x, long ldx, const float *gamma, const float *dy, long lddy, float *dx, long lddx, float *dgamma,
                      float *dbeta, int M, int C, double eps, void *workspace, size_t workspace_bytes, void *stream) {
    VK_REQUIRE(x && gamma && dy && dx && dgamma && dbeta, VK_EINVAL, "layernorm_grad: null argument");
    VK_REQUIRE(M >= 1 && C >= 1 && ldx >= C && lddy >= C && lddx >= C, VK_EINVAL, "layernorm_grad: bad shape M=%d C=%d ldx=%ld lddy=%ld lddx=%ld",
               M, C, ldx, lddy, lddx);
    VK_REQUIRE(eps >= 0.0, VK_EINVAL, "layernorm_grad: eps must not be negative");
    const int S = col_slices(M);
    VK_REQUIRE(S <= 65535, VK_EINVAL, "layernorm_grad: M=%d is beyond the grid", M);
    const size_t need = vk_layernorm_grad_workspace_bytes(M, C);
    VK_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, VK_EINVAL,
               "layernorm_grad: needs an 8-byte aligned workspace of %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    double *stats = (double *)workspace;
    double *part = S > 1 ? stats + (size_t)2 * M : nullptr;
    hipLaunchKernelGGL(ln_grad_rows_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, s, x, ldx, gamma, dy, lddy, dx, lddx, M, C, eps, stats);
    hipLaunchKernelGGL(ln_grad_cols_kernel, dim3(ceil_div(C, 64), S), dim3(256), 0, s, x, ldx, dy, lddy, stats, M, C, COLS_SLICE, S, part,
                       dgamma, dbeta);
    if (part) hipLaunchKernelGGL(col_finish_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, part, S, C, 2, dgamma, dbeta);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_adamw_step(const vk_adamw_tensor *table, int count, int64_t max_n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double bias_correction1, double bias_correction2, void *stream) {
    VK_REQUIRE(table, VK_EINVAL, "adamw_step: null table");
    VK_REQUIRE(count >= 1 && count <= 65535 && max_n >= 1, VK_EINVAL, "adamw_step: count=%d (1..65535) max_n=%lld (>= 1)", count, (long long)max_n);
    VK_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0, VK_EINVAL,
               "adamw_step: lr, eps and weight_decay must not be negative, and the betas must lie in [0, 1)");
    VK_REQUIRE(bias_correction1 > 0.0 && bias_correction2 > 0.0, VK_EINVAL, "adamw_step: the bias corrections must be positive");
    const AdamwArgs a = {lr / bias_correction1, beta1, beta2, eps, 1.0 - lr * weight_decay, 1.0 / sqrt(bias_correction2)};
    hipLaunchKernelGGL(adamw_kernel, dim3(elementwise_blocks(max_n), count), dim3(256), 0, (hipStream_t)stream, table, a);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_add_f32(const float *a, const float *b, float *y, long n, void *stream) {
    VK_REQUIRE(a && b && y, VK_EINVAL, "add_f32: null argument");
    VK_REQUIRE(n >= 1, VK_EINVAL, "add_f32: n=%ld must be positive", n);
    hipLaunchKernelGGL(add_kernel, dim3(elementwise_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, y, n);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_scatter_rows_f32(const float *src, long ld_src, const int32_t *idx, int n, float *dst, long ld_dst, int M, int C, void *stream) {
    VK_REQUIRE(src && idx && dst, VK_EINVAL, "scatter_rows_f32: null argument");
    VK_REQUIRE(n >= 1 && M >= 1 && C >= 1 && ld_src >= C && ld_dst >= C, VK_EINVAL, "scatter_rows_f32: bad shape n=%d M=%d C=%d ld_src=%ld ld_dst=%ld",
               n, M, C, ld_src, ld_dst);
    VK_REQUIRE(ld_dst == C, VK_EINVAL, "scatter_rows_f32: dst is cleared as one block, so its rows must be dense (ld_dst=%ld, C=%d)", ld_dst, C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_zero_kernel, dim3(elementwise_blocks((long)M * C)), dim3(256), 0, s, dst, (long)M * C);
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(n), dim3(256), 0, s, src, ld_src, idx, dst, ld_dst, M, C);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

size_t vk_grad_clip_workspace_bytes(int count) { return count >= 1 ? (size_t)count * CLIP_BLOCKS * sizeof(double) : 0; }

int vk_grad_clip(const vk_adamw_tensor *table, int count, int64_t max_n, double max_norm, float *norm_coef, void *workspace,
                 size_t workspace_bytes, void *stream) {
    VK_REQUIRE(table && norm_coef, VK_EINVAL, "grad_clip: null argument");
    VK_REQUIRE(count >= 1 && count <= 65535 && max_n >= 1, VK_EINVAL, "grad_clip: count=%d (1..65535) max_n=%lld (>= 1)", count, (long long)max_n);
    VK_REQUIRE(max_norm > 0.0, VK_EINVAL, "grad_clip: max_norm must be positive");
    const size_t need = vk_grad_clip_workspace_bytes(count);
    VK_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, VK_EINVAL,
               "grad_clip: needs an 8-byte aligned workspace of %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(clip_sumsq_kernel, dim3(CLIP_BLOCKS, count), dim3(256), 0, s, table, part);
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, s, part, count * CLIP_BLOCKS, max_norm, norm_coef);
    hipLaunchKernelGGL(clip_scale_kernel, dim3(elementwise_blocks(max_n), count), dim3(256), 0, s, table, norm_coef);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
