// The losses of LXMERT's pre-training heads on gfx950 (transformers modeling_lxmert.py v5.15, LxmertForPreTraining.forward
// :1059-1095; the same two kernels serve LxmertForQuestionAnswering :1270-1272): per-row cross-entropy and SmoothL1, the
// reduction of the row losses to one number, and the total.  All arithmetic is fp32 on values read from the storage type,
// except the reduction's fp64 sum.  No atomics: every output has one writer and a fixed summation order, so the same input
// gives the same bits on every run.  Nothing is written behind the last row.
//
//   ce_vec_kernel<T>       one 256-thread workgroup per row; a thread reads 16-byte chunks tid, tid + 256, ... and keeps an
//                          online (max, sum of exp): every logit is read once.  VK_CE_FORM_VEC
//   ce_scalar_kernel<T>    one wave per row, one element per lane and step.  VK_CE_FORM_SCALAR: rows that are not 16-byte
//                          addressable, and rows too narrow for a workgroup to be worth it (the matched head has two columns)
//   smooth_l1_rows_kernel  one wave per row
//   loss_reduce_kernel     one workgroup: fp64 partial sums per thread in row order, a fixed tree over the threads
//
// Rounding points of a cross-entropy row (tests/lxmert_pretrain_util.py derives its bound from them): a = x - m and a * log2(e)
// are rounded once each before v_exp_f32; a running maximum that moves rescales the running sum by exp(m_old - m_new); the joins
// (six shuffle steps in a wave, then the four waves of a workgroup in order) rescale likewise; then lse = m + logf(s) and
// loss = lse - x[label], one rounding each.
#include "row_norm.h"      // ld_chunk

namespace vk {

constexpr int CE_VEC_MIN_C = 128;       // narrower rows go to the wave-per-row form

// The running (max, sum of exp(x - max)) of a row.  exp(m_old - m_new) is skipped where the maximum did not move: the factor is
// then exactly 1, and the -inf - -inf of two sides that have seen nothing finite yet never reaches rescale's exponential.  That
// covers the joins only.  An ELEMENT's own term is exp(x - m) with m = max(running, x), and a -inf logit in front of every finite
// one gives -inf - -inf there: `term` adds 0 for a -inf element (what exp(-inf - m) is for every other m, so no bit changes
// where the maximum is finite, and what torch gives).  The select looks at the element, not at m: fmaxf drops a NaN, so m can
// still be -inf when a NaN logit arrives, and that NaN must reach the exponential.  A NaN logit gives NaN, a +inf logit
// inf - inf = NaN, and a row of nothing but -inf lse = -inf and the loss -inf - -inf = NaN, all as torch.
struct OnlineLse {
    float m, s;
};
__device__ __forceinline__ float rescale(float m_old, float m_new) { return m_old == m_new ? 1.0f : __expf(m_old - m_new); }
__device__ __forceinline__ float term(float x, float m) { return x == -INFINITY ? 0.0f : __expf(x - m); }
__device__ __forceinline__ void lse_add(OnlineLse &a, float x) {
    const float m = fmaxf(a.m, x);
    a.s = a.s * rescale(a.m, m) + term(x, m);
    a.m = m;
}
__device__ __forceinline__ void lse_join(OnlineLse &a, float m2, float s2) {
    const float m = fmaxf(a.m, m2);
    a.s = a.s * rescale(a.m, m) + s2 * rescale(m2, m);
    a.m = m;
}
__device__ __forceinline__ void lse_wave(OnlineLse &a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(a.m, o, 64), s2 = __shfl_xor(a.s, o, 64);
        lse_join(a, m2, s2);
    }
}

// label -> 0: ignored, 1: a class of the row, 2: neither (the row's loss is NaN and no logit is read through it)
__device__ __forceinline__ int label_kind(long label, int ignore_index, int C) {
    return label == (long)ignore_index ? 0 : ((label >= 0 && label < C) ? 1 : 2);
}

template <typename T>
__global__ __launch_bounds__(256) void ce_vec_kernel(const T *__restrict__ logits, int ld, int C, const int64_t *__restrict__ labels,
                                                     int ignore_index, float *__restrict__ row_loss) {
    constexpr int VW = 16 / sizeof(T);
    const long row = blockIdx.x;
    const int tid = threadIdx.x;
    const long label = labels[row];
    const int kind = label_kind(label, ignore_index, C);      // uniform over the workgroup
    if (kind != 1) {
        if (tid == 0) row_loss[row] = kind == 0 ? 0.0f : __builtin_nanf("");
        return;
    }
    const T *x = logits + row * ld;
    OnlineLse a = {-INFINITY, 0.0f};
    const int chunks = C / VW;
    for (int ch = tid; ch < chunks; ch += 256) {
        float v[VW];
        ld_chunk<T, VW>(x + ch * VW, v);
        float cm = v[0];
#pragma unroll
        for (int e = 1; e < VW; ++e) cm = fmaxf(cm, v[e]);
        const float m = fmaxf(a.m, cm);
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < VW; ++e) t += term(v[e], m);
        a.s = a.s * rescale(a.m, m) + t;
        a.m = m;
    }
    if (tid < C - chunks * VW) lse_add(a, ldf(x + chunks * VW + tid));      // the columns behind the last whole chunk
    lse_wave(a);
    __shared__ float sm[4], ss[4];
    if ((tid & 63) == 0) {
        sm[tid >> 6] = a.m;
        ss[tid >> 6] = a.s;
    }
    __syncthreads();
    if (tid == 0) {
        OnlineLse r = {sm[0], ss[0]};
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_join(r, sm[w], ss[w]);
        const float lse = r.m + logf(r.s);
        row_loss[row] = lse - ldf(x + label);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_scalar_kernel(const T *__restrict__ logits, int ld, int M, int C,
                                                        const int64_t *__restrict__ labels, int ignore_index,
                                                        float *__restrict__ row_loss) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const long label = labels[row];
    const int kind = label_kind(label, ignore_index, C);      // uniform over the wave
    if (kind != 1) {
        if (lane == 0) row_loss[row] = kind == 0 ? 0.0f : __builtin_nanf("");
        return;
    }
    const T *x = logits + row * ld;
    OnlineLse a = {-INFINITY, 0.0f};
    for (int c = lane; c < C; c += 64) lse_add(a, ldf(x + c));
    lse_wave(a);
    if (lane == 0) {
        const float lse = a.m + logf(a.s);
        row_loss[row] = lse - ldf(x + label);
    }
}

// row_loss[m] = mean_c SmoothL1(pred[m, c] - target[m, c]) with beta = 1: 0.5 d^2 where |d| < 1, |d| - 0.5 elsewhere.  A lane
// sums its columns lane, lane + 64, ... in order, six shuffle steps join the lanes, one division by C.
template <typename T>
__global__ __launch_bounds__(256) void smooth_l1_rows_kernel(const T *__restrict__ pred, int ld, const float *__restrict__ target,
                                                             int ldt, int M, int C, float *__restrict__ row_loss) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const T *p = pred + row * ld;
    const float *t = target + row * ldt;
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float d = ldf(p + c) - t[c];
        const float ad = fabsf(d);
        s += ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
    }
    s = wave_sum(s);
    if (lane == 0) row_loss[row] = s / (float)C;
}

// labels given:  out = sum over the rows with label != ignore_index of row_loss / their count   (0 / 0 = NaN, as torch)
// labels null:   out = scale * sum_m row_loss[m] * weight[m] / M                                 (weight null: 1)
// Thread t adds rows t, t + 256, ... in fp64 (the product of two floats is exact there), then a tree over the 256 threads.
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float *__restrict__ row_loss, const float *__restrict__ weight,
                                                          const int64_t *__restrict__ labels, int ignore_index, int M, float scale,
                                                          float *__restrict__ out) {
    __shared__ double sum[256];
    __shared__ int cnt[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    int n = 0;
    for (int m = tid; m < M; m += 256) {
        if (labels) {
            if (labels[m] != (int64_t)ignore_index) {
                acc += (double)row_loss[m];
                ++n;
            }
        } else {
            acc += (double)row_loss[m] * (weight ? (double)weight[m] : 1.0);
        }
    }
    sum[tid] = acc;
    cnt[tid] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sum[tid] += sum[tid + o];
            cnt[tid] += cnt[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) *out = labels ? (float)(sum[0] / (double)cnt[0]) : (float)((double)scale * sum[0] / (double)M);
}

// terms [6]: masked-LM, matched, obj, attr, feat, answer; bit i of `present` says that term i takes part.  fp32 adds in
// transformers' order (:1059-1095): total = 0, += mlm, += matched, += (0 + obj + attr + feat), += answer.
__global__ void loss_total_kernel(const float *__restrict__ terms, int present, float *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float total = 0.0f;
    if (present & 1) total += terms[0];
    if (present & 2) total += terms[1];
    if (present & 0x1c) {
        float visual = 0.0f;
        for (int i = 2; i < 5; ++i)
            if (present & (1 << i)) visual += terms[i];
        total += visual;
    }
    if (present & 0x20) total += terms[5];
    *out = total;
}

static bool float_dt(vk_dtype dt) { return dt == VK_F32 || dt == VK_F16 || dt == VK_BF16; }

static int ce_form(int C, int ld, vk_dtype dt, bool aligned16) {
    const int vw = 16 / (int)dtype_size(dt);
    return (aligned16 && ld % vw == 0 && C >= CE_VEC_MIN_C) ? VK_CE_FORM_VEC : VK_CE_FORM_SCALAR;
}

template <typename T>
static void ce_launch(int form, const void *logits, int ld, int M, int C, const int64_t *labels, int ignore_index, float *row_loss,
                      hipStream_t s) {
    if (form == VK_CE_FORM_VEC)
        hipLaunchKernelGGL((ce_vec_kernel<T>), dim3(M), dim3(256), 0, s, (const T *)logits, ld, C, labels, ignore_index, row_loss);
    else
        hipLaunchKernelGGL((ce_scalar_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, s, (const T *)logits, ld, M, C, labels, ignore_index,
                           row_loss);
}

template <typename T>
static void sl1_launch(const void *pred, int ld, const float *target, int ldt, int M, int C, float *row_loss, hipStream_t s) {
    hipLaunchKernelGGL((smooth_l1_rows_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, s, (const T *)pred, ld, target, ldt, M, C, row_loss);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_cross_entropy_form(int C, int ld, vk_dtype dt, int aligned16) {
    if (!float_dt(dt) || C < 1 || ld < C) return -VK_EINVAL;
    return ce_form(C, ld, dt, aligned16 != 0);
}

int vk_cross_entropy(const void *logits, int ld, int M, int C, const int64_t *labels, int ignore_index, float *row_loss, vk_dtype dt,
                     void *stream) {
    VK_REQUIRE(logits && labels && row_loss, VK_EINVAL, "cross_entropy: null argument");
    VK_REQUIRE(float_dt(dt), VK_EINVAL, "cross_entropy: dtype must be f32, f16 or bf16");      // ce_form divides by the dtype's size
    VK_REQUIRE(M >= 1 && C >= 1 && ld >= C, VK_EINVAL, "cross_entropy: bad shape M=%d C=%d ld=%d", M, C, ld);
    VK_REQUIRE(ignore_index < 0, VK_EINVAL, "cross_entropy: ignore_index=%d must be negative (it may not name a class)", ignore_index);
    const int form = ce_form(C, ld, dt, ((uintptr_t)logits & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    VK_DT_SWITCH(dt, "cross_entropy", ce_launch<T>(form, logits, ld, M, C, labels, ignore_index, row_loss, s));
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_smooth_l1_rows(const void *pred, int ld, const float *target, int ldt, int M, int C, float *row_loss, vk_dtype dt, void *stream) {
    VK_REQUIRE(pred && target && row_loss, VK_EINVAL, "smooth_l1_rows: null argument");
    VK_REQUIRE(M >= 1 && C >= 1 && ld >= C && ldt >= C, VK_EINVAL, "smooth_l1_rows: bad shape M=%d C=%d ld=%d ldt=%d", M, C, ld, ldt);
    hipStream_t s = (hipStream_t)stream;
    VK_DT_SWITCH(dt, "smooth_l1_rows", sl1_launch<T>(pred, ld, target, ldt, M, C, row_loss, s));
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_loss_reduce(const float *row_loss, const float *weight, const int64_t *labels, int ignore_index, int M, float scale, float *out,
                   void *stream) {
    VK_REQUIRE(row_loss && out, VK_EINVAL, "loss_reduce: null argument");
    VK_REQUIRE(M >= 1, VK_EINVAL, "loss_reduce: M=%d must be positive", M);
    VK_REQUIRE(!(labels && weight), VK_EINVAL, "loss_reduce: labels (the mean over the counted rows) or weight, not both");
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_loss, weight, labels, ignore_index, M, scale, out);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_loss_total(const float *terms, int present, float *out, void *stream) {
    VK_REQUIRE(terms && out, VK_EINVAL, "loss_total: null argument");
    VK_REQUIRE(present >= 0 && present < 64, VK_EINVAL, "loss_total: present=%d must be a mask of the six terms", present);
    hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, terms, present, out);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
