// LayerNorm and the BERT embedding stage, for every encoder of the package (LXMERT, VisualBERT, ViT): vk_layernorm and
// vk_embed_layernorm.  Restated from transformers/models/lxmert/modeling_lxmert.py (v5.15): LxmertEmbeddings :179-214, LayerNorm
// with eps 1e-12, LxmertVisualFeatureEncoder :452-476 (its two LayerNorms are averaged: scale and accumulate).  HBM-bound; the
// statistics and the arithmetic are fp32 for every storage type.
//
//   layernorm_kernel<T, false>   y = scale * LayerNorm(x) (+ y)      one wave per row, one element per lane and step
//   layernorm_kernel<T, true>    LayerNorm(word[id] + position[l] + token_type[tt])
//   layernorm_vec_kernel         the first, on 16-byte chunks, for rows whose length and strides allow it
#include "vk_common.h"

namespace vk {

constexpr int LN_MAX_PER_LANE = 32;      // rows up to 2048 elements

// x [M, C] (row stride ldx), y [M, C] (row stride ldy).  Mean / biased variance in fp32 over the stored values,
// (x - mean) / sqrt(var + eps) * gamma + beta like at::native::layer_norm.
template <typename T, bool EMBED>
__global__ __launch_bounds__(256) void layernorm_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, T *__restrict__ y, int ldy, int M, int C,
                                                       float eps, float scale, int accumulate,
                                                       // EMBED: x = word table, rows picked by ids; + position + token type
                                                       const int64_t *__restrict__ ids, const int64_t *__restrict__ tts,
                                                       const T *__restrict__ pos, const T *__restrict__ typ, int L) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float v[LN_MAX_PER_LANE];
    const int n = (C + 63) / 64;
    float s = 0.f;
    const T *xr = EMBED ? x + (long)ids[row] * ldx : x + (long)row * ldx;
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        float t = 0.f;
        if (i < n && c < C) {
            t = ldf(xr + c);
            if (EMBED) t = t + ldf(pos + (long)(row % L) * C + c) + ldf(typ + (long)tts[row] * C + c);
        }
        v[i] = t;
        s += t;
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (i < n && c < C) {
            const float d = v[i] - mean;
            q += d * d;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (i < n && c < C) {
            float o = ((v[i] - mean) * rstd * gamma[c] + beta[c]) * scale;
            T *yp = y + (long)row * ldy + c;
            if (accumulate) o += ldf(yp);
            stf(yp, o);
        }
    }
}

// 16-byte-vector form of layernorm_kernel for rows whose length is a multiple of 8 elements (2-byte types) / 4 (f32): a lane owns
// chunks lane, lane + 64, ... of the row.  Same arithmetic.
template <typename T>
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, T *__restrict__ y, int ldy, int M, int C,
                                                           float eps, float scale, int accumulate) {
    constexpr int V = 16 / sizeof(T);
    typedef T vecT __attribute__((ext_vector_type(V)));
    constexpr int MAXC = LN_MAX_PER_LANE / V;          // chunks per lane
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int chunks = C / V;
    float v[MAXC][V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = lane + 64 * i;
        if (ch < chunks) {
            const vecT t = *reinterpret_cast<const vecT *>(x + (long)row * ldx + ch * V);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                v[i][e] = (float)t[e];
                s += v[i][e];
            }
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = lane + 64 * i;
        if (ch < chunks) {
            T *yp = y + (long)row * ldy + ch * V;
            vecT o;
            vecT old;
            if (accumulate) old = *reinterpret_cast<const vecT *>(yp);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float r = ((v[i][e] - mean) * rstd * gamma[ch * V + e] + beta[ch * V + e]) * scale;
                if (accumulate) r += (float)old[e];
                o[e] = (T)r;
            }
            *reinterpret_cast<vecT *>(yp) = o;
        }
    }
}

template <typename T>
static int ln_launch(const void *x, int ldx, const float *g, const float *b, void *y, int ldy, int M, int C, float eps, float scale,
                     int accumulate, const int64_t *ids, const int64_t *tts, const void *pos, const void *typ, int L, hipStream_t s) {
    const dim3 grid((M + 3) / 4), block(256);
    constexpr int V = 16 / sizeof(T);
    if (!ids && C % V == 0 && ldx % V == 0 && ldy % V == 0) {
        hipLaunchKernelGGL((layernorm_vec_kernel<T>), grid, block, 0, s, (const T *)x, ldx, g, b, (T *)y, ldy, M, C, eps, scale, accumulate);
        VK_CHECK_HIP(hipGetLastError());
        return VK_OK;
    }
    if (ids)
        hipLaunchKernelGGL((layernorm_kernel<T, true>), grid, block, 0, s, (const T *)x, ldx, g, b, (T *)y, ldy, M, C, eps, scale, accumulate,
                           ids, tts, (const T *)pos, (const T *)typ, L);
    else
        hipLaunchKernelGGL((layernorm_kernel<T, false>), grid, block, 0, s, (const T *)x, ldx, g, b, (T *)y, ldy, M, C, eps, scale, accumulate,
                           nullptr, nullptr, nullptr, nullptr, 1);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

static int ln_dispatch(vk_dtype dt, const void *x, int ldx, const float *g, const float *b, void *y, int ldy, int M, int C, float eps,
                       float scale, int accumulate, const int64_t *ids, const int64_t *tts, const void *pos, const void *typ, int L,
                       hipStream_t s) {
    VK_REQUIRE(M > 0 && C > 0 && C <= 64 * LN_MAX_PER_LANE, VK_EINVAL, "layernorm: C=%d must be in 1..%d", C, 64 * LN_MAX_PER_LANE);
    switch (dt) {
        case VK_F32: return ln_launch<float>(x, ldx, g, b, y, ldy, M, C, eps, scale, accumulate, ids, tts, pos, typ, L, s);
        case VK_F16: return ln_launch<_Float16>(x, ldx, g, b, y, ldy, M, C, eps, scale, accumulate, ids, tts, pos, typ, L, s);
        case VK_BF16: return ln_launch<__bf16>(x, ldx, g, b, y, ldy, M, C, eps, scale, accumulate, ids, tts, pos, typ, L, s);
        default: break;
    }
    VK_REQUIRE(false, VK_EINVAL, "layernorm: dtype must be f32, f16 or bf16");
    return VK_EINVAL;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_layernorm(const void *x, int ldx, const float *gamma, const float *beta, void *y, int ldy, int M, int C, float eps, float scale,
                 int accumulate, vk_dtype dt, void *stream) {
    VK_REQUIRE(x && gamma && beta && y, VK_EINVAL, "layernorm: null argument");
    return ln_dispatch(dt, x, ldx, gamma, beta, y, ldy, M, C, eps, scale, accumulate, nullptr, nullptr, nullptr, nullptr, 1,
                       (hipStream_t)stream);
}

int vk_embed_layernorm(const int64_t *input_ids, const int64_t *token_type_ids, int B, int L, const void *word, const void *position,
                       const void *token_type, const float *gamma, const float *beta, void *y, int C, float eps, vk_dtype dt,
                       void *stream) {
    VK_REQUIRE(input_ids && token_type_ids && word && position && token_type && gamma && beta && y, VK_EINVAL, "embed: null argument");
    return ln_dispatch(dt, word, C, gamma, beta, y, C, B * L, C, eps, 1.0f, 0, input_ids, token_type_ids, position, token_type, L,
                       (hipStream_t)stream);
}

}  // extern "C"
