// LayerNorm and the BERT embedding stage, for every encoder of the package (LXMERT, VisualBERT, ViT): vk_layernorm and
// vk_embed_layernorm.  Restated from transformers/models/lxmert/modeling_lxmert.py (v5.15): LxmertEmbeddings :179-214, LayerNorm
// with eps 1e-12, LxmertVisualFeatureEncoder :452-476 (its two LayerNorms are averaged: scale and accumulate).  HBM-bound; the
// statistics and the arithmetic are fp32 for every storage type.  Both kernels are a loader in front of row_layernorm (row_norm.h).
//
//   layernorm_kernel<T, VW>      y = scale * LayerNorm(x) (+ y)      one wave per row; VW = 16 / sizeof(T): 16-byte chunks, for rows
//                                whose length, strides and bases allow it; VW = 1: one element per lane and step
//   embed_layernorm_kernel<T>    LayerNorm(word[id] + position[l] + token_type[tt]), one element per lane and step
#include "row_norm.h"

namespace vk {

// x [M, C] (row stride ldx), y [M, C] (row stride ldy).
template <typename T, int VW>
__global__ __launch_bounds__(256) void layernorm_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, T *__restrict__ y, int ldy, int M, int C,
                                                       float eps, float scale, int accumulate) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const T *xr = x + (long)row * ldx;
    row_layernorm<T, VW>(C, lane, [&](int ch, float (&out)[VW]) { ld_chunk<T, VW>(xr + ch * VW, out); }, gamma, beta, eps, scale,
                         accumulate, y + (long)row * ldy);
}

// word [*, C] rows picked by ids, + pos [>= L, C] + typ [*, C] rows picked by tts; y [M, C].  The ids are the caller's to check:
// the entry carries no table sizes.  One element per chunk at every C: the chunk form has another lane partition, so other low
// bits, and is a change of its own.
template <typename T>
__global__ __launch_bounds__(256) void embed_layernorm_kernel(const T *__restrict__ word, const T *__restrict__ pos,
                                                             const T *__restrict__ typ, const int64_t *__restrict__ ids,
                                                             const int64_t *__restrict__ tts, int L, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, T *__restrict__ y, int M, int C,
                                                             float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const T *wr = word + (long)ids[row] * C, *pr = pos + (long)(row % L) * C, *tr = typ + (long)tts[row] * C;
    row_layernorm<T, 1>(C, lane, [&](int c, float (&out)[1]) { out[0] = ldf(wr + c) + ldf(pr + c) + ldf(tr + c); }, gamma, beta, eps,
                        1.0f, 0, y + (long)row * C);
}

template <typename T>
static int ln_launch(const void *x, int ldx, const float *g, const float *b, void *y, int ldy, int M, int C, float eps, float scale,
                     int accumulate, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const bool chunked = row_chunked(VW, C | ldx | ldy, (uintptr_t)x | (uintptr_t)y);
    return row_launch(chunked ? layernorm_kernel<T, VW> : layernorm_kernel<T, 1>, M, s, (const T *)x, ldx, g, b, (T *)y, ldy, M, C, eps,
                      scale, accumulate);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_layernorm(const void *x, int ldx, const float *gamma, const float *beta, void *y, int ldy, int M, int C, float eps, float scale,
                 int accumulate, vk_dtype dt, void *stream) {
    VK_REQUIRE(x && gamma && beta && y, VK_EINVAL, "layernorm: null argument");
    VK_REQUIRE(M > 0 && C > 0 && C <= ROW_MAX_C, VK_EINVAL, "layernorm: C=%d must be in 1..%d", C, ROW_MAX_C);
    VK_DT_SWITCH(dt, "layernorm", return ln_launch<T>(x, ldx, gamma, beta, y, ldy, M, C, eps, scale, accumulate, (hipStream_t)stream));
}

int vk_embed_layernorm(const int64_t *input_ids, const int64_t *token_type_ids, int B, int L, const void *word, const void *position,
                       const void *token_type, const float *gamma, const float *beta, void *y, int C, float eps, vk_dtype dt,
                       void *stream) {
    VK_REQUIRE(input_ids && token_type_ids && word && position && token_type && gamma && beta && y, VK_EINVAL, "embed: null argument");
    const int M = B * L;
    VK_REQUIRE(M > 0 && C > 0 && C <= ROW_MAX_C, VK_EINVAL, "embed: C=%d must be in 1..%d", C, ROW_MAX_C);
    VK_DT_SWITCH(dt, "embed",
                 return row_launch(embed_layernorm_kernel<T>, M, (hipStream_t)stream, (const T *)word, (const T *)position,
                                   (const T *)token_type, input_ids, token_type_ids, L, gamma, beta, (T *)y, M, C, eps));
}

}  // extern "C"
