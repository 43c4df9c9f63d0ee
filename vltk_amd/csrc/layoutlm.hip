// What LayoutLM (transformers/models/layoutlm/modeling_layoutlm.py v5.15) needs beyond the BERT layers: the embedding stage and the
// two inference tails the reference leaves to host loops (vltk/utils/adapters.py map_ocr_predictions) or does not have at all.
//
//   vk_layoutlm_embed     LayoutLMEmbeddings.forward :66-119 as one launch: nine table rows summed in fp32 in transformers' order
//                         word[id] + position[t] + x[x0] + y[y0] + x[x1] + y[y1] + h[y1 - y0] + w[x1 - x0] + token_type[tt],
//                         LayerNorm in fp32, one rounding to the storage type.  row_norm.h's shape: one wave per row, four rows
//                         per workgroup, a lane owns the chunks lane, lane + 64, ...; 16-byte chunks when the row length and
//                         the bases allow, single elements otherwise; the kernel is the source rows and the loader that sums
//                         them.  No LDS, no atomics.  Every index is clamped into its table (the extents at 0 too), so a bad
//                         id or box reads a wrong row, never memory outside one.
//   vk_token_word_labels  arg-max label per token, then per word the most frequent label of its tokens (ties: the smallest label).
//                         One workgroup per example; (word id, label) of every token packed into one LDS word; a thread per word
//                         first collects which labels its tokens carry (a 64-bit set), then counts label by label, ascending.
//   vk_span_select        best (start, end) pair of an extractive-QA head.  One workgroup per example; end logits and the context
//                         mask in LDS; a thread per start scans its ends upward; block reduction on (score, -s, -e).
#include "row_norm.h"

namespace vk {

// ---- vk_layoutlm_embed ------------------------------------------------------------------------------------------------------------
struct LleArgs {
    const int64_t *ids, *tts;            // [B, L]
    const int32_t *bbox;                 // [B, L, 4] (x0, y0, x1, y1)
    const void *word, *position, *x, *y, *h, *w, *token_type;
    const float *gamma, *beta;
    void *out;
    int B, L, C, vocab, max_position, max_2d, type_vocab;
    float eps;
};

// VW: elements per chunk (16 / sizeof(T) on the vector path, 1 on the scalar one); C % VW == 0.
template <typename T, int VW>
__global__ __launch_bounds__(256) void layoutlm_embed_kernel(const LleArgs a) {
    const int C = a.C;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)a.B * a.L) return;
    const int t = (int)(row % a.L);                      // L <= max_position (checked by the entry point)

    // the nine source rows of this output row, in the order they are summed
    const int32_t *bb = a.bbox + row * 4;
    const long x0 = bb[0], y0 = bb[1], x1 = bb[2], y1 = bb[3];
    const T *src[9];
    src[0] = (const T *)a.word + clamp_row(a.ids[row], a.vocab) * C;
    src[1] = (const T *)a.position + (long)t * C;
    src[2] = (const T *)a.x + clamp_row(x0, a.max_2d) * C;
    src[3] = (const T *)a.y + clamp_row(y0, a.max_2d) * C;
    src[4] = (const T *)a.x + clamp_row(x1, a.max_2d) * C;
    src[5] = (const T *)a.y + clamp_row(y1, a.max_2d) * C;
    src[6] = (const T *)a.h + clamp_row(y1 - y0, a.max_2d) * C;
    src[7] = (const T *)a.w + clamp_row(x1 - x0, a.max_2d) * C;
    src[8] = (const T *)a.token_type + clamp_row(a.tts[row], a.type_vocab) * C;

    const auto load = [&](int ch, float (&out)[VW]) {
        float p[9][VW];
#pragma unroll
        for (int k = 0; k < 9; ++k) ld_chunk<T, VW>(src[k] + ch * VW, p[k]);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            float acc = p[0][e];
#pragma unroll
            for (int k = 1; k < 9; ++k) acc += p[k][e];
            out[e] = acc;
        }
    };
    row_layernorm<T, VW>(C, lane, load, a.gamma, a.beta, a.eps, 1.0f, 0, (T *)a.out + row * C);
}

template <typename T>
static int lle_launch(const LleArgs &a, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const uintptr_t bases = (uintptr_t)a.word | (uintptr_t)a.position | (uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.h |
                            (uintptr_t)a.w | (uintptr_t)a.token_type | (uintptr_t)a.out;
    const bool chunked = row_chunked(VW, a.C, bases);
    return row_launch(chunked ? layoutlm_embed_kernel<T, VW> : layoutlm_embed_kernel<T, 1>, (long)a.B * a.L, s, a);
}

// ---- vk_token_word_labels -----------------------------------------------------------------------------------------------------------
constexpr int TWL_MAX_L = 4096, TWL_MAX_C = 64, TWL_THREADS = 256;

// One workgroup per example.  LDS word t = (word id << 8) | label of token t, or -1 for a token that belongs to no counted word.
template <typename T>
__global__ __launch_bounds__(TWL_THREADS) void token_word_labels_kernel(const T *__restrict__ logits, int ld, const int32_t *__restrict__ word_ids,
                                                                        int L, int C, int W, int32_t *__restrict__ token_labels,
                                                                        int32_t *__restrict__ word_labels) {
    __shared__ int32_t tok[TWL_MAX_L];
    const long b = blockIdx.x;
    for (int t = threadIdx.x; t < L; t += TWL_THREADS) {
        const T *r = logits + (b * L + t) * (long)ld;
        float best = -INFINITY;
        int lab = 0;
        for (int c = 0; c < C; ++c) {
            const float v = (float)r[c];
            if (v > best) best = v, lab = c;             // ties keep the lowest index; a NaN never wins
        }
        token_labels[b * L + t] = lab;
        const int32_t w = word_ids[b * L + t];
        tok[t] = (w >= 0 && w < W) ? ((w << 8) | lab) : -1;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += TWL_THREADS) {
        unsigned long long present = 0;                  // the labels this word's tokens carry
        int n = 0;
        for (int t = 0; t < L; ++t) {                    // every thread reads the same LDS word: a broadcast
            const int32_t v = tok[t];
            if (v >= 0 && (v >> 8) == w) present |= 1ull << (v & 255), ++n;      // labels are below TWL_MAX_C = 64
        }
        int label = -1, best = 0, left = n;
        while (present && left > best) {                 // ascending labels, `count > best`: ties give the smallest label
            const int c = __builtin_ctzll(present);
            present &= present - 1;
            const int32_t key = (w << 8) | c;
            int cnt = 0;
            for (int t = 0; t < L; ++t) cnt += tok[t] == key;
            if (cnt > best) best = cnt, label = c;
            left -= cnt;
        }
        word_labels[b * W + w] = label;
    }
}

// ---- vk_span_select ------------------------------------------------------------------------------------------------------------------
constexpr int SPN_MAX_L = 4096, SPN_THREADS = 256;

struct Span {
    float score;
    int s, e;
};

// the better of two candidates: the larger score, then the smaller start, then the smaller end.  A thread that found nothing holds
// (-inf, -1, -1); a found candidate's score is above -inf, so the two never tie.
__device__ __forceinline__ Span spn_better(const Span &a, const Span &b) {
    if (a.score != b.score) return a.score > b.score ? a : b;
    if (a.s != b.s) return a.s < b.s ? a : b;
    return a.e <= b.e ? a : b;
}

template <typename T>
__global__ __launch_bounds__(SPN_THREADS) void span_select_kernel(const T *__restrict__ start_logits, int lds, const T *__restrict__ end_logits,
                                                                  int lde, const int32_t *__restrict__ context, int L, int max_len,
                                                                  int32_t *__restrict__ start, int32_t *__restrict__ end,
                                                                  float *__restrict__ score) {
    __shared__ float ev[SPN_MAX_L];
    __shared__ unsigned char in_ctx[SPN_MAX_L];
    __shared__ Span part[SPN_THREADS / 64];
    const long b = blockIdx.x;
    for (int t = threadIdx.x; t < L; t += SPN_THREADS) {
        ev[t] = (float)end_logits[(b * L + t) * (long)lde];
        in_ctx[t] = context[b * L + t] != 0;
    }
    __syncthreads();
    Span best = {-INFINITY, -1, -1};
    for (int s = threadIdx.x; s < L; s += SPN_THREADS) { // ascending starts, `score > best`: ties keep the smaller start
        if (!in_ctx[s]) continue;
        const float sv = (float)start_logits[(b * L + s) * (long)lds];
        const int stop = (L - s < max_len) ? L : s + max_len;
        for (int e = s; e < stop; ++e) {
            const float sc = sv + ev[e];
            if (in_ctx[e] && sc > best.score) best.score = sc, best.s = s, best.e = e;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Span other;
        other.score = __shfl_xor(best.score, o, 64);
        other.s = __shfl_xor(best.s, o, 64);
        other.e = __shfl_xor(best.e, o, 64);
        best = spn_better(best, other);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < SPN_THREADS / 64; ++k) best = spn_better(best, part[k]);
        start[b] = best.s, end[b] = best.e, score[b] = best.score;
    }
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_layoutlm_embed(const int64_t *input_ids, const int64_t *token_type_ids, const int32_t *bbox, int B, int L, const void *word,
                      int vocab, const void *position, int max_position, const void *x, const void *y, const void *h, const void *w,
                      int max_2d, const void *token_type, int type_vocab, const float *gamma, const float *beta, void *out, int C,
                      float eps, vk_dtype dt, void *stream) {
    VK_REQUIRE(input_ids && token_type_ids && bbox && word && position && x && y && h && w && token_type && gamma && beta && out,
               VK_EINVAL, "layoutlm_embed: null argument");
    VK_REQUIRE(B > 0 && L > 0 && (long)B * (long)L < (1L << 31), VK_EINVAL, "layoutlm_embed: bad geometry (B=%d L=%d)", B, L);
    VK_REQUIRE(C > 0 && C <= ROW_MAX_C, VK_EINVAL, "layoutlm_embed: C=%d must be in 1..%d", C, ROW_MAX_C);
    VK_REQUIRE(vocab > 0 && type_vocab > 0 && max_2d > 0 && max_position > 0 && L <= max_position, VK_EINVAL,
               "layoutlm_embed: %d tokens need max_position >= that (%d); vocab %d, type_vocab %d, max_2d %d", L, max_position, vocab,
               type_vocab, max_2d);
    LleArgs a;
    a.ids = input_ids, a.tts = token_type_ids, a.bbox = bbox;
    a.word = word, a.position = position, a.x = x, a.y = y, a.h = h, a.w = w, a.token_type = token_type;
    a.gamma = gamma, a.beta = beta, a.out = out;
    a.B = B, a.L = L, a.C = C, a.vocab = vocab, a.max_position = max_position, a.max_2d = max_2d, a.type_vocab = type_vocab;
    a.eps = eps;
    VK_DT_SWITCH(dt, "layoutlm_embed", return lle_launch<T>(a, (hipStream_t)stream));
}

int vk_token_word_labels(const void *logits, int ld, const int32_t *word_ids, int B, int L, int C, int W, int32_t *token_labels,
                         int32_t *word_labels, vk_dtype dt, void *stream) {
    VK_REQUIRE(logits && word_ids && token_labels && word_labels, VK_EINVAL, "token_word_labels: null argument");
    VK_REQUIRE(B > 0 && L >= 1 && L <= TWL_MAX_L, VK_EINVAL, "token_word_labels: B=%d must be positive and L=%d in 1..%d", B, L, TWL_MAX_L);
    VK_REQUIRE(C >= 1 && C <= TWL_MAX_C && ld >= C, VK_EINVAL, "token_word_labels: C=%d must be in 1..%d and the row stride %d at least C",
               C, TWL_MAX_C, ld);
    VK_REQUIRE(W >= 1 && W <= L, VK_EINVAL, "token_word_labels: W=%d words per example must be in 1..L=%d", W, L);
    const dim3 grid((unsigned)B), block(TWL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    VK_DT_SWITCH(dt, "token_word_labels",
                 hipLaunchKernelGGL(token_word_labels_kernel<T>, grid, block, 0, s, (const T *)logits, ld, word_ids, L, C, W, token_labels,
                                    word_labels));
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_span_select(const void *start_logits, int start_stride, const void *end_logits, int end_stride, const int32_t *context_mask,
                   int B, int L, int max_answer_tokens, int32_t *start, int32_t *end, float *score, vk_dtype dt, void *stream) {
    VK_REQUIRE(start_logits && end_logits && context_mask && start && end && score, VK_EINVAL, "span_select: null argument");
    VK_REQUIRE(B > 0 && L >= 1 && L <= SPN_MAX_L, VK_EINVAL, "span_select: B=%d must be positive and L=%d in 1..%d", B, L, SPN_MAX_L);
    VK_REQUIRE(start_stride >= 1 && end_stride >= 1, VK_EINVAL, "span_select: element strides %d / %d must be positive", start_stride,
               end_stride);
    VK_REQUIRE(max_answer_tokens >= 1, VK_EINVAL, "span_select: max_answer_tokens=%d must be at least 1", max_answer_tokens);
    const dim3 grid((unsigned)B), block(SPN_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const int ml = max_answer_tokens < L ? max_answer_tokens : L;
    VK_DT_SWITCH(dt, "span_select",
                 hipLaunchKernelGGL(span_select_kernel<T>, grid, block, 0, s, (const T *)start_logits, start_stride, (const T *)end_logits,
                                    end_stride, context_mask, L, ml, start, end, score));
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
