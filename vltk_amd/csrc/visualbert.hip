// The embedding stage of the single-stream VisualBERT encoder (transformers/models/visual_bert/modeling_visual_bert.py v5.15,
// VisualBertEmbeddings.forward :72-168), the one piece of that model the LXMERT ops do not already cover: text and visual rows
// are summed, LayerNormed and written into ONE [B * (Lt + V), C] tensor by one launch, so the concatenation never exists.
//
//   text row   (b, t < Lt)   word[ids[b, t]] + token_type[tt[b, t]] + position[t]
//   visual row (b, Lt + j)   proj[b * V + j] + visual_token_type[vtt[b, j]] + visual_position[0]
//                            (+ mean over the valid a of position[align[b, j, a]]; -1 pads, a box with none adds zero)
//   then LayerNorm over the row: sums, statistics and the affine in fp32, one rounding to the storage type on the way out.
//
// One wave per row, four rows per workgroup; the text / visual branch is wave-uniform.  The kernel sets up the source rows and the
// loader that sums a chunk of them; the lane partition, the LayerNorm and the launch rule (16-byte chunks when the row length, the
// projection's stride and the bases allow, single elements otherwise) are row_norm.h's.  No LDS, no atomics.  Every table index
// is clamped into its table, so a bad id reads a wrong row, never memory outside one; refusing bad ids is the caller's job
// (vltk_amd/visualbert.py does, before the launch).
#include "row_norm.h"

namespace vk {

constexpr int VBE_MAX_ALIGN = 16;        // alignment entries per box

struct VbeArgs {
    const int64_t *ids, *tts, *vtts;     // [B, Lt], [B, Lt], [B, V]
    const int32_t *align;                // [B, V, A] or nullptr
    const void *word, *position, *token_type, *visual_token_type, *visual_position, *proj;
    const float *gamma, *beta;
    void *y;
    int A, B, Lt, V, C, ldp, vocab, type_vocab, max_position;
    float eps;
};

// VW: elements per chunk (16 / sizeof(T) on the vector path, 1 on the scalar one); C % VW == 0.
template <typename T, int VW>
__global__ __launch_bounds__(256) void visualbert_embed_kernel(const VbeArgs a) {
    const int L = a.Lt + a.V, C = a.C;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)a.B * L) return;
    const int b = (int)(row / L), r = (int)(row - (long)b * L);
    const bool text = r < a.Lt;                          // wave-uniform
    const T *pos = (const T *)a.position;

    // the three (four) source rows of this output row
    const T *s0, *s1, *s2;
    int32_t al[VBE_MAX_ALIGN];
#pragma unroll
    for (int k = 0; k < VBE_MAX_ALIGN; ++k) al[k] = -1;
    int count = 0;
    if (text) {
        const long i = (long)b * a.Lt + r;
        s0 = (const T *)a.word + clamp_row(a.ids[i], a.vocab) * C;
        s1 = (const T *)a.token_type + clamp_row(a.tts[i], a.type_vocab) * C;
        s2 = pos + (long)r * C;                          // Lt <= max_position (checked by the entry point)
    } else {
        const long j = (long)b * a.V + (r - a.Lt);
        s0 = (const T *)a.proj + j * a.ldp;
        s1 = (const T *)a.visual_token_type + clamp_row(a.vtts[j], a.type_vocab) * C;
        s2 = (const T *)a.visual_position;               // visual position id 0
        if (a.align) {
#pragma unroll
            for (int k = 0; k < VBE_MAX_ALIGN; ++k) {
                int32_t v = -1;
                if (k < a.A) v = a.align[j * a.A + k];
                if (v >= a.max_position) v = a.max_position - 1;
                al[k] = v;
                count += v >= 0;
            }
        }
    }
    const float denom = (float)(count > 0 ? count : 1);

    // by value but for the index array: captured by reference, the scalars cost the f32 chunk form two VGPRs and a wave per SIMD
    const auto load = [=, &al](int ch, float (&out)[VW]) {
        float t0[VW], t1[VW], t2[VW];
        ld_chunk<T, VW>(s0 + ch * VW, t0);
        ld_chunk<T, VW>(s1 + ch * VW, t1);
        ld_chunk<T, VW>(s2 + ch * VW, t2);
#pragma unroll
        for (int e = 0; e < VW; ++e) out[e] = t0[e] + t1[e] + t2[e];
        if (!text && count > 0) {
            float m[VW];
#pragma unroll
            for (int e = 0; e < VW; ++e) m[e] = 0.f;
#pragma unroll
            for (int k = 0; k < VBE_MAX_ALIGN; ++k)
                if (k < a.A && al[k] >= 0) {
                    float p[VW];
                    ld_chunk<T, VW>(pos + (long)al[k] * C + ch * VW, p);
#pragma unroll
                    for (int e = 0; e < VW; ++e) m[e] += p[e];
                }
#pragma unroll
            for (int e = 0; e < VW; ++e) out[e] += m[e] / denom;
        }
    };
    row_layernorm<T, VW>(C, lane, load, a.gamma, a.beta, a.eps, 1.0f, 0, (T *)a.y + row * C);
}

template <typename T>
static int vbe_launch(const VbeArgs &a, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const uintptr_t bases = (uintptr_t)a.word | (uintptr_t)a.position | (uintptr_t)a.token_type | (uintptr_t)a.visual_token_type |
                            (uintptr_t)a.visual_position | (uintptr_t)a.proj | (uintptr_t)a.y;
    const bool chunked = row_chunked(VW, a.C | a.ldp, bases);
    return row_launch(chunked ? visualbert_embed_kernel<T, VW> : visualbert_embed_kernel<T, 1>, (long)a.B * (a.Lt + a.V), s, a);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_visualbert_embed(const int64_t *input_ids, const int64_t *token_type_ids, const int64_t *visual_token_type_ids,
                        const int32_t *image_text_alignment, int A, int B, int Lt, int V, const void *word, int vocab,
                        const void *position, int max_position, const void *token_type, const void *visual_token_type, int type_vocab,
                        const void *visual_position, const void *proj, int ldp, const float *gamma, const float *beta, void *y, int C,
                        float eps, vk_dtype dt, void *stream) {
    VK_REQUIRE(input_ids && token_type_ids && visual_token_type_ids && word && position && token_type && visual_token_type &&
                   visual_position && proj && gamma && beta && y,
               VK_EINVAL, "visualbert_embed: null argument");
    VK_REQUIRE(B > 0 && Lt > 0 && V > 0 && (long)B * ((long)Lt + V) < (1L << 31), VK_EINVAL,
               "visualbert_embed: bad geometry (B=%d Lt=%d V=%d)", B, Lt, V);
    VK_REQUIRE(C > 0 && C <= ROW_MAX_C, VK_EINVAL, "visualbert_embed: C=%d must be in 1..%d", C, ROW_MAX_C);
    VK_REQUIRE(ldp >= C, VK_EINVAL, "visualbert_embed: projection row stride %d below the row length %d", ldp, C);
    VK_REQUIRE(vocab > 0 && type_vocab > 0 && max_position > 0 && Lt <= max_position, VK_EINVAL,
               "visualbert_embed: %d text tokens need max_position >= that (%d); vocab %d, type_vocab %d", Lt, max_position, vocab,
               type_vocab);
    VK_REQUIRE(image_text_alignment ? (A >= 1 && A <= VBE_MAX_ALIGN) : A == 0, VK_EINVAL,
               "visualbert_embed: A=%d alignment entries per box (1..%d with image_text_alignment, 0 without)", A, VBE_MAX_ALIGN);
    VbeArgs a;
    a.ids = input_ids, a.tts = token_type_ids, a.vtts = visual_token_type_ids, a.align = image_text_alignment;
    a.word = word, a.position = position, a.token_type = token_type, a.visual_token_type = visual_token_type;
    a.visual_position = visual_position, a.proj = proj, a.gamma = gamma, a.beta = beta, a.y = y;
    a.A = A, a.B = B, a.Lt = Lt, a.V = V, a.C = C, a.ldp = ldp, a.vocab = vocab, a.type_vocab = type_vocab, a.max_position = max_position;
    a.eps = eps;
    VK_DT_SWITCH(dt, "visualbert_embed", return vbe_launch<T>(a, (hipStream_t)stream));
}

}  // extern "C"
