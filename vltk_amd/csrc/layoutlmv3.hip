// The embedding stage of LayoutLMv3 (transformers/models/layoutlmv3/modeling_layoutlmv3.py v5.15): LayoutLMv3TextEmbeddings.forward
// :160-199, LayoutLMv3Model.forward_image :603-618 and the joint part of LayoutLMv3Model.forward :729-774 as ONE launch over the
// B * (Lt + V) rows of the joint sequence, so neither the concatenation of the two parts nor an intermediate LayerNorm result exists
// in memory.  It also writes what every layer's vk_attention_relpos reads: the (pos, x, y) triple of each row and the additive mask.
//
//   text row   (b, t < Lt)   ((word[id] + type[tt]) + pos[p]) + spatial, in fp32 in that order
//                            p        RoBERTa's padding-aware position (:138-146), counted here: the wave loads ids[b, 0..t] in
//                                     64-token chunks, ballots id != pad and adds the popcounts, so no host pass over the ids
//                            spatial  x[x0] | y[y0] | x[x1] | y[y1] | h[clip(y1 - y0)] | w[clip(x1 - x0)] side by side along the
//                                     row (:112-136): a column belongs to ONE of the six tables, so a chunk is one more load, not six
//                            -> LayerNorm embeddings.LayerNorm
//   visual row (b, Lt + v)   v = 0: cls_token + pos_embed[0];  v >= 1: proj[b * Np + v - 1] + pos_embed[v]  -> LayerNorm norm
//   both                     with an image (V > 0) a second LayerNorm (LayerNorm, :766) over the first one's fp32 result, which
//                            never leaves the lane's registers; one rounding, at the store
//
// The shape is row_norm.h's: one wave per row, four rows per workgroup, a lane owns the chunks lane, lane + 64, ...; the text /
// visual branch is wave-uniform.  Vector form: 16-byte chunks, taken when coordinate_size and shape_size (hence the row) are whole
// chunks, so that a chunk never straddles two tables; scalar form: single elements, the table picked per element.  No LDS, no
// atomics.  Every table index is clamped into its table, so a bad id or box reads a wrong row, never memory outside one.
#include <cfloat>

#include "row_norm.h"

namespace vk {

struct L3eArgs {
    const int64_t *ids, *tts;            // [B, Lt]
    const int32_t *bbox, *vbox;          // [B, Lt, 4], [V, 4] (x0, y0, x1, y1)
    const float *amask;                  // [B, Lt] 1 / 0, or nullptr
    const void *word, *type, *pos, *x, *y, *h, *w, *cls, *vpos, *proj;
    const float *g_text, *b_text, *g_norm, *b_norm, *g_out, *b_out;
    void *out;                           // [B * (Lt + V), C]
    int32_t *rel;                        // [B, Lt + V, 3]
    float *mask;                         // [B, Lt + V] or nullptr
    int B, Lt, V, C, cs, ss, ldp, vocab, type_vocab, max_position, max_2d, pad;
    float eps, eps_norm;
};

// One LayerNorm of the row a wave holds in registers, in place: row_layernorm's arithmetic (mean, then the biased variance of the
// deviations, six shuffle steps each) without its load and store.
template <int VW>
__device__ __forceinline__ void l3e_norm(float (&v)[ROW_MAX_PER_LANE / VW][VW], int C, int chunks, int lane, const float *__restrict__ gamma,
                                         const float *__restrict__ beta, float eps) {
    constexpr int MAXC = ROW_MAX_PER_LANE / VW;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int e = 0; e < VW; ++e) s += v[i][e];
        }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int e = 0; e < VW; ++e) q = add_square<VW>(q, v[i][e] - mean);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = lane + 64 * i;
        if (ch < chunks) {
#pragma unroll
            for (int e = 0; e < VW; ++e) v[i][e] = (v[i][e] - mean) * rstd * gamma[ch * VW + e] + beta[ch * VW + e];
        }
    }
}

// VW: elements per chunk (16 / sizeof(T) on the vector form, 1 on the scalar one); C, cs and ss are multiples of VW.
template <typename T, int VW>
__global__ __launch_bounds__(256) void layoutlmv3_embed_kernel(const L3eArgs a) {
    constexpr int MAXC = ROW_MAX_PER_LANE / VW;
    const int L = a.Lt + a.V, C = a.C, chunks = C / VW;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)a.B * L) return;
    const int b = (int)(row / L), r = (int)(row - (long)b * L);
    const bool text = r < a.Lt;                          // wave-uniform
    float v[MAXC][VW];
    int32_t rx, ry;                                      // the coordinates the attention takes differences of: x0 and y1
    float madd = 0.f;

    if (text) {
        const long i = (long)b * a.Lt + r;
        const int64_t *idrow = a.ids + (long)b * a.Lt;
        int seen = 0;                                    // non-pad ids among ids[b, 0..r]
        for (int c0 = 0; c0 <= r; c0 += 64) {
            const int t = c0 + lane;                     // the last chunk stops at lane r % 64
            seen += __popcll(__ballot(t <= r && idrow[t] != a.pad));
        }
        const long p = idrow[r] != a.pad ? (long)a.pad + seen : a.pad;
        const int32_t *bb = a.bbox + i * 4;
        const long x0 = bb[0], y0 = bb[1], x1 = bb[2], y1 = bb[3];
        const long hh = y1 - y0, ww = x1 - x0;           // torch.clip(., 0, 1023), then into the table
        const T *s_word = (const T *)a.word + clamp_row(a.ids[i], a.vocab) * C;
        const T *s_type = (const T *)a.type + clamp_row(a.tts[i], a.type_vocab) * C;
        const T *s_pos = (const T *)a.pos + clamp_row(p, a.max_position) * C;
        const int cs = a.cs, ss = a.ss;
        const T *seg[6];                                 // the row of each of the six segments
        seg[0] = (const T *)a.x + clamp_row(x0, a.max_2d) * cs;
        seg[1] = (const T *)a.y + clamp_row(y0, a.max_2d) * cs;
        seg[2] = (const T *)a.x + clamp_row(x1, a.max_2d) * cs;
        seg[3] = (const T *)a.y + clamp_row(y1, a.max_2d) * cs;
        seg[4] = (const T *)a.h + clamp_row(clamp_row(hh, 1024), a.max_2d) * ss;
        seg[5] = (const T *)a.w + clamp_row(clamp_row(ww, 1024), a.max_2d) * ss;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            const int ch = lane + 64 * k;
            if (ch < chunks) {
                const int col = ch * VW;                 // the segment this chunk lies in, whole
                const int c4 = col - 4 * cs;
                const int sg = c4 < 0 ? col / cs : 4 + c4 / ss;
                const int off = c4 < 0 ? col - sg * cs : c4 - (sg - 4) * ss;
                const T *s_sp = sg == 0 ? seg[0] : sg == 1 ? seg[1] : sg == 2 ? seg[2] : sg == 3 ? seg[3] : sg == 4 ? seg[4] : seg[5];
                float t0[VW], t1[VW], t2[VW], t3[VW];
                ld_chunk<T, VW>(s_word + col, t0);
                ld_chunk<T, VW>(s_type + col, t1);
                ld_chunk<T, VW>(s_pos + col, t2);
                ld_chunk<T, VW>(s_sp + off, t3);
#pragma unroll
                for (int e = 0; e < VW; ++e) v[k][e] = ((t0[e] + t1[e]) + t2[e]) + t3[e];
            }
        }
        l3e_norm<VW>(v, C, chunks, lane, a.g_text, a.b_text, a.eps);
        rx = bb[0], ry = bb[3];
        if (a.amask) madd = (1.0f - a.amask[i]) * -FLT_MAX;      // bert_ops.additive_mask's value
    } else {
        const int vi = r - a.Lt;
        const T *s0 = vi == 0 ? (const T *)a.cls : (const T *)a.proj + ((long)b * (a.V - 1) + (vi - 1)) * a.ldp;
        const T *s1 = (const T *)a.vpos + (long)vi * C;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            const int ch = lane + 64 * k;
            if (ch < chunks) {
                float t0[VW], t1[VW];
                ld_chunk<T, VW>(s0 + ch * VW, t0);
                ld_chunk<T, VW>(s1 + ch * VW, t1);
#pragma unroll
                for (int e = 0; e < VW; ++e) v[k][e] = t0[e] + t1[e];
            }
        }
        l3e_norm<VW>(v, C, chunks, lane, a.g_norm, a.b_norm, a.eps_norm);
        rx = a.vbox[vi * 4], ry = a.vbox[vi * 4 + 3];
    }
    if (a.V > 0) l3e_norm<VW>(v, C, chunks, lane, a.g_out, a.b_out, a.eps);

    T *yr = (T *)a.out + row * C;
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
        const int ch = lane + 64 * k;
        if (ch < chunks) st_chunk<T, VW>(yr + ch * VW, v[k]);
    }
    if (lane == 0) {
        int32_t *rr = a.rel + row * 3;
        rr[0] = text ? r : r - a.Lt, rr[1] = rx, rr[2] = ry;     // the 1-D term is arange per part, not the RoBERTa position
        if (a.mask) a.mask[row] = madd;
    }
}

// The vector form needs whole chunks in every segment, hence in the row.
static inline bool l3e_vector_shape(int C, int cs, int ss, int vw) { return cs % vw == 0 && ss % vw == 0 && C % vw == 0; }

template <typename T>
static int l3e_launch(const L3eArgs &a, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const uintptr_t bases = (uintptr_t)a.word | (uintptr_t)a.type | (uintptr_t)a.pos | (uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.h |
                            (uintptr_t)a.w | (uintptr_t)a.cls | (uintptr_t)a.vpos | (uintptr_t)a.proj | (uintptr_t)a.out;
    const bool vec = l3e_vector_shape(a.C, a.cs, a.ss, VW) && row_chunked(VW, a.C | a.ldp, bases);
    return row_launch(vec ? layoutlmv3_embed_kernel<T, VW> : layoutlmv3_embed_kernel<T, 1>, (long)a.B * (a.Lt + a.V), s, a);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_layoutlmv3_embed_form(int C, int coordinate_size, int shape_size, vk_dtype dt, int aligned16) {
    if (dt != VK_F32 && dt != VK_F16 && dt != VK_BF16) return -VK_EINVAL;
    if (C < 1 || C > ROW_MAX_C || coordinate_size < 1 || shape_size < 1 || 4L * coordinate_size + 2L * shape_size != C) return -VK_EINVAL;
    const int vw = 16 / (int)dtype_size(dt);
    return aligned16 && l3e_vector_shape(C, coordinate_size, shape_size, vw) ? VK_L3E_FORM_VEC : VK_L3E_FORM_SCALAR;
}

int vk_layoutlmv3_embed(const int64_t *input_ids, const int64_t *token_type_ids, const int32_t *bbox, const float *attention_mask, int B,
                        int Lt, int pad_token_id, const void *word, int vocab, const void *token_type, int type_vocab,
                        const void *position, int max_position, const void *x, const void *y, const void *h, const void *w, int max_2d,
                        int coordinate_size, int shape_size, const float *text_gamma, const float *text_beta, float eps, const void *proj,
                        int ldp, const void *cls_token, const void *pos_embed, const int32_t *visual_bbox, int V, const float *norm_gamma,
                        const float *norm_beta, float norm_eps, const float *out_gamma, const float *out_beta, void *out, int32_t *rel,
                        float *mask, int C, vk_dtype dt, void *stream) {
    VK_REQUIRE(input_ids && token_type_ids && bbox && word && token_type && position && x && y && h && w && text_gamma && text_beta &&
                   out && rel,
               VK_EINVAL, "layoutlmv3_embed: null argument");
    VK_REQUIRE(B > 0 && Lt > 0 && V >= 0 && V != 1 && (long)B * ((long)Lt + V) < (1L << 31), VK_EINVAL,
               "layoutlmv3_embed: bad geometry (B=%d Lt=%d V=%d; V is 0 or 1 + patches)", B, Lt, V);
    VK_REQUIRE(C > 0 && C <= ROW_MAX_C, VK_EINVAL, "layoutlmv3_embed: C=%d must be in 1..%d", C, ROW_MAX_C);
    VK_REQUIRE(coordinate_size > 0 && shape_size > 0 && 4L * coordinate_size + 2L * shape_size == C, VK_EINVAL,
               "layoutlmv3_embed: 4 * coordinate_size (%d) + 2 * shape_size (%d) must be the row length %d", coordinate_size, shape_size, C);
    VK_REQUIRE(vocab > 0 && type_vocab > 0 && max_2d > 0 && max_position > 0 && pad_token_id >= 0 && pad_token_id < max_position, VK_EINVAL,
               "layoutlmv3_embed: vocab %d, type_vocab %d, max_2d %d, max_position %d, pad_token_id %d", vocab, type_vocab, max_2d,
               max_position, pad_token_id);
    const bool image = V > 0;
    VK_REQUIRE(image ? (proj && cls_token && pos_embed && visual_bbox && norm_gamma && norm_beta && out_gamma && out_beta && ldp >= C)
                     : (!proj && !cls_token && !pos_embed && !visual_bbox && !norm_gamma && !norm_beta && !out_gamma && !out_beta),
               VK_EINVAL, "layoutlmv3_embed: V=%d takes %s of the visual arguments (ldp=%d, C=%d)", V, image ? "all" : "none", ldp, C);
    VK_REQUIRE((mask != nullptr) == (image || attention_mask != nullptr), VK_EINVAL,
               "layoutlmv3_embed: mask is written with an attention_mask or an image, and not passed without both");
    L3eArgs a;
    a.ids = input_ids, a.tts = token_type_ids, a.bbox = bbox, a.vbox = visual_bbox, a.amask = attention_mask;
    a.word = word, a.type = token_type, a.pos = position, a.x = x, a.y = y, a.h = h, a.w = w;
    a.cls = cls_token, a.vpos = pos_embed, a.proj = proj;
    a.g_text = text_gamma, a.b_text = text_beta, a.g_norm = norm_gamma, a.b_norm = norm_beta, a.g_out = out_gamma, a.b_out = out_beta;
    a.out = out, a.rel = rel, a.mask = mask;
    a.B = B, a.Lt = Lt, a.V = V, a.C = C, a.cs = coordinate_size, a.ss = shape_size, a.ldp = image ? ldp : C;
    a.vocab = vocab, a.type_vocab = type_vocab, a.max_position = max_position, a.max_2d = max_2d, a.pad = pad_token_id;
    a.eps = eps, a.eps_norm = norm_eps;
    VK_DT_SWITCH(dt, "layoutlmv3_embed", return l3e_launch<T>(a, (hipStream_t)stream));
}

}  // extern "C"
