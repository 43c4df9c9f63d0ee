// vk_attention_relpos: attention whose scores carry LayoutLMv3's relative-position bias, formed inside the kernel (DESIGN.md
// section 34).  Restated from transformers/models/layoutlmv3/modeling_layoutlmv3.py (v5.15): LayoutLMv3Encoder._cal_1d_pos_emb /
// _cal_2d_pos_emb and LayoutLMv3SelfAttention.forward.
//
//   O = softmax((Q K^T + bias) / sqrt(d) + mask) V                                    per (batch, head)
//   bias[b, h, i, j] = T1[h][c1(pk[b, j] - pq[b, i])] + (TX[h][c2(xk[b, j] - xq[b, i])] + TY[h][c2(yk[b, j] - yq[b, i])])
//   c_r(t) = clamp(t, -r, r) + r
//
// transformers gathers the bias into [B, heads, L, L] and every layer reads it; here a pair's bias is three reads of the head's
// table in LDS, indexed by differences of integers the lanes hold.  The host folds distance -> bucket -> weight into the table
// once per model (vltk_amd/layoutlmv3.py relpos_lut): relative_position_bucket is constant from max_distance on, so a table over
// the clamped difference is exact and no kernel takes a logarithm.  A score is (dot + (t1 + (tx + ty))) * scale + mask in fp32
// (rp_score of relpos.h).
//
//   attention_relpos_kernel         bf16 / f16, head dim 32 / 64, 16-byte aligned rows: v_mfma_f32_16x16x32, 64-key tiles, online
//                                   soft-max, P rounded to the storage type for the second product (attention_tiled_kernel's
//                                   arithmetic), with a work split of its own (below).  Like that kernel it keeps its body written
//                                   out: a boundary rule changed in attention_mma.h has to be changed here too
//   attention_stream_kernel, BIAS   every type, head dim <= 256, any alignment: the strict form, attention_stream.h's kernel with
//                                   the bias switched on: fp32 FMAs over LDS tiles, P not rounded
//
// No atomics: the same input gives the same bits.
#include <algorithm>

#include "attention_stream.h"
#include "attention_tiled.h"

namespace vk {

// ---- the matrix-core form ----
// A WORKGROUP of 1 .. 4 waves per (batch, head, run of waves * QB * 16 queries): wave w serves the w-th block of QB * 16 queries
// of the run, so what a workgroup shares is shared by one head:
//   * the head's table, loaded into LDS once;
//   * a tile's 64 key triples (pos, x, y), staged once per tile;
//   * the tile's V^T image, built once by all waves together (attention_tiled_kernel: every wave builds its own).
// Both are double-buffered: the image of tile t + 1 is built after tile t's P is written, into the other buffer, so a tile costs
// two barriers as in the tiled kernel (the V^T image of tile t, then P of tile t, before anybody reads them).  Each wave keeps its
// own P image; K fragments come straight from memory.  Lane layouts are attention_tiled_kernel's: a lane holds S[q = 4 g + e][key
// = 16 kb + j], keeps the 4 QB triples of its query rows in registers for the whole kernel, reads its four key triples per tile,
// and forms each index with a subtract and a clamp: three LDS reads per score element.  A wave whose block lies past Lq computes
// on zero queries and stores nothing: the barriers stay uniform.
// LDS: V^T [2][D][72] T | P [waves][QB * 16][72] T | key triples [2][3][64] int | table.
template <typename T, int D, int QB>
__global__ __launch_bounds__(256) void attention_relpos_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                              const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                              const int32_t *__restrict__ rel_q, const int32_t *__restrict__ rel_k,
                                                              const float *__restrict__ lut, int r1, int r2, T *__restrict__ out, int ldo,
                                                              int heads, int Lq, int Lk, int nrun, float scale) {
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = ATT_KT / 16, CH = D / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
    const int bh = blockIdx.x / nrun, run = blockIdx.x - bh * nrun;
    const int b = bh / heads, h = bh - b * heads;
    const int q0 = (run * nw + wave) * (QB * 16);
    const int n1 = 2 * r1 + 1, n2 = 2 * r2 + 1, nlut = n1 + 2 * n2;
    T *vt0 = reinterpret_cast<T *>(rp_lds), *pt = vt0 + 2 * D * ATT_PP + wave * (QB * 16 * ATT_PP);
    int *kr0 = reinterpret_cast<int *>(vt0 + 2 * D * ATT_PP + nw * (QB * 16 * ATT_PP));
    float *t1s = reinterpret_cast<float *>(kr0 + 2 * 3 * ATT_KT), *txs = t1s + n1, *tys = txs + n2;
    const frag zf = {};

    for (int i = tid; i < nlut; i += nthr) t1s[i] = lut[(long)h * nlut + i];

    // the V^T image and the key triples of the tile at k0 -> buffer buf; lane = (key pair, 16-byte chunk of a V row): 32-bit LDS
    // writes, consecutive lanes on consecutive words.  Padded keys carry V = 0 and the triple (0, 0, 0).
    auto stage = [&](int k0, int buf) {
        unsigned *vt32 = reinterpret_cast<unsigned *>(vt0 + buf * (D * ATT_PP));
        for (int i = tid; i < 32 * CH; i += nthr) {
            const int kp = i & 31, c = i >> 5, key = k0 + 2 * kp;
            frag t0 = zf, t1 = zf;
            if (key < Lk) t0 = *reinterpret_cast<const frag *>(v + ((long)b * Lk + key) * ldv + h * D + c * 8);
            if (key + 1 < Lk) t1 = *reinterpret_cast<const frag *>(v + ((long)b * Lk + key + 1) * ldv + h * D + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                vt32[((c * 8 + e) * ATT_PP) / 2 + kp] = pack16<T>(t0[e], t1[e]);
            }
        }
        if (tid < ATT_KT) {
            const int key = k0 + tid;
            const bool ok = key < Lk;
            const int32_t *src = rel_k + ((long)b * Lk + (ok ? key : 0)) * 3;
            int *kr = kr0 + buf * (3 * ATT_KT);
            kr[tid] = ok ? src[0] : 0;
            kr[ATT_KT + tid] = ok ? src[1] : 0;
            kr[2 * ATT_KT + tid] = ok ? src[2] : 0;
        }
    };

    frag qf[QB][KD];
    int qp[QB][4], qx[QB][4], qy[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int r = q0 + qb * 16 + j;
        const bool ok = r < Lq;
        const T *src = q + ((long)b * Lq + (ok ? r : 0)) * ldq + h * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KD; ++ks) {
            const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
            qf[qb][ks] = ok ? t : zf;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = q0 + qb * 16 + g * 4 + e;
            const bool rok = row < Lq;
            const int32_t *rs = rel_q + ((long)b * Lq + (rok ? row : 0)) * 3;
            qp[qb][e] = rok ? rs[0] : 0;
            qx[qb][e] = rok ? rs[1] : 0;
            qy[qb][e] = rok ? rs[2] : 0;
        }
    }
    m16_f4 o[QB][NDB];
    float m[QB][4], l[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[qb][db] = m16_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[qb][e] = -INFINITY;
            l[qb][e] = 0.f;
        }
    }

    stage(0, 0);
    int buf = 0;
    for (int k0 = 0; k0 < Lk; k0 += ATT_KT, buf ^= 1) {
        // ---- K fragments straight from memory ----
        frag kf[KB][KD];
        float mk[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int r = k0 + kb * 16 + j;
            const bool ok = r < Lk;
            const T *src = k + ((long)b * Lk + (ok ? r : 0)) * ldk + h * D + g * 8;
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) {
                const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
                kf[kb][ks] = ok ? t : zf;
            }
            mk[kb] = ok ? (mask ? mask[(long)b * Lk + r] : 0.f) : -INFINITY;
        }
        __syncthreads();            // this tile's V^T image and key triples (first tile: the table too) are in LDS
        const int *kr = kr0 + buf * (3 * ATT_KT);
        const T *vt = vt0 + buf * (D * ATT_PP);
        int kp[KB], kx[KB], ky[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            kp[kb] = kr[kb * 16 + j];
            kx[kb] = kr[ATT_KT + kb * 16 + j];
            ky[kb] = kr[2 * ATT_KT + kb * 16 + j];
        }
        // ---- S = (Q K^T + bias) * scale + mask; online soft-max; P image ----
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            m16_f4 sc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                m16_f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = Mma16<T>::mma(qf[qb][ks], kf[kb][ks], a);
                const bool ok = k0 + kb * 16 + j < Lk;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t1 = t1s[rp_idx(kp[kb], qp[qb][e], r1)];
                    const float tx = txs[rp_idx(kx[kb], qx[qb][e], r2)];
                    const float ty = tys[rp_idx(ky[kb], qy[qb][e], r2)];
                    a[e] = ok ? rp_score(a[e], t1, tx, ty, scale, mk[kb]) : -INFINITY;
                }
                sc[kb] = a;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float mx = sc[0][e];
#pragma unroll
                for (int kb = 1; kb < KB; ++kb) mx = fmaxf(mx, sc[kb][e]);
#pragma unroll
                for (int s = 8; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
                const float mn = fmaxf(m[qb][e], mx);
                const float alpha = att_exp(m[qb][e] - mn);      // first tile: exp(-inf) = 0
                float sum = 0.f;
                const int row = qb * 16 + g * 4 + e;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const float p = att_exp(sc[kb][e] - mn);     // padded keys: exp(-inf) = 0
                    sum += p;
                    pt[row * ATT_PP + kb * 16 + j] = (T)p;
                }
#pragma unroll
                for (int s = 8; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
                m[qb][e] = mn;
                l[qb][e] = alpha * l[qb][e] + sum;
#pragma unroll
                for (int db = 0; db < NDB; ++db) o[qb][db][e] *= alpha;
            }
        }
        __syncthreads();            // P is written; every wave is past the previous tile's second product, whose buffer is free
        if (k0 + ATT_KT < Lk) stage(k0 + ATT_KT, buf ^ 1);
        // ---- O += P V: A = P rows (keys contiguous), B = V^T rows (keys contiguous) ----
        const int nk2 = Lk - k0 > 32 ? 2 : 1;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            if (k2 >= nk2) continue;
            frag pf[QB];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) pf[qb] = *reinterpret_cast<const frag *>(pt + (qb * 16 + j) * ATT_PP + k2 * 32 + g * 8);
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const frag vf = *reinterpret_cast<const frag *>(vt + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) o[qb][db] = Mma16<T>::mma(pf[qb], vf, o[qb][db]);
            }
        }
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = q0 + qb * 16 + g * 4 + e;
            if (row >= Lq) continue;
#pragma unroll
            for (int db = 0; db < NDB; ++db) out[((long)b * Lq + row) * ldo + h * D + db * 16 + j] = (T)(o[qb][db][e] / l[qb][e]);
        }
}

// ---- the rule (host only) ----
static int relpos_form(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16) {
    if (!(Lq >= 1 && Lk >= 1 && d >= 1)) {
        set_error("attention_relpos: bad geometry (Lq=%d Lk=%d d=%d)", Lq, Lk, d);
        return -VK_EINVAL;
    }
    if (!(dt == VK_F32 || dt == VK_F16 || dt == VK_BF16)) {
        set_error("attention_relpos: dtype must be f32, f16 or bf16");
        return -VK_EINVAL;
    }
    if (!env_off("VK_ATTENTION_MFMA") && (dt == VK_F16 || dt == VK_BF16) && (d == 32 || d == 64) && ldq % 8 == 0 && ldk % 8 == 0 &&
        ldv % 8 == 0 && aligned16)
        return VK_RELPOS_FORM_MFMA;
    if (d > STR_MAXD) {
        set_error("attention_relpos: head dim %d is beyond the strict form's limit of %d", d, STR_MAXD);
        return -VK_EINVAL;
    }
    return VK_RELPOS_FORM_STRICT;
}

// Queries per workgroup.  Matrix-core form: a wave serves 16 queries up to Lq = 16 and 32 beyond; a workgroup has as many waves as
// cover Lq, four at the most: 16, 32, 64, 96, then 128 from Lq = 97 on (27 tokens: one wave; 77: three; 709: six workgroups of four
// per head).  Strict form: 16.
static int relpos_queries(int form, int Lq) {
    if (form != VK_RELPOS_FORM_MFMA) return STR_QB;
    return Lq <= 16 ? 16 : 32 * std::min(ATT_MAXW, ceil_div(Lq, 32));
}

struct RelArgs {
    AttArgs a;
    RelBias rb;
};

static size_t mfma_lds_bytes(int D, int QB, int waves, int nlut) {
    return (size_t)(2 * D + waves * QB * 16) * ATT_PP * 2 + (size_t)2 * 3 * ATT_KT * sizeof(int) + (size_t)nlut * sizeof(float);
}

template <typename T, int D, int QB>
static int relpos_mfma_launch_qb(const RelArgs &r, float scale, hipStream_t s) {
    const AttArgs &a = r.a;
    const int per = relpos_queries(VK_RELPOS_FORM_MFMA, a.Lq), waves = per / (QB * 16), nrun = ceil_div(a.Lq, per);
    const size_t smem = mfma_lds_bytes(D, QB, waves, relpos_lut_len(r.rb.r1, r.rb.r2));
    const size_t cap = mfma_lds_bytes(D, QB, ATT_MAXW, 0) + RELPOS_LUT_MAX;
    return launch_lds(attention_relpos_kernel<T, D, QB>, dim3(a.B * a.heads * nrun), dim3(64 * waves), smem, cap, s, (const T *)a.q, a.ldq,
                      (const T *)a.k, a.ldk, (const T *)a.v, a.ldv, a.mask, r.rb.rel_q, r.rb.rel_k, r.rb.lut, r.rb.r1, r.rb.r2, (T *)a.out,
                      a.ldo, a.heads, a.Lq, a.Lk, nrun, scale);
}
template <typename T, int D>
static int relpos_mfma_launch(const RelArgs &r, float scale, hipStream_t s) {
    return r.a.Lq <= 16 ? relpos_mfma_launch_qb<T, D, 1>(r, scale, s) : relpos_mfma_launch_qb<T, D, 2>(r, scale, s);
}

template <typename T>
static int relpos_strict_launch(const RelArgs &r, float scale, hipStream_t s) {
    const AttArgs &a = r.a;
    const int nqb = ceil_div(a.Lq, STR_QB);
    return launch_lds(attention_stream_kernel<T, true, RelBias>, dim3(a.B * a.heads * nqb), dim3(256),
                      stream_bias_lds_bytes(a.d, relpos_lut_len(r.rb.r1, r.rb.r2)), stream_bias_lds_bytes(STR_MAXD, 0) + RELPOS_LUT_MAX, s,
                      VK_ATT_IO(T), a.d, nqb, scale, r.rb);
}

// what the launch refuses, reading through no pointer
static int relpos_check(const RelArgs &r) {
    const AttArgs &a = r.a;
    VK_REQUIRE(a.q && a.k && a.v && a.out && r.rb.rel_q && r.rb.rel_k && r.rb.lut, VK_EINVAL, "attention_relpos: null argument");
    VK_REQUIRE(a.B >= 1 && a.heads >= 1 && a.Lq >= 1 && a.Lk >= 1 && a.d >= 1, VK_EINVAL,
               "attention_relpos: sizes must be positive (B=%d heads=%d Lq=%d Lk=%d d=%d)", a.B, a.heads, a.Lq, a.Lk, a.d);
    VK_TRY(relpos_lut_check("attention_relpos", r.rb.r1, r.rb.r2));
    const long H = (long)a.heads * a.d;
    VK_REQUIRE(a.ldq >= H && a.ldk >= H && a.ldv >= H && a.ldo >= H, VK_EINVAL,
               "attention_relpos: a leading dimension (%d %d %d %d) is below heads * d = %ld", a.ldq, a.ldk, a.ldv, a.ldo, H);
    VK_REQUIRE(a.dt == VK_F32 || a.dt == VK_F16 || a.dt == VK_BF16, VK_EINVAL, "attention_relpos: dtype must be f32, f16 or bf16");
    const uintptr_t es = dtype_size(a.dt);
    VK_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out) % es == 0, VK_EINVAL,
               "attention_relpos: q, k, v and out must be aligned to their element");
    VK_REQUIRE(((uintptr_t)r.rb.rel_q | (uintptr_t)r.rb.rel_k | (uintptr_t)r.rb.lut | (uintptr_t)a.mask) % 4 == 0, VK_EINVAL,
               "attention_relpos: rel_q, rel_k, lut and mask must be 4-byte aligned");
    VK_REQUIRE((long)a.B * a.heads * ceil_div(a.Lq, 16) < (1L << 31), VK_EINVAL, "attention_relpos: too many (batch, head, query block) items");
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_attention_relpos_form(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16) {
    return relpos_form(Lq, Lk, d, dt, ldq, ldk, ldv, aligned16);
}

int vk_attention_relpos_queries(int form, int Lq) {
    if (!((form == VK_RELPOS_FORM_MFMA || form == VK_RELPOS_FORM_STRICT) && Lq >= 1)) {
        set_error("attention_relpos_queries: form %d, Lq %d", form, Lq);
        return -VK_EINVAL;
    }
    return relpos_queries(form, Lq);
}

int vk_attention_relpos_check(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask,
                              const int32_t *rel_q, const int32_t *rel_k, const float *lut, int r1, int r2, const void *out, int ldo, int B,
                              int heads, int Lq, int Lk, int d, vk_dtype dt) {
    const RelArgs r = {{q, k, v, mask, const_cast<void *>(out), ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d, dt}, {rel_q, rel_k, lut, r1, r2}};
    VK_TRY(relpos_check(r));
    const int aligned = ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0;
    const int form = relpos_form(Lq, Lk, d, dt, ldq, ldk, ldv, aligned);
    return form < 0 ? -form : VK_OK;
}

int vk_attention_relpos(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, const int32_t *rel_q,
                        const int32_t *rel_k, const float *lut, int r1, int r2, void *out, int ldo, int B, int heads, int Lq, int Lk, int d,
                        vk_dtype dt, void *stream) {
    const RelArgs r = {{q, k, v, mask, out, ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d, dt}, {rel_q, rel_k, lut, r1, r2}};
    VK_TRY(relpos_check(r));
    const int aligned = ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0;
    const int form = relpos_form(Lq, Lk, d, dt, ldq, ldk, ldv, aligned);
    if (form < 0) return -form;
    const float scale = 1.0f / sqrtf((float)d);
    hipStream_t s = (hipStream_t)stream;
    if (form == VK_RELPOS_FORM_MFMA) VK_DT16_D_SWITCH(dt, d, return relpos_mfma_launch<T, D>(r, scale, s));
    VK_DT_SWITCH(dt, "attention_relpos", return relpos_strict_launch<T>(r, scale, s));
    return VK_EINVAL;
}

}  // extern "C"
