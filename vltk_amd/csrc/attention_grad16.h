// The backward of the 16-bit attention forward (attention_tiled_kernel of attention_tiled.h) on the matrix cores: what mixed-precision
// fine-tuning needs beside gemm16.hip.  q, k, v, o and dout are bf16 / fp16; dq, dk and dv are fp32.  It
// keeps the ownership scheme of attention_grad.hip, so it needs no atomics and no split accumulation: every output element has
// one writer and one fixed summation order, and the same input gives the same bits.
//
//   ag16_dq_kernel    one wave (a 64-thread workgroup) owns 16 queries: Q and dO fragments in registers, straight from memory.
//                     Pass 1 walks the keys 64 at a time (K rows are the B fragments as they lie in memory), S = Q K^T on
//                     v_mfma_f32_16x16x32, and keeps the online row maximum m and row sum l exactly as the forward does; then
//                     D = sum_c dO O per row.  m, 1 / l and D go to the workspace for the other kernel.  Pass 2 walks the keys
//                     again: S and dP = dO V^T (V rows from memory), P = exp(s - m) (1 / l), dS = P (dP - D) in fp32; dS, rounded
//                     to T, goes through a [query][key] LDS image and K through a transposed [c][key] image to become the operands
//                     of dQ += dS K.  dQ = scale * (the sum).
//   ag16_dkv_kernel   the mirror image: one wave owns 16 keys (K and V fragments in registers, as the A operands: S^T = K Q^T and
//                     dP^T = V dO^T leave a lane with key 4 g + e of query j) and walks the queries 64 at a time with their
//                     statistics from the workspace.  P^T and dS^T, rounded to T, go through [key][query] images, Q and dO through
//                     transposed [c][query] images: dV += P^T dO, dK += dS^T Q.  dK = scale * (the sum).
//
// A key or query outside the sequence carries P = 0 and dS = 0 and zero rows in every image.  A key whose mask is below -1e30
// absorbs q . k in fp32, so a row with every key masked has s - m = 0 and the uniform P the forward gives.
//
// LDS per workgroup (one wave), images of pitch 72 elements = 144 bytes: dQ kernel (16 + d) rows: 11520 bytes at d = 64, 6912 at
// d = 32; dK/dV kernel (32 + 2 d) rows: 23040 / 13824 bytes.  Of 160 KiB that is 14 and 7 workgroups per CU at d = 64; the
// registers (110 and 134 at d = 64) hold the kernels to 4 and 3 waves per SIMD first.  Accesses, all forms the forward already uses:
//   dS / P image write   ds_write_b16, lane 16 g + j at row 4 g + e, element 16 kb + j: a half-wave writes 16 consecutive halves
//                        of two rows 4 rows = 144 words = 16 banks (of 32) apart: 16 words on 16 different banks, two lanes on
//                        each word (the halves of a word are separate writes: 2-way at most).
//   transposed image write   ds_write_b32, lane = (key pair kp = lane & 31, half of the chunks): a half-wave writes 32 consecutive
//                        words of one row: conflict-free.
//   fragment read        ds_read_b128 at row j, elements 32 k2 + 8 g ..: rows 36 words apart, first banks (of 64) 0, 36, 8, 44, ..,
//                        28: the 16 rows of a lane group take 16 different 4-bank slots: conflict-free.
//
// Rounding points (u16 = the unit of T, u = 2^-24):
//   s        the instruction's fp32 sum over c (exact products), then fmaf(s, scale, mask)
//   m, l     m exact; per 64-key tile alpha = exp(m_old - m_new), e = exp(s - m_new) (v_exp_f32 on x log2 e, about 1e-6), the
//            tile's sum over registers then the xor-shuffle tree, l = fmaf(alpha, l, sum); 1 / l one division
//   P        exp(s - m) * (1 / l) in fp32; rounded to T (u16) for dV = P^T dO only
//   D        per lane 8 (d = 32) or 16 (d = 64) fmaf steps, then two xor-shuffle adds
//   dP       the instruction's fp32 sum;  dS = P (dP - D) from the unrounded P, two roundings, then rounded to T (u16)
//   dQ, dK, dV   fp32 accumulation of exact products over 32-row slices ascending; dQ and dK then one product with scale
// Integer data chosen so that P and dS are representable in T and every sum stays below 2^24 is exact.
//
// DROP (vk_attention_grad_16_dropout, instantiated in attention_dropout.hip; the one trailing argument is a DropArgs): the backward
// of dropout(softmax(s)) under the mask of philox.h.  D is unchanged (o is the dropped forward's output); dP~ = keep ? rs dP : 0;
// dS = P (dP~ - D) from the undropped P; dV sums P~ = keep ? rs P : 0 rounded to T.  Per 16 x 64 tile a lane makes one Philox call
// and four ds_bpermute_b32 (drop_tile_bits): the dQ kernel's lane holds S[4 g + e][16 kb + j] and tests bit 8 (j & 3) + e of block
// (g, 4 kb + (j >> 2)); the dK/dV kernel's lane holds S^T[4 g + e][16 qb + j] and tests bit 8 e + (j & 3) of the block of query
// block 4 qb + (j >> 2) and key block g: the 4 x 4 block is its own transpose, so the three kernels agree.  LDS as above; VGPRs
// as the compiler reports them, plain -> DROP: dQ 94 -> 100 (d = 64), 74 -> 82 (d = 32); dK/dV 98 -> 108, 88 -> 90: both keep
// four waves per SIMD at d = 64.  DROP = false takes no trailing argument and is the kernel as it was.
//
// Row fragments, the transposed images, the online row update of pass 1 (att_online_row), D, the statistics store,
// the image products and the scaled stores are attention_mma.h's; what stays here is how a score, dP and dS are formed.
#pragma once
#include "attention_mma.h"
#include "philox.h"

namespace vk {

constexpr int AG16_OWN = 16;                        // queries (dQ kernel) or keys (dK/dV kernel) a wave owns

struct AttGrad16Args {
    const void *q, *k, *v, *o, *dout;
    const float *mask;
    float *dq, *dk, *dv;
    float *stats;                                   // [3][B * heads * Lq]: m, 1 / l, D
    long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, heads, Lq, Lk;
    float scale;
};

template <typename T, int D, bool DROP, typename... DA>
__global__ __launch_bounds__(64) void ag16_dq_kernel(AttGrad16Args a, int nqb, DA... drop) {
    static_assert(sizeof...(DA) == (DROP ? 1 : 0), "a DropArgs behind the arguments of the DROP form, nothing otherwise");
    const DropArgs da = drop_args_of(drop...);
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = ATT_KT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char ag16_lds[];
    T *dsi = reinterpret_cast<T *>(ag16_lds), *kt = dsi + AG16_OWN * ATT_PP;
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const int bh = blockIdx.x / nqb, q0 = (blockIdx.x - bh * nqb) * AG16_OWN;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int nq = a.Lq - q0;                        // owned rows inside the sequence (16 or more: all)
    const T *qb_ = static_cast<const T *>(a.q) + (long)b * a.Lq * a.ldq + h * D + q0 * a.ldq;
    const T *dob = static_cast<const T *>(a.dout) + (long)b * a.Lq * a.lddo + h * D + q0 * a.lddo;
    const T *ob = static_cast<const T *>(a.o) + (long)b * a.Lq * a.ldo + h * D + q0 * a.ldo;
    const T *kbase = static_cast<const T *>(a.k) + (long)b * a.Lk * a.ldk + h * D;
    const T *vbase = static_cast<const T *>(a.v) + (long)b * a.Lk * a.ldv + h * D;
    const float *mrow = a.mask ? a.mask + (long)b * a.Lk : nullptr;

    frag qf[KD], dof[KD];
    att_row_frags<T, KD>(qf, qb_, a.ldq, j, nq, g);
    att_row_frags<T, KD>(dof, dob, a.lddo, j, nq, g);

    // ---- pass 1: m and l of rows 4 g + e, online over the key tiles as the forward keeps them ----
    float m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = -INFINITY;
        l[e] = 0.f;
    }
    for (int k0 = 0; k0 < a.Lk; k0 += ATT_KT) {
        m16_f4 sc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            frag kf[KD];
            att_row_frags<T, KD>(kf, kbase, a.ldk, k0 + kb * 16 + j, a.Lk, g);
            m16_f4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) s = Mma16<T>::mma(qf[ks], kf[ks], s);
            const int key = k0 + kb * 16 + j;
            const bool ok = key < a.Lk;
            const float mk = ok && mrow ? mrow[key] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = ok ? fmaf(s[e], a.scale, mk) : -INFINITY;
            sc[kb] = s;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) att_online_row(sc, e, m[e], l[e]);
    }
    float il[4], dd[4];
    frag of[KD];
    att_row_frags<T, KD>(of, ob, a.ldo, j, nq, g);
    att_grad_d<T, KD>(dd, il, dof, of, l, g);
    att_store_stats(a.stats, (long)a.B * a.heads * a.Lq, (long)bh * a.Lq + q0, nq, m, il, dd, g, j);

    // ---- pass 2: dQ ----
    m16_f4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Lk; k0 += ATT_KT) {
        att_image_t<T, D>(kt, kbase, a.ldk, k0, a.Lk, lane);
        uint32_t keep[KB] = {};
        if constexpr (DROP) {
            drop_tile_bits(keep, da, (uint64_t)bh * ((a.Lq + 3) >> 2), (uint64_t)((a.Lk + 3) >> 2), q0 >> 2, k0 >> 2, true, g, j);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) keep[kb] >>= 8 * (j & 3);            // bit e: query 4 g + e of this lane's key
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            frag kf[KD], vf[KD];
            att_row_frags<T, KD>(kf, kbase, a.ldk, k0 + kb * 16 + j, a.Lk, g);
            att_row_frags<T, KD>(vf, vbase, a.ldv, k0 + kb * 16 + j, a.Lk, g);
            m16_f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) {
                s = Mma16<T>::mma(qf[ks], kf[ks], s);
                dp = Mma16<T>::mma(dof[ks], vf[ks], dp);
            }
            const int key = k0 + kb * 16 + j;
            const bool okk = key < a.Lk;
            const float mk = okk && mrow ? mrow[key] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float dsv = 0.f;
                if (okk && 4 * g + e < nq) {
                    const float p = att_exp(fmaf(s[e], a.scale, mk) - m[e]) * il[e];
                    if constexpr (DROP) dsv = p * (((keep[kb] >> e) & 1u ? da.rs * dp[e] : 0.f) - dd[e]);
                    else dsv = p * (dp[e] - dd[e]);
                }
                dsi[(4 * g + e) * ATT_PP + kb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();
        att_image_mma<T, NDB>(acc, dsi, kt, g, j);
        __syncthreads();            // the next tile overwrites the images
    }
    att_store_rows<NDB>(a.dq + ((long)b * a.Lq + q0) * a.lddq + h * D, a.lddq, acc, a.scale, nq, g, j);
}

template <typename T, int D, bool DROP, typename... DA>
__global__ __launch_bounds__(64) void ag16_dkv_kernel(AttGrad16Args a, int nkb, DA... drop) {
    static_assert(sizeof...(DA) == (DROP ? 1 : 0), "a DropArgs behind the arguments of the DROP form, nothing otherwise");
    const DropArgs da = drop_args_of(drop...);
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, QB = ATT_KT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char ag16_lds[];
    T *pt = reinterpret_cast<T *>(ag16_lds), *dst = pt + AG16_OWN * ATT_PP, *qt = dst + AG16_OWN * ATT_PP, *dot = qt + D * ATT_PP;
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const int bh = blockIdx.x / nkb, j0 = (blockIdx.x - bh * nkb) * AG16_OWN;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int nk = a.Lk - j0;                        // owned keys inside the sequence (16 or more: all)
    const T *qbase = static_cast<const T *>(a.q) + (long)b * a.Lq * a.ldq + h * D;
    const T *dobase = static_cast<const T *>(a.dout) + (long)b * a.Lq * a.lddo + h * D;
    const T *kb_ = static_cast<const T *>(a.k) + ((long)b * a.Lk + j0) * a.ldk + h * D;
    const T *vb_ = static_cast<const T *>(a.v) + ((long)b * a.Lk + j0) * a.ldv + h * D;
    const long n = (long)a.B * a.heads * a.Lq;
    const float *st = a.stats + (long)bh * a.Lq;

    frag kf[KD], vf[KD];
    att_row_frags<T, KD>(kf, kb_, a.ldk, j, nk, g);
    att_row_frags<T, KD>(vf, vb_, a.ldv, j, nk, g);
    float mk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) mk[e] = a.mask && 4 * g + e < nk ? a.mask[(long)b * a.Lk + j0 + 4 * g + e] : 0.f;

    m16_f4 acck[NDB], accv[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acck[db] = accv[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < a.Lq; q0 += ATT_KT) {
        att_image_t<T, D>(qt, qbase, a.ldq, q0, a.Lq, lane);
        att_image_t<T, D>(dot, dobase, a.lddo, q0, a.Lq, lane);
        uint32_t keep[QB] = {};
        if constexpr (DROP) {
            drop_tile_bits(keep, da, (uint64_t)bh * ((a.Lq + 3) >> 2), (uint64_t)((a.Lk + 3) >> 2), q0 >> 2, j0 >> 2, false, g, j);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) keep[qb] >>= j & 3;                  // bit 8 e: key 4 g + e of this lane's query
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int qr = q0 + qb * 16 + j;
            const bool okq = qr < a.Lq;
            frag qf[KD], dof[KD];
            att_row_frags<T, KD>(qf, qbase, a.ldq, qr, a.Lq, g);
            att_row_frags<T, KD>(dof, dobase, a.lddo, qr, a.Lq, g);
            m16_f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) {
                s = Mma16<T>::mma(kf[ks], qf[ks], s);
                dp = Mma16<T>::mma(vf[ks], dof[ks], dp);
            }
            const float mm = okq ? st[qr] : 0.f, il = okq ? st[n + qr] : 0.f, dd = okq ? st[2 * n + qr] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p = 0.f, dsv = 0.f;
                if (okq && 4 * g + e < nk) {
                    p = att_exp(fmaf(s[e], a.scale, mk[e]) - mm) * il;
                    if constexpr (DROP) {
                        const bool kept = (keep[qb] >> (8 * e)) & 1u;
                        dsv = p * ((kept ? da.rs * dp[e] : 0.f) - dd);
                        p = kept ? da.rs * p : 0.f;                      // P~, what dV sums
                    } else {
                        dsv = p * (dp[e] - dd);
                    }
                }
                pt[(4 * g + e) * ATT_PP + qb * 16 + j] = (T)p;
                dst[(4 * g + e) * ATT_PP + qb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();
        // the two products interleaved: att_image_mma's step, for two accumulators at once
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            const frag pf = *reinterpret_cast<const frag *>(pt + j * ATT_PP + k2 * 32 + g * 8);
            const frag sf = *reinterpret_cast<const frag *>(dst + j * ATT_PP + k2 * 32 + g * 8);
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const frag of = *reinterpret_cast<const frag *>(dot + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
                const frag qf = *reinterpret_cast<const frag *>(qt + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
                accv[db] = Mma16<T>::mma(pf, of, accv[db]);
                acck[db] = Mma16<T>::mma(sf, qf, acck[db]);
            }
        }
        __syncthreads();            // the next tile overwrites the images
    }
    float *dkb = a.dk + ((long)b * a.Lk + j0) * a.lddk + h * D, *dvb = a.dv + ((long)b * a.Lk + j0) * a.lddv + h * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        if (r >= nk) continue;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            dkb[(long)r * a.lddk + db * 16 + j] = acck[db][e] * a.scale;
            dvb[(long)r * a.lddv + db * 16 + j] = accv[db][e];
        }
    }
}

static size_t ag16_workspace_bytes(int B, int heads, int Lq) {
    if (B < 1 || heads < 1 || Lq < 1) return 0;
    return (size_t)3 * B * heads * Lq * sizeof(float);
}

// everything the launch refuses, without touching a device or reading through a pointer
static int ag16_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const void *o, long ldo, const void *dout,
                      long lddo, const float *dq, long lddq, const float *dk, long lddk, const float *dv, long lddv, int B, int heads, int Lq,
                      int Lk, int d, vk_dtype dt, const void *workspace, size_t workspace_bytes) {
    VK_REQUIRE(q && k && v && o && dout && dq && dk && dv, VK_EINVAL, "attention_grad_16: null argument");
    VK_REQUIRE(dt == VK_F16 || dt == VK_BF16, VK_EINVAL, "attention_grad_16: dt must be f16 or bf16 (fp32 is vk_attention_grad's)");
    VK_REQUIRE(B >= 1 && heads >= 1 && Lq >= 1 && Lk >= 1, VK_EINVAL, "attention_grad_16: bad geometry (B=%d heads=%d Lq=%d Lk=%d)", B, heads,
               Lq, Lk);
    VK_REQUIRE(d == 32 || d == 64, VK_EINVAL, "attention_grad_16: head dim %d is neither 32 nor 64 (the 16-bit forward's reach)", d);
    const long width = (long)heads * d;
    const long lds[8] = {ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv};
    const void *const ptrs[8] = {q, k, v, o, dout, dq, dk, dv};
    static const char *const names[8] = {"q", "k", "v", "o", "dout", "dq", "dk", "dv"};
    for (int i = 0; i < 8; ++i) {
        VK_REQUIRE(lds[i] >= width, VK_EINVAL, "attention_grad_16: the leading dimension %ld of %s is below heads * d = %ld", lds[i], names[i],
                   width);
        VK_REQUIRE(lds[i] % 8 == 0, VK_EINVAL, "attention_grad_16: the leading dimension %ld of %s is no multiple of 8", lds[i], names[i]);
        VK_REQUIRE(((uintptr_t)ptrs[i] & 15) == 0, VK_EINVAL, "attention_grad_16: %s is not 16-byte aligned", names[i]);
    }
    VK_REQUIRE((long)B * heads * ceil_div(Lq > Lk ? Lq : Lk, AG16_OWN) < (1L << 31), VK_EINVAL,
               "attention_grad_16: too many (batch, head, tile) items");
    const size_t need = ag16_workspace_bytes(B, heads, Lq);
    VK_REQUIRE(workspace && workspace_bytes >= need, VK_EINVAL, "attention_grad_16: needs a workspace of %zu bytes, got %zu", need,
               workspace_bytes);
    VK_REQUIRE(((uintptr_t)workspace & 3) == 0, VK_EINVAL, "attention_grad_16: the workspace must be 4-byte aligned");
    return VK_OK;
}

// the DROP forms (a DropArgs behind the stream) have the same grids and LDS
template <typename T, int D, typename... DA>
static int ag16_launch(const AttGrad16Args &a, hipStream_t s, DA... da) {
    constexpr bool DROP = sizeof...(DA) != 0;
    const int nqb = ceil_div(a.Lq, AG16_OWN), nkb = ceil_div(a.Lk, AG16_OWN);
    const size_t lq = (size_t)(AG16_OWN + D) * ATT_PP * sizeof(T), lk = (size_t)(2 * AG16_OWN + 2 * D) * ATT_PP * sizeof(T);
    VK_TRY(launch_lds(ag16_dq_kernel<T, D, DROP, DA...>, dim3(a.B * a.heads * nqb), dim3(64), lq, lq, s, a, nqb, da...));
    VK_TRY(launch_lds(ag16_dkv_kernel<T, D, DROP, DA...>, dim3(a.B * a.heads * nkb), dim3(64), lk, lk, s, a, nkb, da...));
    return VK_OK;
}

}  // namespace vk
