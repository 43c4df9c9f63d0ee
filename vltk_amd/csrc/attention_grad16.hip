// The backward of the 16-bit attention forward (attention_tiled_kernel of attention.hip) on the matrix cores: what mixed-precision
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
#include "mfma16.h"

namespace vk {

constexpr int AG16_OWN = 16, AG16_STEP = 64, AG16_PP = 72;

struct AttGrad16Args {
    const void *q, *k, *v, *o, *dout;
    const float *mask;
    float *dq, *dk, *dv;
    float *stats;                                   // [3][B * heads * Lq]: m, 1 / l, D
    long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, heads, Lq, Lk;
    float scale;
};

// the forward's exponential (tat_exp of attention.hip): exp(0) = 1 and exp(-inf) = 0 exactly
static __device__ __forceinline__ float ag16_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// row r of a sequence of R rows that starts at `base` (row 0, this head's first column): the lane's fragments of the KD 32-wide
// slices, zero for a row outside the sequence
template <typename T, int KD>
__device__ __forceinline__ void ag16_row_frags(typename Mma16<T>::frag (&f)[KD], const T *base, long ld, int r, int R, int g) {
    typedef typename Mma16<T>::frag frag;
    const bool ok = r < R;
    const T *src = base + (long)(ok ? r : 0) * ld + g * 8;
#pragma unroll
    for (int ks = 0; ks < KD; ++ks) {
        const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
        f[ks] = ok ? t : frag{};
    }
}

// rows [r0, r0 + 64) of that sequence, transposed, into img[c][row - r0] (pitch AG16_PP), zero for the rows outside it: a lane
// takes two rows and half of their 16-byte chunks, and writes (row, row + 1) pairs as words (attention_tiled_kernel's V^T image)
template <typename T, int D>
__device__ __forceinline__ void ag16_image_t(T *img, const T *base, long ld, int r0, int R, int lane) {
    typedef typename Mma16<T>::frag frag;
    constexpr int HALF = D / 16;
    unsigned *img32 = reinterpret_cast<unsigned *>(img);
    const int kp = lane & 31, c0 = (lane >> 5) * HALF;
    const int row = r0 + 2 * kp;
#pragma unroll
    for (int it = 0; it < HALF; ++it) {
        const int c = c0 + it;
        frag t0 = {}, t1 = {};
        if (row < R) t0 = *reinterpret_cast<const frag *>(base + (long)row * ld + c * 8);
        if (row + 1 < R) t1 = *reinterpret_cast<const frag *>(base + (long)(row + 1) * ld + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) img32[((c * 8 + e) * AG16_PP) / 2 + kp] = pack16<T>(t0[e], t1[e]);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(64) void ag16_dq_kernel(AttGrad16Args a, int nqb) {
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = AG16_STEP / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char ag16_lds[];
    T *dsi = reinterpret_cast<T *>(ag16_lds), *kt = dsi + AG16_OWN * AG16_PP;
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
    ag16_row_frags<T, KD>(qf, qb_, a.ldq, j, nq, g);
    ag16_row_frags<T, KD>(dof, dob, a.lddo, j, nq, g);

    // ---- pass 1: m and l of rows 4 g + e, online over the key tiles as the forward keeps them ----
    float m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = -INFINITY;
        l[e] = 0.f;
    }
    for (int k0 = 0; k0 < a.Lk; k0 += AG16_STEP) {
        m16_f4 sc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            frag kf[KD];
            ag16_row_frags<T, KD>(kf, kbase, a.ldk, k0 + kb * 16 + j, a.Lk, g);
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
        for (int e = 0; e < 4; ++e) {
            float mx = sc[0][e];
#pragma unroll
            for (int kb = 1; kb < KB; ++kb) mx = fmaxf(mx, sc[kb][e]);
#pragma unroll
            for (int s = 8; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            const float mn = fmaxf(m[e], mx);
            const float alpha = ag16_exp(m[e] - mn);            // first tile: exp(-inf) = 0
            float sum = 0.f;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) sum += ag16_exp(sc[kb][e] - mn);      // keys outside: exp(-inf) = 0
#pragma unroll
            for (int s = 8; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
            m[e] = mn;
            l[e] = fmaf(alpha, l[e], sum);
        }
    }
    float il[4], dd[4];
    {
        // D of row j: this lane's 8 KD columns, then the four lanes of the row; rows 4 g + e fetch theirs from lanes 4 g + e
        float part = 0.f;
        frag of[KD];
        ag16_row_frags<T, KD>(of, ob, a.ldo, j, nq, g);
#pragma unroll
        for (int ks = 0; ks < KD; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) part = fmaf((float)dof[ks][e], (float)of[ks][e], part);
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dd[e] = __shfl(part, 4 * g + e, 64);
            il[e] = 1.0f / l[e];
        }
    }
    if (j == 0) {
        const long n = (long)a.B * a.heads * a.Lq;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            if (r < nq) {
                const long srow = (long)bh * a.Lq + q0 + r;
                a.stats[srow] = m[e];
                a.stats[n + srow] = il[e];
                a.stats[2 * n + srow] = dd[e];
            }
        }
    }

    // ---- pass 2: dQ ----
    m16_f4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Lk; k0 += AG16_STEP) {
        ag16_image_t<T, D>(kt, kbase, a.ldk, k0, a.Lk, lane);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            frag kf[KD], vf[KD];
            ag16_row_frags<T, KD>(kf, kbase, a.ldk, k0 + kb * 16 + j, a.Lk, g);
            ag16_row_frags<T, KD>(vf, vbase, a.ldv, k0 + kb * 16 + j, a.Lk, g);
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
                    const float p = ag16_exp(fmaf(s[e], a.scale, mk) - m[e]) * il[e];
                    dsv = p * (dp[e] - dd[e]);
                }
                dsi[(4 * g + e) * AG16_PP + kb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            const frag pf = *reinterpret_cast<const frag *>(dsi + j * AG16_PP + k2 * 32 + g * 8);
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const frag kf = *reinterpret_cast<const frag *>(kt + (db * 16 + j) * AG16_PP + k2 * 32 + g * 8);
                acc[db] = Mma16<T>::mma(pf, kf, acc[db]);
            }
        }
        __syncthreads();            // the next tile overwrites the images
    }
    float *dqb = a.dq + ((long)b * a.Lq + q0) * a.lddq + h * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        if (r >= nq) continue;
#pragma unroll
        for (int db = 0; db < NDB; ++db) dqb[(long)r * a.lddq + db * 16 + j] = acc[db][e] * a.scale;
    }
}

template <typename T, int D>
__global__ __launch_bounds__(64) void ag16_dkv_kernel(AttGrad16Args a, int nkb) {
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, QB = AG16_STEP / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char ag16_lds[];
    T *pt = reinterpret_cast<T *>(ag16_lds), *dst = pt + AG16_OWN * AG16_PP, *qt = dst + AG16_OWN * AG16_PP, *dot = qt + D * AG16_PP;
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
    ag16_row_frags<T, KD>(kf, kb_, a.ldk, j, nk, g);
    ag16_row_frags<T, KD>(vf, vb_, a.ldv, j, nk, g);
    float mk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) mk[e] = a.mask && 4 * g + e < nk ? a.mask[(long)b * a.Lk + j0 + 4 * g + e] : 0.f;

    m16_f4 acck[NDB], accv[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acck[db] = accv[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < a.Lq; q0 += AG16_STEP) {
        ag16_image_t<T, D>(qt, qbase, a.ldq, q0, a.Lq, lane);
        ag16_image_t<T, D>(dot, dobase, a.lddo, q0, a.Lq, lane);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int qr = q0 + qb * 16 + j;
            const bool okq = qr < a.Lq;
            frag qf[KD], dof[KD];
            ag16_row_frags<T, KD>(qf, qbase, a.ldq, qr, a.Lq, g);
            ag16_row_frags<T, KD>(dof, dobase, a.lddo, qr, a.Lq, g);
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
                    p = ag16_exp(fmaf(s[e], a.scale, mk[e]) - mm) * il;
                    dsv = p * (dp[e] - dd);
                }
                pt[(4 * g + e) * AG16_PP + qb * 16 + j] = (T)p;
                dst[(4 * g + e) * AG16_PP + qb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            const frag pf = *reinterpret_cast<const frag *>(pt + j * AG16_PP + k2 * 32 + g * 8);
            const frag sf = *reinterpret_cast<const frag *>(dst + j * AG16_PP + k2 * 32 + g * 8);
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const frag of = *reinterpret_cast<const frag *>(dot + (db * 16 + j) * AG16_PP + k2 * 32 + g * 8);
                const frag qf = *reinterpret_cast<const frag *>(qt + (db * 16 + j) * AG16_PP + k2 * 32 + g * 8);
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

template <typename T, int D>
static int ag16_launch(const AttGrad16Args &a, hipStream_t s) {
    const int nqb = ceil_div(a.Lq, AG16_OWN), nkb = ceil_div(a.Lk, AG16_OWN);
    const size_t lq = (size_t)(AG16_OWN + D) * AG16_PP * sizeof(T), lk = (size_t)(2 * AG16_OWN + 2 * D) * AG16_PP * sizeof(T);
    VK_TRY(launch_lds(ag16_dq_kernel<T, D>, dim3(a.B * a.heads * nqb), dim3(64), lq, lq, s, a, nqb));
    VK_TRY(launch_lds(ag16_dkv_kernel<T, D>, dim3(a.B * a.heads * nkb), dim3(64), lk, lk, s, a, nkb));
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

size_t vk_attention_grad_16_workspace_bytes(int B, int heads, int Lq) { return ag16_workspace_bytes(B, heads, Lq); }

int vk_attention_grad_16_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o,
                               long ldo, const void *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk,
                               const float *dv, long lddv, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, const void *workspace,
                               size_t workspace_bytes) {
    (void)mask;                     // may be NULL: no key is masked
    return ag16_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, dt, workspace,
                      workspace_bytes);
}

int vk_attention_grad_16(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o, long ldo,
                         const void *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, int B, int heads,
                         int Lq, int Lk, int d, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream) {
    VK_TRY(ag16_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, dt, workspace,
                      workspace_bytes));
    const AttGrad16Args a = {q, k, v, o, dout, mask, dq, dk, dv, (float *)workspace, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                             B, heads, Lq, Lk, 1.0f / sqrtf((float)d)};
    hipStream_t s = (hipStream_t)stream;
    if (dt == VK_BF16) return d == 64 ? ag16_launch<__bf16, 64>(a, s) : ag16_launch<__bf16, 32>(a, s);
    return d == 64 ? ag16_launch<_Float16, 64>(a, s) : ag16_launch<_Float16, 32>(a, s);
}

}  // extern "C"
