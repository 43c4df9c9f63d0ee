// The device pieces the 16-bit matrix-core attention kernels share, each written once.  All of them assume
// the lane layout of v_mfma_f32_16x16x32 (mfma16.h): lane = 16 g + j, a score tile leaves a lane with S[row 4 g + e][column j].
//
//   att_row_frags        attention_mfma_kernel, ag16_* and rg_* kernels
//   att_image_t          ag16_dq_kernel (K^T), ag16_dkv_kernel (Q^T, dO^T): one wave builds it
//   att_image_t_wg       rg_dq_kernel (K^T), rg_dkv_kernel (Q^T, dO^T): the workgroup builds it
//   att_stage_triples, att_lane_triples      rg_dq_kernel, rg_dkv_kernel
//   att_online_row       pass 1 of ag16_dq_kernel and of rg_dq_kernel
//   att_grad_d, att_store_stats            ag16_dq_kernel, rg_dq_kernel
//   att_image_mma, att_store_rows            ag16_dq_kernel, rg_dq_kernel, rg_dkv_kernel (ag16_dkv_kernel keeps its two products
//                                            interleaved and its two stores in one loop)
// The bias score, rp_score, is relpos.h's.  The two online-soft-max forwards, attention_tiled_kernel and attention_relpos_kernel,
// share the constants, the exponential, pack16 (and rp_score) only and keep their bodies written out, instruction for instruction
// what they were: a boundary rule or the m / l update changed here has to be changed in those two as well.
#pragma once
#include "mfma16.h"

namespace vk {

constexpr int ATT_PP = 72;      // row pitch (elements) of every LDS image: 64 keys or queries + 8 (bank skew)
constexpr int ATT_KT = 64;      // keys (in the dK/dV kernels: queries) per tile: four 16-wide score blocks, two 32-wide product slices
constexpr int ATT_MAXW = 4;     // waves per workgroup at most

// The online soft-max's exponential: v_exp_f32 on x * log2(e).  Its error (about 1e-6 relative at a soft-max's arguments) is far
// below the rounding of P to a 16-bit type; exp(0) = 1 and exp(-inf) = 0 exactly, and a result below the normal range is 0.
static __device__ __forceinline__ float att_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// row r of a sequence of R rows that starts at `base` (row 0, this head's first column): the lane's fragments of the KD 32-wide
// slices, zero for a row outside the sequence
template <typename T, int KD>
__device__ __forceinline__ void att_row_frags(typename Mma16<T>::frag (&f)[KD], const T *base, long ld, int r, int R, int g) {
    typedef typename Mma16<T>::frag frag;
    const bool ok = r < R;
    const T *src = base + (long)(ok ? r : 0) * ld + g * 8;
#pragma unroll
    for (int ks = 0; ks < KD; ++ks) {
        const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
        f[ks] = ok ? t : frag{};
    }
}

// Rows [r0, r0 + 64) of that sequence, transposed, into img[c][row - r0] (pitch ATT_PP), zero for the rows outside it: 16-byte chunk
// c of rows r0 + 2 kp and r0 + 2 kp + 1 is written as eight (row, row + 1) words (32-bit LDS writes, consecutive kp on consecutive
// words).  The two forms assign (kp, c) differently and stay side by side.
// The wave form: a lane takes one row pair and half of its chunks.
template <typename T, int D>
__device__ __forceinline__ void att_image_t(T *img, const T *base, long ld, int r0, int R, int lane) {
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
        for (int e = 0; e < 8; ++e) img32[((c * 8 + e) * ATT_PP) / 2 + kp] = pack16<T>(t0[e], t1[e]);
    }
}
// The workgroup form: thread = (row pair, chunk), all threads of the workgroup together.
template <typename T, int D>
__device__ __forceinline__ void att_image_t_wg(T *img, const T *base, long ld, int r0, int R, int tid, int nthr) {
    typedef typename Mma16<T>::frag frag;
    unsigned *img32 = reinterpret_cast<unsigned *>(img);
    for (int i = tid; i < 32 * (D / 8); i += nthr) {
        const int kp = i & 31, c = i >> 5, row = r0 + 2 * kp;
        frag t0 = {}, t1 = {};
        if (row < R) t0 = *reinterpret_cast<const frag *>(base + (long)row * ld + c * 8);
        if (row + 1 < R) t1 = *reinterpret_cast<const frag *>(base + (long)(row + 1) * ld + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) img32[((c * 8 + e) * ATT_PP) / 2 + kp] = pack16<T>(t0[e], t1[e]);
    }
}

// the position triples of rows [r0, r0 + 64) of rel [R, 3] into tr[3][64], (0, 0, 0) past the end: threads 0 .. 63 of the workgroup
__device__ __forceinline__ void att_stage_triples(int *tr, const int32_t *rel, int r0, int R, int tid) {
    if (tid < ATT_KT) {
        const int row = r0 + tid;
        const bool ok = row < R;
        const int32_t *src = rel + (long)(ok ? row : 0) * 3;
        tr[tid] = ok ? src[0] : 0;
        tr[ATT_KT + tid] = ok ? src[1] : 0;
        tr[2 * ATT_KT + tid] = ok ? src[2] : 0;
    }
}
// the triples of a lane's own four rows r0 + e, into registers, (0, 0, 0) past the end
__device__ __forceinline__ void att_lane_triples(int (&p)[4], int (&x)[4], int (&y)[4], const int32_t *rel, int r0, int R) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool ok = r0 + e < R;
        const int32_t *src = rel + (long)(ok ? r0 + e : 0) * 3;
        p[e] = ok ? src[0] : 0;
        x[e] = ok ? src[1] : 0;
        y[e] = ok ? src[2] : 0;
    }
}

// One tile of the online soft-max for row 4 g + e, whose scores of the tile are sc[kb][e] (-inf outside the sequence): the row
// maximum over the key blocks in registers, then over the 16 lanes of the group; the sum of exp(s - m_new) the same way; m and l
// updated, l by ONE fmaf (first tile: alpha = exp(-inf) = 0).  Pass 1 of both dQ kernels; the forwards write the same steps out
// around their P image and must keep them equal to this.
template <int KB>
__device__ __forceinline__ void att_online_row(const m16_f4 (&sc)[KB], int e, float &m, float &l) {
    float mx = sc[0][e];
#pragma unroll
    for (int kb = 1; kb < KB; ++kb) mx = fmaxf(mx, sc[kb][e]);
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    const float mn = fmaxf(m, mx);
    const float alpha = att_exp(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) sum += att_exp(sc[kb][e] - mn);        // keys outside: exp(-inf) = 0
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
    m = mn;
    l = fmaf(alpha, l, sum);
}

// What pass 2 of a dQ kernel needs of rows 4 g + e beside m: D = sum_c dO O, from the fragments of row j (this lane's 8 KD columns,
// then the four lanes of the row; rows 4 g + e fetch theirs from lanes 4 g + e), and 1 / l, one division
template <typename T, int KD>
__device__ __forceinline__ void att_grad_d(float (&dd)[4], float (&il)[4], const typename Mma16<T>::frag (&dof)[KD],
                                           const typename Mma16<T>::frag (&of)[KD], const float (&l)[4], int g) {
    float part = 0.f;
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

// (m, 1 / l, D) of the first nq of a wave's 16 rows to stats[3][n], whose first row is srow0: lanes j = 0, rows 4 g + e
__device__ __forceinline__ void att_store_stats(float *stats, long n, long srow0, int nq, const float (&m)[4], const float (&il)[4],
                                                const float (&dd)[4], int g, int j) {
    if (j != 0) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        if (r < nq) {
            stats[srow0 + r] = m[e];
            stats[n + srow0 + r] = il[e];
            stats[2 * n + srow0 + r] = dd[e];
        }
    }
}

// acc[db] += A B over one 64-wide tile: `a` is the [16][64] image of A (dS, P^T or dS^T), `bt` the [16 NDB][64] transposed image of
// B (K^T, dO^T or Q^T); two 32-wide slices ascending
template <typename T, int NDB>
__device__ __forceinline__ void att_image_mma(m16_f4 (&acc)[NDB], const T *a, const T *bt, int g, int j) {
    typedef typename Mma16<T>::frag frag;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
        const frag af = *reinterpret_cast<const frag *>(a + j * ATT_PP + k2 * 32 + g * 8);
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const frag bf = *reinterpret_cast<const frag *>(bt + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
            acc[db] = Mma16<T>::mma(af, bf, acc[db]);
        }
    }
}

// the first n of a wave's 16 accumulator rows, times scale, to dst (the wave's row 0, this head's first column)
template <int NDB>
__device__ __forceinline__ void att_store_rows(float *dst, long ld, const m16_f4 (&acc)[NDB], float scale, int n, int g, int j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        if (r >= n) continue;
#pragma unroll
        for (int db = 0; db < NDB; ++db) dst[(long)r * ld + db * 16 + j] = acc[db][e] * scale;
    }
}

}  // namespace vk
