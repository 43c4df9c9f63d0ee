// vk_attention_relpos_grad: the backward of the matrix-core form of vk_attention_relpos, what fine-tuning
// LayoutLMv3 needs beside attention_grad16.h.  q, k, v, o and dout are bf16 / fp16, head dim 32 / 64; dq, dk, dv and dlut are fp32.
//
//   s  = (q . k + (t1 + (tx + ty))) * scale + mask          the forward's score, the bias read from the head's table in LDS
//   P  = softmax(s),  D = sum_c dO O,  dP = dO V^T,  dS = P (dP - D)
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO       P rounded to T for dV only, dS rounded to T for dQ / dK only
//   dlut[h][e] = scale * sum of the UNROUNDED dS[b, h, i, j] over every (b, i, j) whose clamped distance for that term is e
//
// The arithmetic, lane layouts and two-pass scheme are ag16_dq_kernel's and ag16_dkv_kernel's (a lane holds S[4 g + e][16 kb + j],
// or S^T in the mirror); the work split is the forward's:
//
//   rg_dq_kernel    a WORKGROUP of 1 .. 4 waves per (batch, head, run of waves * 16 queries); wave w owns the w-th 16 queries.  The
//                   waves share the head's table, the integer histogram of the table gradient, a tile's 64 key triples and the
//                   tile's K^T image (ag16: every wave builds its own), the last two double-buffered.  A lane keeps the triples of
//                   its four query rows in registers and forms an index with subtract, max, min, add.  Pass 1 (m, l, D -> the
//                   workspace) costs one barrier a tile, pass 2 (dS -> histogram, dS image, dQ += dS K) two.
//   rg_dkv_kernel   the mirror: wave w owns 16 keys (fragments, mask and triples in registers); the waves share the table, a tile's
//                   64 query triples and the Q^T and dO^T images (single-buffered: three barriers a tile, and LDS for three workgroups
//                   a CU).  P^T and dS^T images are per wave.
//   A wave whose rows lie past the end of the sequence computes on zeros and stores nothing: the barriers stay uniform.
//
// LDS (T = 2 bytes, image pitch 72):
//   dQ     K^T [2][D][72] T | dS [waves][16][72] T | key triples [2][3][64] int | histogram [nlut] int64 | table [nlut] float
//          d = 64, four waves, radii 128 / 256 (nlut = 1283): 18432 + 9216 + 1536 + 10264 + 5132 = 44580 bytes
//   dK/dV  Q^T [D][72] T | dO^T [D][72] T | P^T [waves][16][72] T | dS^T [waves][16][72] T | query triples [3][64] int | table
//          the same case: 18432 + 18432 + 768 + 5132 = 42764 bytes
//
// The table gradient, with the same bits on every run.  Float atomics would make the sum depend on arrival order; integer addition
// is associative, so the sum is taken in fixed point:
//   * rg_norm_kernel: per head the maxima over all rows of ||dO row||^2 and ||V row||^2, as integer atomic max on the bit patterns
//     of non-negative floats.  M_h = 2 max||dO|| max||V||.  |dS| <= M_h: P <= 1, |dP| <= ||dO|| ||V||, |D| <= ||dO|| ||O|| and O is a
//     convex combination of V rows.
//   * the quantum of head h is q_h = 2^(E + 1 - shift), E = ceil(log2 M_h): |dS| / q_h <= 2^(shift - 1), one bit spare for the
//     roundings of M_h and of o.  shift = 61 - floor(log2(B Lq Lk)) on the host, so B Lq Lk 2^shift < 2^62 and a 64-bit sum of
//     B Lq Lk terms cannot overflow.  32 x 709 x 709 leaves shift = 38 bits below the bound; the check refuses B Lq Lk >= 2^32,
//     where fewer than 30 would remain.
//   * pass 2 of rg_dq_kernel converts every dS to int64 in units of q_h (ldexp is exact, the conversion is the one rounding) and
//     adds it at its three indices of the LDS histogram (ds_add_u64); at the end a workgroup adds its non-zero entries to the
//     [heads, nlut] int64 buffer in the workspace (64-bit integer atomics).  The entry zeroes that buffer with a kernel.
//   * rg_fold_kernel: dlut = (float)((double)count * q_h * scale).  M_h = 0: zeros.  A non-finite M_h (NaN or inf in dout or v) or a
//     dS that is NaN or past the bound (NaN in q or k, an `o` that is not the forward's) makes the head's whole row NaN: decided from
//     M_h and a flag word, never from an integer conversion of such a value.
// One histogram serves the workgroup; a copy per 16-lane group (against same-address serialisation) is not built.
//
// Rounding points: attention_grad16.h's, with the bias added to the instruction's fp32 sum before the product with scale.
#include <algorithm>

#include "attention_grad16.h"
#include "relpos.h"

namespace vk {

constexpr int RG_MIN_SHIFT = 30;        // bits below the bound the size rule keeps

struct RelGradArgs {
    AttGrad16Args a;
    const int32_t *rel_q, *rel_k;
    const float *lut;
    float *dlut;
    long long *hist;        // [heads][nlut]
    unsigned *norm2;        // [2][heads]: bits of max ||dout row||^2, max ||v row||^2
    unsigned *bad;          // [heads]: nonzero where a dS was NaN or past the bound
    int r1, r2, shift;
};

static size_t rg_stats_bytes(int B, int heads, int Lq) { return align_up(ag16_workspace_bytes(B, heads, Lq), 8); }
static size_t rg_fixed_words(int heads, int nlut) { return (size_t)heads * nlut + ((size_t)3 * heads + 1) / 2; }      // of 8 bytes
static size_t rg_workspace_bytes(int B, int heads, int Lq, int r1, int r2) {
    if (B < 1 || heads < 1 || Lq < 1 || r1 < 1 || r2 < 1) return 0;
    return rg_stats_bytes(B, heads, Lq) + 8 * rg_fixed_words(heads, relpos_lut_len(r1, r2));
}

__global__ __launch_bounds__(256) void rg_zero_kernel(unsigned long long *p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// norm2[which][h] = max over the rows of ||row, head h||^2 (which 0: dout, 1: v): a thread per row, a wave's maximum by shuffles,
// one integer atomic max per wave.  A NaN's pattern lies above every finite one.
template <typename T, int D>
__global__ __launch_bounds__(256) void rg_norm_kernel(const T *__restrict__ dout, long lddo, long rows_do, const T *__restrict__ v, long ldv,
                                                     long rows_v, int heads, unsigned *__restrict__ norm2) {
    typedef typename Mma16<T>::frag frag;
    const int which = blockIdx.z, h = blockIdx.y;
    const T *src = which ? v : dout;
    const long ld = which ? ldv : lddo, rows = which ? rows_v : rows_do;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    if (r < rows) {
        const T *p = src + r * ld + h * D;
#pragma unroll
        for (int c = 0; c < D / 8; ++c) {
            const frag t = *reinterpret_cast<const frag *>(p + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf((float)t[e], (float)t[e], s);
        }
    }
    unsigned bits = __float_as_uint(s) & 0x7fffffffu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o, 64));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(norm2 + which * heads + h, bits);
}

// M_h and E = ceil(log2 M_h); false where M_h is zero or not finite (no histogram is taken)
__device__ __forceinline__ bool rg_bound(const unsigned *norm2, int heads, int h, float *M, int *E) {
    const float m = 2.f * sqrtf(__uint_as_float(norm2[h])) * sqrtf(__uint_as_float(norm2[heads + h]));
    *M = m;
    *E = 0;
    if (!(m > 0.f) || !(m <= 3.402823466e38f)) return false;
    int e;
    const float f = frexpf(m, &e);          // m = f 2^e, f in [1/2, 1)
    *E = f == 0.5f ? e - 1 : e;
    return true;
}

template <typename T, int D, bool HIST>
__global__ __launch_bounds__(256) void rg_dq_kernel(RelGradArgs r, int nrun) {
    const AttGrad16Args &a = r.a;
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = ATT_KT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
    const int bh = blockIdx.x / nrun, run = blockIdx.x - bh * nrun;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int q0 = (run * nw + wave) * AG16_OWN;
    const int nq = a.Lq - q0;                       // owned rows inside the sequence: 16 or more (all), or none (an idle wave)
    const int n1 = 2 * r.r1 + 1, n2 = 2 * r.r2 + 1, nlut = n1 + 2 * n2;
    T *kt0 = reinterpret_cast<T *>(rg_lds), *dsi = kt0 + 2 * D * ATT_PP + wave * (AG16_OWN * ATT_PP);
    int *kr0 = reinterpret_cast<int *>(kt0 + 2 * D * ATT_PP + nw * (AG16_OWN * ATT_PP));
    unsigned long long *hs = reinterpret_cast<unsigned long long *>(kr0 + 2 * 3 * ATT_KT);
    float *t1s = reinterpret_cast<float *>(hs + nlut), *txs = t1s + n1, *tys = txs + n2;
    const T *qseq = static_cast<const T *>(a.q) + (long)b * a.Lq * a.ldq + h * D;
    const T *doseq = static_cast<const T *>(a.dout) + (long)b * a.Lq * a.lddo + h * D;
    const T *oseq = static_cast<const T *>(a.o) + (long)b * a.Lq * a.ldo + h * D;
    const T *kbase = static_cast<const T *>(a.k) + (long)b * a.Lk * a.ldk + h * D;
    const T *vbase = static_cast<const T *>(a.v) + (long)b * a.Lk * a.ldv + h * D;
    const float *mrow = a.mask ? a.mask + (long)b * a.Lk : nullptr;
    const int32_t *relk = r.rel_k + (long)b * a.Lk * 3;

    for (int i = tid; i < nlut; i += nthr) {
        t1s[i] = r.lut[(long)h * nlut + i];
        if (HIST) hs[i] = 0;
    }
    frag qf[KD], dof[KD];
    att_row_frags<T, KD>(qf, qseq, a.ldq, q0 + j, a.Lq, g);
    att_row_frags<T, KD>(dof, doseq, a.lddo, q0 + j, a.Lq, g);
    int qp[4], qx[4], qy[4];
    att_lane_triples(qp, qx, qy, r.rel_q + (long)b * a.Lq * 3, q0 + 4 * g, a.Lq);

    // ---- pass 1: m and l of rows 4 g + e, online over the key tiles; the next tile's triples go into the other buffer ----
    float m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = -INFINITY;
        l[e] = 0.f;
    }
    att_stage_triples(kr0, relk, 0, a.Lk, tid);
    int buf = 0;
    for (int k0 = 0; k0 < a.Lk; k0 += ATT_KT, buf ^= 1) {
        __syncthreads();            // this tile's triples (first tile: the table too) are in LDS; the other buffer is free
        if (k0 + ATT_KT < a.Lk) att_stage_triples(kr0 + (buf ^ 1) * (3 * ATT_KT), relk, k0 + ATT_KT, a.Lk, tid);
        const int *kr = kr0 + buf * (3 * ATT_KT);
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
            const int kp = kr[kb * 16 + j], kx = kr[ATT_KT + kb * 16 + j], ky = kr[2 * ATT_KT + kb * 16 + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t1 = t1s[rp_idx(kp, qp[e], r.r1)], tx = txs[rp_idx(kx, qx[e], r.r2)], ty = tys[rp_idx(ky, qy[e], r.r2)];
                s[e] = ok ? rp_score(s[e], t1, tx, ty, a.scale, mk) : -INFINITY;
            }
            sc[kb] = s;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) att_online_row(sc, e, m[e], l[e]);
    }
    float il[4], dd[4];
    frag of[KD];
    att_row_frags<T, KD>(of, oseq, a.ldo, q0 + j, a.Lq, g);
    att_grad_d<T, KD>(dd, il, dof, of, l, g);
    att_store_stats(a.stats, (long)a.B * a.heads * a.Lq, (long)bh * a.Lq + q0, nq, m, il, dd, g, j);

    // ---- pass 2: dS -> the histogram and dQ ----
    float M = 0.f, lim = 0.f;
    int E = 0;
    bool hist_on = false, bad = false;
    if (HIST) {
        hist_on = rg_bound(r.norm2, a.heads, h, &M, &E);
        lim = ldexpf(1.f, E);                        // >= M_h; finite, or the head is flagged through M_h
    }
    const int sh = r.shift - 1 - E;
    m16_f4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();                // every wave is past pass 1's last triples
    att_image_t_wg<T, D>(kt0, kbase, a.ldk, 0, a.Lk, tid, nthr);
    att_stage_triples(kr0, relk, 0, a.Lk, tid);
    buf = 0;
    for (int k0 = 0; k0 < a.Lk; k0 += ATT_KT, buf ^= 1) {
        __syncthreads();            // this tile's K^T image and triples are in LDS
        const int *kr = kr0 + buf * (3 * ATT_KT);
        const T *kt = kt0 + buf * (D * ATT_PP);
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
            const int kp = kr[kb * 16 + j], kx = kr[ATT_KT + kb * 16 + j], ky = kr[2 * ATT_KT + kb * 16 + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float dsv = 0.f;
                if (okk && 4 * g + e < nq) {
                    const int i1 = rp_idx(kp, qp[e], r.r1), ix = rp_idx(kx, qx[e], r.r2), iy = rp_idx(ky, qy[e], r.r2);
                    const float sb = rp_score(s[e], t1s[i1], txs[ix], tys[iy], a.scale, mk);
                    dsv = att_exp(sb - m[e]) * il[e] * (dp[e] - dd[e]);
                    if (HIST && hist_on) {
                        if (!(fabsf(dsv) <= lim)) {
                            bad = true;
                        } else if (dsv != 0.f) {
                            const unsigned long long c = (unsigned long long)__float2ll_rn(ldexpf(dsv, sh));
                            atomicAdd(hs + i1, c);
                            atomicAdd(hs + n1 + ix, c);
                            atomicAdd(hs + n1 + n2 + iy, c);
                        }
                    }
                }
                dsi[(4 * g + e) * ATT_PP + kb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();            // dS is written; every wave is past the previous tile's product, whose buffer is free
        if (k0 + ATT_KT < a.Lk) {
            att_image_t_wg<T, D>(kt0 + (buf ^ 1) * (D * ATT_PP), kbase, a.ldk, k0 + ATT_KT, a.Lk, tid, nthr);
            att_stage_triples(kr0 + (buf ^ 1) * (3 * ATT_KT), relk, k0 + ATT_KT, a.Lk, tid);
        }
        att_image_mma<T, NDB>(acc, dsi, kt, g, j);
    }
    att_store_rows<NDB>(a.dq + ((long)b * a.Lq + q0) * a.lddq + h * D, a.lddq, acc, a.scale, nq, g, j);
    if (HIST) {
        if (bad) atomicOr(r.bad + h, 1u);
        __syncthreads();            // every wave's histogram adds are done
        unsigned long long *out = reinterpret_cast<unsigned long long *>(r.hist) + (long)h * nlut;
        for (int i = tid; i < nlut; i += nthr) {
            const unsigned long long c = hs[i];
            if (c) atomicAdd(out + i, c);
        }
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rg_dkv_kernel(RelGradArgs r, int nrun) {
    const AttGrad16Args &a = r.a;
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, QB = ATT_KT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
    const int bh = blockIdx.x / nrun, run = blockIdx.x - bh * nrun;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int j0 = (run * nw + wave) * AG16_OWN;
    const int nk = a.Lk - j0;                       // owned keys inside the sequence: 16 or more (all), or none (an idle wave)
    const int n1 = 2 * r.r1 + 1, n2 = 2 * r.r2 + 1, nlut = n1 + 2 * n2;
    T *qt = reinterpret_cast<T *>(rg_lds), *dot = qt + D * ATT_PP;
    T *pt = dot + D * ATT_PP + wave * (2 * AG16_OWN * ATT_PP), *dst = pt + AG16_OWN * ATT_PP;
    int *qr = reinterpret_cast<int *>(dot + D * ATT_PP + nw * (2 * AG16_OWN * ATT_PP));
    float *t1s = reinterpret_cast<float *>(qr + 3 * ATT_KT), *txs = t1s + n1, *tys = txs + n2;
    const T *qbase = static_cast<const T *>(a.q) + (long)b * a.Lq * a.ldq + h * D;
    const T *dobase = static_cast<const T *>(a.dout) + (long)b * a.Lq * a.lddo + h * D;
    const T *kseq = static_cast<const T *>(a.k) + (long)b * a.Lk * a.ldk + h * D;
    const T *vseq = static_cast<const T *>(a.v) + (long)b * a.Lk * a.ldv + h * D;
    const long n = (long)a.B * a.heads * a.Lq;
    const float *st = a.stats + (long)bh * a.Lq;
    const int32_t *relq = r.rel_q + (long)b * a.Lq * 3;

    for (int i = tid; i < nlut; i += nthr) t1s[i] = r.lut[(long)h * nlut + i];
    frag kf[KD], vf[KD];
    att_row_frags<T, KD>(kf, kseq, a.ldk, j0 + j, a.Lk, g);
    att_row_frags<T, KD>(vf, vseq, a.ldv, j0 + j, a.Lk, g);
    float mk[4];
    int kp[4], kx[4], ky[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) mk[e] = a.mask && j0 + 4 * g + e < a.Lk ? a.mask[(long)b * a.Lk + j0 + 4 * g + e] : 0.f;
    att_lane_triples(kp, kx, ky, r.rel_k + (long)b * a.Lk * 3, j0 + 4 * g, a.Lk);

    m16_f4 acck[NDB], accv[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acck[db] = accv[db] = m16_f4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < a.Lq; q0 += ATT_KT) {
        att_image_t_wg<T, D>(qt, qbase, a.ldq, q0, a.Lq, tid, nthr);
        att_image_t_wg<T, D>(dot, dobase, a.lddo, q0, a.Lq, tid, nthr);
        att_stage_triples(qr, relq, q0, a.Lq, tid);
        __syncthreads();            // the tile's images and triples (first tile: the table too) are in LDS
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int row = q0 + qb * 16 + j;
            const bool okq = row < a.Lq;
            frag qf[KD], dof[KD];
            att_row_frags<T, KD>(qf, qbase, a.ldq, row, a.Lq, g);
            att_row_frags<T, KD>(dof, dobase, a.lddo, row, a.Lq, g);
            m16_f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KD; ++ks) {
                s = Mma16<T>::mma(kf[ks], qf[ks], s);
                dp = Mma16<T>::mma(vf[ks], dof[ks], dp);
            }
            const float mm = okq ? st[row] : 0.f, il = okq ? st[n + row] : 0.f, dd = okq ? st[2 * n + row] : 0.f;
            const int qp = qr[qb * 16 + j], qx = qr[ATT_KT + qb * 16 + j], qy = qr[2 * ATT_KT + qb * 16 + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p = 0.f, dsv = 0.f;
                if (okq && 4 * g + e < nk) {
                    const float t1 = t1s[rp_idx(kp[e], qp, r.r1)], tx = txs[rp_idx(kx[e], qx, r.r2)], ty = tys[rp_idx(ky[e], qy, r.r2)];
                    p = att_exp(rp_score(s[e], t1, tx, ty, a.scale, mk[e]) - mm) * il;
                    dsv = p * (dp[e] - dd);
                }
                pt[(4 * g + e) * ATT_PP + qb * 16 + j] = (T)p;
                dst[(4 * g + e) * ATT_PP + qb * 16 + j] = (T)dsv;
            }
        }
        __syncthreads();            // P^T and dS^T are written
        att_image_mma<T, NDB>(accv, pt, dot, g, j);
        att_image_mma<T, NDB>(acck, dst, qt, g, j);
        __syncthreads();            // the next tile overwrites the images and the triples
    }
    att_store_rows<NDB>(a.dk + ((long)b * a.Lk + j0) * a.lddk + h * D, a.lddk, acck, a.scale, nk, g, j);
    att_store_rows<NDB>(a.dv + ((long)b * a.Lk + j0) * a.lddv + h * D, a.lddv, accv, 1.f, nk, g, j);
}

// dlut[h][e] = (double)count * q_h * scale, rounded once to fp32; NaN rows where M_h is not finite or a dS was refused
__global__ __launch_bounds__(256) void rg_fold_kernel(const long long *__restrict__ hist, const unsigned *__restrict__ norm2,
                                                     const unsigned *__restrict__ bad, int heads, int nlut, int shift, float scale,
                                                     float *__restrict__ dlut) {
    const int h = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nlut) return;
    float M;
    int E;
    const bool on = rg_bound(norm2, heads, h, &M, &E);
    float out = 0.f;
    if (bad[h] || (!on && !(M == 0.f))) out = __uint_as_float(0x7fc00000u);
    else if (on) out = (float)(ldexp((double)hist[(long)h * nlut + i], E + 1 - shift) * (double)scale);
    dlut[(long)h * nlut + i] = out;
}

// dw[h][bucket] (+)= the fp64 sum, in ascending entry order, of the entries of dlut[h][off .. off + n) whose bucket it is.  A thread
// per (head, bucket) walks all n entries and re-reads the map (the threads of a wave read the same word): O(n) each, which at
// 12 heads x 64 buckets x 513 entries is one short launch a layer; an entry whose bucket lies outside [0, bins) reaches no thread.
__global__ __launch_bounds__(256) void relpos_lut_grad_kernel(const float *__restrict__ dlut, int ld, int off, int n,
                                                             const int32_t *__restrict__ bucket, int bins, int heads, int accumulate,
                                                             float *__restrict__ dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= heads * bins) return;
    const int h = i / bins, bk = i - h * bins;
    const float *row = dlut + (long)h * ld + off;
    double s = 0.0;
    for (int e = 0; e < n; ++e)
        if (bucket[off + e] == bk) s += (double)row[e];
    dw[i] = accumulate ? (float)((double)dw[i] + s) : (float)s;
}

static int rg_shift(int B, int Lq, int Lk) {
    const unsigned __int128 n = (unsigned __int128)B * (unsigned)Lq * (unsigned)Lk;
    if (n >> 32) return -1;
    int fl = 0;
    while ((n >> (fl + 1)) != 0) ++fl;
    return 61 - fl;
}

// everything the launch refuses, without touching a device or reading through a pointer
static int rg_check(const AttGrad16Args &a, const int32_t *rel_q, const int32_t *rel_k, const float *lut, int r1, int r2, const float *dlut,
                    int d, vk_dtype dt, const void *workspace, size_t workspace_bytes) {
    VK_TRY(ag16_check(a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.o, a.ldo, a.dout, a.lddo, a.dq, a.lddq, a.dk, a.lddk, a.dv, a.lddv, a.B, a.heads,
                      a.Lq, a.Lk, d, dt, workspace, workspace_bytes));
    VK_REQUIRE(rel_q && rel_k && lut && dlut, VK_EINVAL, "attention_relpos_grad: null argument");
    VK_TRY(relpos_lut_check("attention_relpos_grad", r1, r2));
    VK_REQUIRE(((uintptr_t)rel_q | (uintptr_t)rel_k | (uintptr_t)lut | (uintptr_t)dlut | (uintptr_t)a.mask) % 4 == 0, VK_EINVAL,
               "attention_relpos_grad: rel_q, rel_k, lut, dlut and mask must be 4-byte aligned");
    VK_REQUIRE(rg_shift(a.B, a.Lq, a.Lk) >= RG_MIN_SHIFT, VK_EINVAL,
               "attention_relpos_grad: B * Lq * Lk = %d * %d * %d is 2^32 or more: the fixed-point sum of the table gradient would keep "
               "fewer than %d bits; split the batch",
               a.B, a.Lq, a.Lk, RG_MIN_SHIFT);
    const size_t need = rg_workspace_bytes(a.B, a.heads, a.Lq, r1, r2);
    VK_REQUIRE(workspace_bytes >= need, VK_EINVAL, "attention_relpos_grad: needs a workspace of %zu bytes, got %zu", need, workspace_bytes);
    VK_REQUIRE(((uintptr_t)workspace & 7) == 0, VK_EINVAL, "attention_relpos_grad: the workspace must be 8-byte aligned");
    return VK_OK;
}

static size_t rg_dq_lds(int D, int waves, int nlut) {
    return (size_t)(2 * D + waves * AG16_OWN) * ATT_PP * 2 + (size_t)2 * 3 * ATT_KT * sizeof(int) + (size_t)nlut * 12;
}
static size_t rg_dkv_lds(int D, int waves, int nlut) {
    return (size_t)(2 * D + 2 * waves * AG16_OWN) * ATT_PP * 2 + (size_t)3 * ATT_KT * sizeof(int) + (size_t)nlut * 4;
}

template <typename T, int D>
static int rg_launch(const RelGradArgs &r, hipStream_t s) {
    const AttGrad16Args &a = r.a;
    const int nlut = relpos_lut_len(r.r1, r.r2);
    const long words = (long)rg_fixed_words(a.heads, nlut);
    hipLaunchKernelGGL(rg_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(r.hist),
                       words);
    VK_CHECK_HIP(hipGetLastError());
    const long rows_do = (long)a.B * a.Lq, rows_v = (long)a.B * a.Lk;
    hipLaunchKernelGGL((rg_norm_kernel<T, D>), dim3((unsigned)((std::max(rows_do, rows_v) + 255) / 256), a.heads, 2), dim3(256), 0, s,
                       static_cast<const T *>(a.dout), a.lddo, rows_do, static_cast<const T *>(a.v), a.ldv, rows_v, a.heads, r.norm2);
    VK_CHECK_HIP(hipGetLastError());
    const int wq = std::min(ATT_MAXW, ceil_div(a.Lq, AG16_OWN)), wk = std::min(ATT_MAXW, ceil_div(a.Lk, AG16_OWN));
    const int nrq = ceil_div(a.Lq, wq * AG16_OWN), nrk = ceil_div(a.Lk, wk * AG16_OWN);
    const size_t capq = rg_dq_lds(D, ATT_MAXW, 0) + RELPOS_LUT_MAX * 3, capk = rg_dkv_lds(D, ATT_MAXW, 0) + RELPOS_LUT_MAX;
#ifdef VK_ABLATION
    if (env_off("VK_RELPOS_GRAD_HIST"))             // tools only: the launches without the table gradient (dlut is zeros)
        VK_TRY(launch_lds(rg_dq_kernel<T, D, false>, dim3(a.B * a.heads * nrq), dim3(64 * wq), rg_dq_lds(D, wq, nlut), capq, s, r, nrq));
    else
#endif
    VK_TRY(launch_lds(rg_dq_kernel<T, D, true>, dim3(a.B * a.heads * nrq), dim3(64 * wq), rg_dq_lds(D, wq, nlut), capq, s, r, nrq));
    VK_TRY(launch_lds(rg_dkv_kernel<T, D>, dim3(a.B * a.heads * nrk), dim3(64 * wk), rg_dkv_lds(D, wk, nlut), capk, s, r, nrk));
    hipLaunchKernelGGL(rg_fold_kernel, dim3(ceil_div(nlut, 256), a.heads), dim3(256), 0, s, r.hist, r.norm2, r.bad, a.heads, nlut, r.shift,
                       a.scale, r.dlut);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

size_t vk_attention_relpos_grad_workspace_bytes(int B, int heads, int Lq, int r1, int r2) { return rg_workspace_bytes(B, heads, Lq, r1, r2); }

int vk_attention_relpos_grad_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask,
                                   const int32_t *rel_q, const int32_t *rel_k, const float *lut, int r1, int r2, const void *o, long ldo,
                                   const void *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk, const float *dv,
                                   long lddv, const float *dlut, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, const void *workspace,
                                   size_t workspace_bytes) {
    const AttGrad16Args a = {q, k, v, o, dout, mask, (float *)dq, (float *)dk, (float *)dv, nullptr, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                             B, heads, Lq, Lk, 0.f};
    return rg_check(a, rel_q, rel_k, lut, r1, r2, dlut, d, dt, workspace, workspace_bytes);
}

int vk_attention_relpos_grad(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const int32_t *rel_q,
                             const int32_t *rel_k, const float *lut, int r1, int r2, const void *o, long ldo, const void *dout, long lddo,
                             float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, float *dlut, int B, int heads, int Lq, int Lk,
                             int d, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream) {
    RelGradArgs r = {{q, k, v, o, dout, mask, dq, dk, dv, (float *)workspace, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, B, heads, Lq, Lk,
                      1.0f / sqrtf((float)d)},
                     rel_q, rel_k, lut, dlut, nullptr, nullptr, nullptr, r1, r2, 0};
    VK_TRY(rg_check(r.a, rel_q, rel_k, lut, r1, r2, dlut, d, dt, workspace, workspace_bytes));
    const int nlut = relpos_lut_len(r1, r2);
    r.hist = reinterpret_cast<long long *>(static_cast<char *>(workspace) + rg_stats_bytes(B, heads, Lq));
    r.norm2 = reinterpret_cast<unsigned *>(r.hist + (size_t)heads * nlut);
    r.bad = r.norm2 + 2 * heads;
    r.shift = rg_shift(B, Lq, Lk);
    VK_DT16_D_SWITCH(dt, d, return rg_launch<T, D>(r, (hipStream_t)stream));
}

int vk_relpos_lut_grad(const float *dlut, int heads, int r1, int r2, int term, const int32_t *bucket, int bins, float *dweight,
                       int accumulate, void *stream) {
    VK_REQUIRE(dlut && bucket && dweight, VK_EINVAL, "relpos_lut_grad: null argument");
    VK_REQUIRE(heads >= 1 && r1 >= 1 && r2 >= 1 && bins >= 1, VK_EINVAL, "relpos_lut_grad: sizes must be positive (heads=%d r1=%d r2=%d bins=%d)",
               heads, r1, r2, bins);
    VK_REQUIRE(((uintptr_t)dlut | (uintptr_t)bucket | (uintptr_t)dweight) % 4 == 0, VK_EINVAL,
               "relpos_lut_grad: dlut, bucket and dweight must be 4-byte aligned");
    VK_REQUIRE(term >= 0 && term <= 2, VK_EINVAL, "relpos_lut_grad: term %d is none of 0 (1-D), 1 (x), 2 (y)", term);
    VK_REQUIRE((long)heads * bins < (1L << 31), VK_EINVAL, "relpos_lut_grad: too many (head, bucket) items");
    const int n1 = 2 * r1 + 1, n2 = 2 * r2 + 1;
    const int off = term == 0 ? 0 : n1 + (term - 1) * n2, n = term == 0 ? n1 : n2;
    hipLaunchKernelGGL(relpos_lut_grad_kernel, dim3(ceil_div(heads * bins, 256)), dim3(256), 0, (hipStream_t)stream, dlut, n1 + 2 * n2, off, n,
                       bucket, bins, heads, accumulate ? 1 : 0, dweight);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
