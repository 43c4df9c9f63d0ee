// Attention, softmax(Q K^T / sqrt(d) + mask) V per (batch, head), for the BERT-style encoders (LXMERT, VisualBERT, ViT): the four
// kernels, the pure routing function that picks one, one launcher, and the entry points vk_attention, vk_attention_tiled and
// vk_attention_route (DESIGN.md sections 19 and 20).  Restated from transformers/models/lxmert/modeling_lxmert.py (v5.15),
// LxmertAttention :217-266.
//
//   attention_kernel         f32 / f16 / bf16: Q, K and V of one head live in LDS as fp32 (whatever fits 160 KiB; fp32: strict mode)
//   attention_mfma_kernel    bf16 / f16, head dim 32 / 64, Lq <= 48, Lk <= 64: v_mfma_f32_16x16x32, one wave per (batch, head), the
//                            whole score matrix in registers
//   attention_tiled_kernel   bf16 / f16, head dim 32 / 64, any Lq, Lk: v_mfma_f32_16x16x32, one wave per (batch, head, block of
//                            16 or 32 queries), 64-key tiles, P rounded to the storage type for the second product
//   attention_stream_kernel  f32 / f16 / bf16, head dim <= 256, any alignment: fp32 FMAs over fp32 LDS tiles, P not rounded
//
// The last two are the online-soft-max forms of the first two.  They keep scores, running maximum m, running sum l and O in fp32:
// per tile m' = max(m, rowmax), a = exp(m - m'), p = exp(s - m'), O = a O + p V, l = a l + sum p; the output is O / l (a true
// division), rounded once.  A padding key of the last tile scores -inf; no tile is all padding, so m is finite after the first tile
// (a masked key scores about finfo.min, which is finite).
#include <cstdlib>

#include "vk_common.h"

namespace vk {

// One workgroup per (batch b, head h).  Q, K, V of the head are staged in LDS as fp32 (rows padded by one float so
// that column walks do not collide on a bank); 256 threads share the Lq x Lk scores, one wave per row does the
// soft-max, then the threads share the Lq x d outputs.  Scores, soft-max and the weighted sum are fp32 (the
// reference matmuls and soft-maxes in the model dtype; the bf16-emulating oracle restates THIS kernel's rounding
// points: inputs and output only).
template <typename T>
__global__ __launch_bounds__(256) void attention_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                       const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                       T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int d, float scale) {
    extern __shared__ float sm[];
    const int dp = d + 1, lp = Lk + 1;
    float *qs = sm, *ks = qs + Lq * dp, *vs = ks + Lk * dp, *ps = vs + Lk * d;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, tid = threadIdx.x;
    constexpr int V = 16 / sizeof(T);
    typedef T vecT __attribute__((ext_vector_type(V)));
    if (d % V == 0 && ldq % V == 0 && ldk % V == 0 && ldv % V == 0) {       // 16-byte staging loads
        const int dv = d / V;
        for (int i = tid; i < Lk * dv; i += 256) {
            const int r = i / dv, c = (i - r * dv) * V;
            const vecT kk = *reinterpret_cast<const vecT *>(k + ((long)b * Lk + r) * ldk + h * d + c);
            const vecT vv = *reinterpret_cast<const vecT *>(v + ((long)b * Lk + r) * ldv + h * d + c);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                ks[r * dp + c + e] = (float)kk[e];
                vs[r * d + c + e] = (float)vv[e];
            }
        }
        for (int i = tid; i < Lq * dv; i += 256) {
            const int r = i / dv, c = (i - r * dv) * V;
            const vecT qq = *reinterpret_cast<const vecT *>(q + ((long)b * Lq + r) * ldq + h * d + c);
#pragma unroll
            for (int e = 0; e < V; ++e) qs[r * dp + c + e] = (float)qq[e];
        }
    } else {
        for (int i = tid; i < Lk * d; i += 256) {
            const int r = i / d, c = i - r * d;
            ks[r * dp + c] = ldf(k + ((long)b * Lk + r) * ldk + h * d + c);
            vs[i] = ldf(v + ((long)b * Lk + r) * ldv + h * d + c);
        }
        for (int i = tid; i < Lq * d; i += 256) {
            const int r = i / d, c = i - r * d;
            qs[r * dp + c] = ldf(q + ((long)b * Lq + r) * ldq + h * d + c);
        }
    }
    __syncthreads();
    for (int i = tid; i < Lq * Lk; i += 256) {
        const int r = i / Lk, j = i - r * Lk;
        float s = 0.f;
        for (int c = 0; c < d; ++c) s += qs[r * dp + c] * ks[j * dp + c];
        ps[r * lp + j] = s * scale + (mask ? mask[(long)b * Lk + j] : 0.f);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < Lq; r += 4) {
        float mx = -INFINITY;
        for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, ps[r * lp + j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float den = 0.f;
        for (int j = lane; j < Lk; j += 64) {
            const float e = expf(ps[r * lp + j] - mx);
            ps[r * lp + j] = e;
            den += e;
        }
        den = wave_sum(den);
        const float inv = 1.0f / den;
        for (int j = lane; j < Lk; j += 64) ps[r * lp + j] *= inv;
    }
    __syncthreads();
    for (int i = tid; i < Lq * d; i += 256) {
        const int r = i / d, c = i - r * d;
        float o = 0.f;
        for (int j = 0; j < Lk; ++j) o += ps[r * lp + j] * vs[j * d + c];
        stf(out + ((long)b * Lq + r) * ldo + h * d + c, o);
    }
}

// What attention_kernel needs of LDS for one head: the rule and the launch both ask here.
static size_t lds_kernel_bytes(int Lq, int Lk, int d) {
    return ((size_t)(Lq + Lk) * (d + 1) + (size_t)Lk * d + (size_t)Lq * (Lk + 1)) * sizeof(float);
}
constexpr size_t LDS_KERNEL_MAX = 160 * 1024;

// ---- the same attention on the matrix cores (bf16 / f16, head dim 32 or 64, Lq <= 48, Lk <= 64: the whole score matrix of
// LXMERT's usual 20 text and 36 visual tokens in registers; longer sequences run attention_tiled_kernel's online-soft-max form) ----
// One WAVE per (batch, head), four per workgroup.  S = Q K^T and O = P V are v_mfma_f32_16x16x32 tiles:
//   * Q and K rows are the A / B operand fragments as they lie in memory (8 consecutive head-dim elements per lane):
//     no staging at all for the first product;
//   * a score tile leaves a lane with S[q = 4g + e][key = j]: the soft-max over the keys of a row reduces over the
//     key blocks in registers and over the 16 lanes of a group with four shuffles; fp32 throughout;
//   * P (rounded to the storage type, as the reference's own bf16 matmul sees it) and V^T go through a per-wave LDS
//     image to become the second product's operands; padded keys carry P = 0 and V = 0.
typedef _Float16 att_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 att_b8 __attribute__((ext_vector_type(8)));
typedef float att_f4 __attribute__((ext_vector_type(4)));
template <typename T>
struct AttFrag;
template <>
struct AttFrag<_Float16> {
    typedef att_h8 type;
    static __device__ __forceinline__ att_f4 mma(att_h8 a, att_h8 b, att_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <>
struct AttFrag<__bf16> {
    typedef att_b8 type;
    static __device__ __forceinline__ att_f4 mma(att_b8 a, att_b8 b, att_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

constexpr int ATT_MAXQB = 3, ATT_MAXKB = 4;     // 48 queries, 64 keys
constexpr int ATT_PP = 72;                      // row pitch (elements) of the P and V^T images: 64 keys + 8 (bank skew)

template <typename T, int D>
__global__ __launch_bounds__(256) void attention_mfma_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                            const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                            T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int total,
                                                            float scale) {
    typedef typename AttFrag<T>::type frag;
    constexpr int KD = D / 32, NDB = D / 16;
    __shared__ __attribute__((aligned(16))) T lds[4][(48 + D) * ATT_PP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int pair = blockIdx.x * 4 + wave;
    const bool live = pair < total;
    const int pc = live ? pair : total - 1;             // idle waves redo the last pair (no early exit before the barrier)
    const int b = pc / heads, h = pc - b * heads;
    const int QB = (Lq + 15) >> 4, KB = (Lk + 15) >> 4, KS2 = (Lk + 31) >> 5;
    T *pt = lds[wave], *vt = pt + 48 * ATT_PP;
    const frag zf = {};

    // ---- operand fragments straight from memory ----
    frag qf[ATT_MAXQB][KD], kf[ATT_MAXKB][KD];
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb) {
        const int r = qb * 16 + j;
        const bool ok = qb < QB && r < Lq;
        const T *src = q + ((long)b * Lq + (ok ? r : 0)) * ldq + h * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KD; ++ks) {
            const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
            qf[qb][ks] = ok ? t : zf;
        }
    }
#pragma unroll
    for (int kb = 0; kb < ATT_MAXKB; ++kb) {
        const int r = kb * 16 + j;
        const bool ok = kb < KB && r < Lk;
        const T *src = k + ((long)b * Lk + (ok ? r : 0)) * ldk + h * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KD; ++ks) {
            const frag t = *reinterpret_cast<const frag *>(src + ks * 32);
            kf[kb][ks] = ok ? t : zf;
        }
    }
    // ---- V^T image: vt[d][key], zero for the padded keys ----
    {
        constexpr int CH = D / 8;                        // 16-byte chunks per V row
        for (int i = lane; i < KS2 * 32 * CH; i += 64) {
            const int key = i / CH, c = i - key * CH;
            frag t = zf;
            if (key < Lk) t = *reinterpret_cast<const frag *>(v + ((long)b * Lk + key) * ldv + h * D + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(c * 8 + e) * ATT_PP + key] = t[e];
        }
    }
    // ---- S = Q K^T * scale + mask ----
    att_f4 sc[ATT_MAXQB][ATT_MAXKB];
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb)
#pragma unroll
        for (int kb = 0; kb < ATT_MAXKB; ++kb) {
            att_f4 a = {0.f, 0.f, 0.f, 0.f};
            if (qb < QB && kb < KB) {
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = AttFrag<T>::mma(qf[qb][ks], kf[kb][ks], a);
            }
            const int key = kb * 16 + j;
            const float m = key < Lk ? (mask ? mask[(long)b * Lk + key] : 0.f) : -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = key < Lk ? a[e] * scale + m : -INFINITY;
            sc[qb][kb] = a;
        }
    // ---- soft-max over the keys of each row q = qb*16 + 4g + e: registers (kb), then the 16 lanes of the group ----
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb) {
        if (qb >= QB) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float mx = sc[qb][0][e];
#pragma unroll
            for (int kb = 1; kb < ATT_MAXKB; ++kb) mx = fmaxf(mx, sc[qb][kb][e]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            float den = 0.f;
#pragma unroll
            for (int kb = 0; kb < ATT_MAXKB; ++kb) {
                const float ex = expf(sc[qb][kb][e] - mx);       // padded keys: exp(-inf) = 0
                sc[qb][kb][e] = ex;
                den += ex;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) den += __shfl_xor(den, o, 64);
            const float inv = 1.0f / den;
            const int row = qb * 16 + g * 4 + e;
#pragma unroll
            for (int kb = 0; kb < ATT_MAXKB; ++kb) pt[row * ATT_PP + kb * 16 + j] = (T)(sc[qb][kb][e] * inv);
        }
    }
    __syncthreads();
    // ---- O = P V: A = P rows (keys contiguous), B = V^T rows (keys contiguous) ----
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb) {
        if (qb >= QB) continue;
        frag pf[2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) pf[k2] = *reinterpret_cast<const frag *>(pt + (qb * 16 + j) * ATT_PP + k2 * 32 + g * 8);
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            att_f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                if (k2 >= KS2) continue;
                const frag vf = *reinterpret_cast<const frag *>(vt + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
                o = AttFrag<T>::mma(pf[k2], vf, o);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = qb * 16 + g * 4 + e;
                if (live && row < Lq) out[((long)b * Lq + row) * ldo + h * D + db * 16 + j] = (T)o[e];
            }
        }
    }
}

// The tiled kernel's exponential: v_exp_f32 on x * log2(e).  Its error (about 1e-6 relative at a soft-max's arguments) is far
// below the rounding of P to a 16-bit type; exp(0) = 1 and exp(-inf) = 0 exactly, and a result below the normal range is 0.
static __device__ __forceinline__ float tat_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

constexpr int TAT_KT = 64;                      // keys per tile (four 16-key score blocks, two 32-key slices of the second product)

// One WAVE per (batch, head, block of QB * 16 queries), four per workgroup; the lane layouts are attention_mfma_kernel's:
//   * Q fragments of the block stay in registers; a tile's K rows are the B fragments as they lie in memory;
//   * a score tile leaves a lane with S[q = 4g + e][key = j]: row maximum and row sum reduce over the four key blocks in
//     registers and over the 16 lanes of a group with four shuffles;
//   * O's accumulator rows are the same 4g + e, so the rescale factor of a row is already in the lanes that hold it;
//   * P (rounded to T) and V^T go through a per-wave LDS image; a lane transposes two keys at a time (32-bit LDS writes,
//     consecutive lanes on consecutive words).  Padded keys carry P = 0 and V = 0.
// Every wave of a workgroup runs the same number of tiles (idle waves redo the last item and store nothing), so the
// barriers are uniform.
template <typename T, int D, int QB>
__global__ __launch_bounds__(256) void attention_tiled_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                             const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                             T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int nqb, int total,
                                                             float scale) {
    typedef typename AttFrag<T>::type frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = TAT_KT / 16, PER_WAVE = (QB * 16 + D) * ATT_PP;
    extern __shared__ __attribute__((aligned(16))) unsigned char tat_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int item = blockIdx.x * 4 + wave;
    const bool live = item < total;
    const int ic = live ? item : total - 1;
    const int bh = ic / nqb, q0 = (ic - bh * nqb) * (QB * 16);
    const int b = bh / heads, h = bh - b * heads;
    T *pt = reinterpret_cast<T *>(tat_lds) + wave * PER_WAVE, *vt = pt + QB * 16 * ATT_PP;
    unsigned *vt32 = reinterpret_cast<unsigned *>(vt);
    const frag zf = {};

    frag qf[QB][KD];
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
    }
    att_f4 o[QB][NDB];
    float m[QB][4], l[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[qb][db] = att_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[qb][e] = -INFINITY;
            l[qb][e] = 0.f;
        }
    }

    for (int k0 = 0; k0 < Lk; k0 += TAT_KT) {
        // ---- K fragments straight from memory ----
        frag kf[KB][KD];
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
        }
        // ---- V^T image of the tile: vt[d][key]; lane = (key pair, half of the 16-byte chunks of a row) ----
        {
            constexpr int CH = D / 8, HALF = CH / 2;
            const int kp = lane & 31, c0 = (lane >> 5) * HALF;
            const int key = k0 + 2 * kp;
#pragma unroll
            for (int it = 0; it < HALF; ++it) {
                const int c = c0 + it;
                frag t0 = zf, t1 = zf;
                if (key < Lk) t0 = *reinterpret_cast<const frag *>(v + ((long)b * Lk + key) * ldv + h * D + c * 8);
                if (key + 1 < Lk) t1 = *reinterpret_cast<const frag *>(v + ((long)b * Lk + key + 1) * ldv + h * D + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const T lo = t0[e], hi = t1[e];
                    unsigned short ulo, uhi;
                    __builtin_memcpy(&ulo, &lo, 2);
                    __builtin_memcpy(&uhi, &hi, 2);
                    vt32[((c * 8 + e) * ATT_PP) / 2 + kp] = (unsigned)ulo | ((unsigned)uhi << 16);
                }
            }
        }
        // ---- S = Q K^T * scale + mask; online soft-max; P image ----
        float mk[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int key = k0 + kb * 16 + j;
            mk[kb] = key < Lk ? (mask ? mask[(long)b * Lk + key] : 0.f) : -INFINITY;
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            att_f4 sc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                att_f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = AttFrag<T>::mma(qf[qb][ks], kf[kb][ks], a);
                const bool ok = k0 + kb * 16 + j < Lk;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = ok ? a[e] * scale + mk[kb] : -INFINITY;
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
                const float alpha = tat_exp(m[qb][e] - mn);      // first tile: exp(-inf) = 0
                float sum = 0.f;
                const int row = qb * 16 + g * 4 + e;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const float p = tat_exp(sc[kb][e] - mn);     // padded keys: exp(-inf) = 0
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
        __syncthreads();
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
                for (int qb = 0; qb < QB; ++qb) o[qb][db] = AttFrag<T>::mma(pf[qb], vf, o[qb][db]);
            }
        }
        __syncthreads();            // the next tile overwrites the images
    }
    if (!live) return;
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

// ---- the strict form ----
// One workgroup per (batch, head, block of 16 queries).  The Q block and a 64-key K / V tile are staged in LDS as fp32 (K and Q
// rows padded by one float, as attention_kernel pads them); 256 threads share the 16 x 64 scores, a wave owns every fourth
// row's running maximum and sum, then a thread owns up to 16 of the 16 x d outputs in registers across the tiles.
constexpr int STR_QB = 16, STR_KT = 64, STR_MAXD = 256;
constexpr int STR_OUT = STR_QB * STR_MAXD / 256;          // outputs per thread at the largest head dim

static size_t stream_lds_bytes(int d) {
    return ((size_t)(STR_QB + STR_KT) * (d + 1) + (size_t)STR_KT * d + (size_t)STR_QB * (STR_KT + 1) + 3 * STR_QB) * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(256) void attention_stream_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                              const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                              T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int d, int nqb,
                                                              float scale) {
    extern __shared__ float str_lds[];
    const int dp = d + 1, lp = STR_KT + 1;
    float *qs = str_lds, *ks = qs + STR_QB * dp, *vs = ks + STR_KT * dp, *ps = vs + STR_KT * d, *ms = ps + STR_QB * lp,
          *ls = ms + STR_QB, *as = ls + STR_QB;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bh = blockIdx.x / nqb, q0 = (blockIdx.x - bh * nqb) * STR_QB;
    const int b = bh / heads, h = bh - b * heads;
    const int nq = min(STR_QB, Lq - q0);
    for (int i = tid; i < STR_QB * d; i += 256) {
        const int r = i / d, c = i - r * d;
        qs[r * dp + c] = r < nq ? ldf(q + ((long)b * Lq + q0 + r) * ldq + h * d + c) : 0.f;
    }
    if (tid < STR_QB) {
        ms[tid] = -INFINITY;
        ls[tid] = 0.f;
    }
    float o[STR_OUT];
#pragma unroll
    for (int n = 0; n < STR_OUT; ++n) o[n] = 0.f;

    for (int k0 = 0; k0 < Lk; k0 += STR_KT) {
        const int nk = min(STR_KT, Lk - k0);
        for (int i = tid; i < STR_KT * d; i += 256) {
            const int r = i / d, c = i - r * d;
            const bool ok = r < nk;
            ks[r * dp + c] = ok ? ldf(k + ((long)b * Lk + k0 + r) * ldk + h * d + c) : 0.f;
            vs[i] = ok ? ldf(v + ((long)b * Lk + k0 + r) * ldv + h * d + c) : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < STR_QB * STR_KT; i += 256) {
            const int r = i / STR_KT, jj = i - r * STR_KT;
            float s = 0.f;
            for (int c = 0; c < d; ++c) s += qs[r * dp + c] * ks[jj * dp + c];
            ps[r * lp + jj] = jj < nk ? s * scale + (mask ? mask[(long)b * Lk + k0 + jj] : 0.f) : -INFINITY;
        }
        __syncthreads();
        for (int r = wave; r < STR_QB; r += 4) {
            const float x = ps[r * lp + lane];
            float mx = x;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            const float mo = ms[r], mn = fmaxf(mo, mx);
            const float alpha = expf(mo - mn);                   // first tile: exp(-inf) = 0
            const float p = expf(x - mn);                        // padded keys: exp(-inf) = 0
            ps[r * lp + lane] = p;
            float sum = p;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
            const float lo = ls[r];
            if (lane == 0) {
                ms[r] = mn;
                ls[r] = alpha * lo + sum;
                as[r] = alpha;
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < STR_OUT; ++n) {
            const int i = tid + 256 * n;
            if (i < STR_QB * d) {
                const int r = i / d, c = i - r * d;
                float acc = as[r] * o[n];
                for (int jj = 0; jj < STR_KT; ++jj) acc += ps[r * lp + jj] * vs[jj * d + c];
                o[n] = acc;
            }
        }
        __syncthreads();            // the next tile overwrites K, V and the scores
    }
#pragma unroll
    for (int n = 0; n < STR_OUT; ++n) {
        const int i = tid + 256 * n;
        if (i < STR_QB * d) {
            const int r = i / d, c = i - r * d;
            if (r < nq) out[((long)b * Lq + q0 + r) * ldo + h * d + c] = (T)(o[n] / ls[r]);
        }
    }
}

// The one routing rule (host only): the launcher switches on it for both entry points, vk_attention_route reports it.  The
// small matrix-core kernel takes 16-bit types, head dim 32 / 64, up to 48 queries and 64 keys, 16-byte aligned rows; the LDS
// kernel whatever fits 160 KiB; beyond that, and for every shape at the tiled entry, the online-soft-max kernels
// (VK_ATTENTION_MFMA=0, VK_ATTENTION_TILED=0).
static int attention_route(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16, int tiled_entry) {
    if (!(Lq >= 1 && Lk >= 1 && d >= 1)) {
        set_error("attention: bad geometry (Lq=%d Lk=%d d=%d)", Lq, Lk, d);
        return -VK_EINVAL;
    }
    if (!(dt == VK_F32 || dt == VK_F16 || dt == VK_BF16)) {
        set_error("attention: dtype must be f32, f16 or bf16");
        return -VK_EINVAL;
    }
    const bool mfma_ok = !env_off("VK_ATTENTION_MFMA") && (dt == VK_F16 || dt == VK_BF16) && (d == 32 || d == 64) && ldq % 8 == 0 &&
                         ldk % 8 == 0 && ldv % 8 == 0 && aligned16;
    int route;
    if (tiled_entry && !env_off("VK_ATTENTION_TILED"))
        route = mfma_ok ? VK_ATT_ROUTE_TILED : VK_ATT_ROUTE_STREAM;
    else if (mfma_ok && Lq <= 48 && Lk <= 64)
        route = VK_ATT_ROUTE_MFMA;
    else if (lds_kernel_bytes(Lq, Lk, d) <= LDS_KERNEL_MAX)
        route = VK_ATT_ROUTE_LDS;
    else
        route = mfma_ok ? VK_ATT_ROUTE_TILED : VK_ATT_ROUTE_STREAM;
    if (route == VK_ATT_ROUTE_STREAM && d > STR_MAXD) {
        set_error("attention: head dim %d is beyond the streaming kernel's limit of %d (Lq=%d Lk=%d)", d, STR_MAXD, Lq, Lk);
        return -VK_EINVAL;
    }
    return route;
}

// The arguments of vk_attention / vk_attention_tiled.
struct AttArgs {
    const void *q, *k, *v;
    const float *mask;
    void *out;
    int ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d;
    vk_dtype dt;
};
// the leading arguments every kernel takes, as T
#define VK_ATT_IO(T) (const T *)a.q, a.ldq, (const T *)a.k, a.ldk, (const T *)a.v, a.ldv, a.mask, (T *)a.out, a.ldo, a.heads, a.Lq, a.Lk

// what both entry points ask of their arguments before the rule sees them (which checks Lq, Lk, d and the dtype)
static int check_attention_args(const AttArgs &a) {
    VK_REQUIRE(a.q && a.k && a.v && a.out, VK_EINVAL, "attention: null argument");
    VK_REQUIRE(a.B > 0 && a.heads > 0, VK_EINVAL, "attention: bad geometry (B=%d heads=%d)", a.B, a.heads);
    return VK_OK;
}

static int route_of(const AttArgs &a, int tiled_entry) {
    const int aligned = ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) % 16 == 0;
    return attention_route(a.Lq, a.Lk, a.d, a.dt, a.ldq, a.ldk, a.ldv, aligned, tiled_entry);
}

template <typename T>
static int lds_launch(const AttArgs &a, float scale, hipStream_t s) {
    return launch_lds(attention_kernel<T>, dim3(a.B * a.heads), dim3(256), lds_kernel_bytes(a.Lq, a.Lk, a.d), LDS_KERNEL_MAX, s, VK_ATT_IO(T),
                      a.d, scale);
}

template <typename T, int D>
static int mfma_launch(const AttArgs &a, float scale, hipStream_t s) {
    const int total = a.B * a.heads;
    hipLaunchKernelGGL((attention_mfma_kernel<T, D>), dim3((total + 3) / 4), dim3(256), 0, s, VK_ATT_IO(T), total, scale);
    return VK_OK;
}

template <typename T, int D, int QB>
static int tiled_launch_qb(const AttArgs &a, float scale, hipStream_t s) {
    const int nqb = (a.Lq + QB * 16 - 1) / (QB * 16), total = a.B * a.heads * nqb;
    const size_t smem = (size_t)4 * (QB * 16 + D) * ATT_PP * sizeof(T);
    return launch_lds(attention_tiled_kernel<T, D, QB>, dim3((total + 3) / 4), dim3(256), smem, smem, s, VK_ATT_IO(T), nqb, total, scale);
}
template <typename T, int D>
static int tiled_launch(const AttArgs &a, float scale, hipStream_t s) {
    return a.Lq <= 16 ? tiled_launch_qb<T, D, 1>(a, scale, s) : tiled_launch_qb<T, D, 2>(a, scale, s);
}

template <typename T>
static int stream_launch(const AttArgs &a, float scale, hipStream_t s) {
    const int nqb = (a.Lq + STR_QB - 1) / STR_QB;
    return launch_lds(attention_stream_kernel<T>, dim3(a.B * a.heads * nqb), dim3(256), stream_lds_bytes(a.d), stream_lds_bytes(STR_MAXD), s,
                      VK_ATT_IO(T), a.d, nqb, scale);
}

// The one launcher: `route` is attention_route's answer for these arguments, so the dtype and the head dim are the kernel's.
static int launch_attention(int route, const AttArgs &a, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)a.d);
    VK_REQUIRE((long)a.B * a.heads * ((a.Lq + 15) / 16) < (1L << 31), VK_EINVAL, "attention: too many (batch, head, query block) items");
    const bool f16 = a.dt == VK_F16, d64 = a.d == 64;
    int st = VK_EINVAL;
    switch (route) {
        case VK_ATT_ROUTE_MFMA:
            st = f16 ? (d64 ? mfma_launch<_Float16, 64>(a, scale, s) : mfma_launch<_Float16, 32>(a, scale, s))
                     : (d64 ? mfma_launch<__bf16, 64>(a, scale, s) : mfma_launch<__bf16, 32>(a, scale, s));
            break;
        case VK_ATT_ROUTE_TILED:
            st = f16 ? (d64 ? tiled_launch<_Float16, 64>(a, scale, s) : tiled_launch<_Float16, 32>(a, scale, s))
                     : (d64 ? tiled_launch<__bf16, 64>(a, scale, s) : tiled_launch<__bf16, 32>(a, scale, s));
            break;
        case VK_ATT_ROUTE_LDS:
            st = a.dt == VK_F32 ? lds_launch<float>(a, scale, s) : f16 ? lds_launch<_Float16>(a, scale, s) : lds_launch<__bf16>(a, scale, s);
            break;
        case VK_ATT_ROUTE_STREAM:
            st = a.dt == VK_F32 ? stream_launch<float>(a, scale, s) : f16 ? stream_launch<_Float16>(a, scale, s) : stream_launch<__bf16>(a, scale, s);
            break;
        default: VK_REQUIRE(false, VK_EINVAL, "attention: route %d names no kernel", route);
    }
    VK_TRY(st);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}
#undef VK_ATT_IO

}  // namespace vk

using namespace vk;

extern "C" {

int vk_attention_route(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16, int tiled_entry) {
    return attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, aligned16, tiled_entry);
}

int vk_attention(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo, int B,
                 int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream) {
    const AttArgs a = {q, k, v, mask, out, ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d, dt};
    VK_TRY(check_attention_args(a));
    const int route = route_of(a, 0);
    if (route < 0) return -route;
    return launch_attention(route, a, (hipStream_t)stream);
}

// The same, with the rule asked as the tiled entry: the online-soft-max kernels at every shape (VK_ATTENTION_TILED=0: exactly
// vk_attention's choice).
int vk_attention_tiled(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo,
                       int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream) {
    const AttArgs a = {q, k, v, mask, out, ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d, dt};
    VK_TRY(check_attention_args(a));
    const int route = route_of(a, 1);
    if (route < 0) return -route;
    return launch_attention(route, a, (hipStream_t)stream);
}

}  // extern "C"
