// attention_stream_kernel, the strict online-soft-max attention: every type, head dim <= 256, any alignment, fp32 FMAs over fp32 LDS
// tiles, P not rounded.  attention.hip instantiates the plain form, attention_relpos.hip the BIAS form (LayoutLMv3's position bias,
// relpos.h): a kernel is instantiated in one unit only.
#pragma once
#include "attention_mma.h"
#include "relpos.h"

namespace vk {

// One workgroup per (batch, head, block of 16 queries).  The Q block and a 64-key K / V tile are staged in LDS as fp32 (K and Q
// rows padded by one float, as attention_kernel pads them); 256 threads share the 16 x 64 scores, a wave owns every fourth
// row's running maximum and sum, then a thread owns up to 16 of the 16 x d outputs in registers across the tiles.
// BIAS (the one trailing argument is a RelBias): a score is rp_score's; beside the rest in LDS lie the 16 query triples, the tile's
// 64 key triples and the head's table.  BIAS = false has no trailing argument.
constexpr int STR_QB = 16, STR_MAXD = 256;
constexpr int STR_OUT = STR_QB * STR_MAXD / 256;          // outputs per thread at the largest head dim

// the plain form's LDS; the BIAS form adds the triples and a table of nlut floats
static size_t stream_lds_bytes(int d) {
    return ((size_t)(STR_QB + ATT_KT) * (d + 1) + (size_t)ATT_KT * d + (size_t)STR_QB * (ATT_KT + 1) + 3 * STR_QB) * sizeof(float);
}
static size_t stream_bias_lds_bytes(int d, int nlut) { return stream_lds_bytes(d) + (size_t)(3 * (STR_QB + ATT_KT) + nlut) * sizeof(float); }

template <typename T, bool BIAS, typename... RA>
__global__ __launch_bounds__(256) void attention_stream_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                              const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                              T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int d, int nqb,
                                                              float scale, RA... rel) {
    static_assert(sizeof...(RA) == (BIAS ? 1 : 0), "a RelBias behind the arguments of the BIAS form, nothing otherwise");
    const RelBias rb = rel_bias_of(rel...);
    extern __shared__ float str_lds[];
    const int dp = d + 1, lp = ATT_KT + 1;
    const int n1 = 2 * rb.r1 + 1, n2 = 2 * rb.r2 + 1, nlut = n1 + 2 * n2;
    float *qs = str_lds, *ks = qs + STR_QB * dp, *vs = ks + ATT_KT * dp, *ps = vs + ATT_KT * d, *ms = ps + STR_QB * lp,
          *ls = ms + STR_QB, *as = ls + STR_QB;
    int *qr = reinterpret_cast<int *>(as + STR_QB), *kr = qr + 3 * STR_QB;                       // BIAS only, as the table
    float *t1s = reinterpret_cast<float *>(kr + 3 * ATT_KT), *txs = t1s + n1, *tys = txs + n2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bh = blockIdx.x / nqb, q0 = (blockIdx.x - bh * nqb) * STR_QB;
    const int b = bh / heads, h = bh - b * heads;
    const int nq = min(STR_QB, Lq - q0);
    for (int i = tid; i < STR_QB * d; i += 256) {
        const int r = i / d, c = i - r * d;
        qs[r * dp + c] = r < nq ? ldf(q + ((long)b * Lq + q0 + r) * ldq + h * d + c) : 0.f;
    }
    if constexpr (BIAS) {
        for (int i = tid; i < nlut; i += 256) t1s[i] = rb.lut[(long)h * nlut + i];
        if (tid < 3 * STR_QB) qr[tid] = tid / 3 < nq ? rb.rel_q[((long)b * Lq + q0) * 3 + tid] : 0;
    }
    if (tid < STR_QB) {
        ms[tid] = -INFINITY;
        ls[tid] = 0.f;
    }
    float o[STR_OUT];
#pragma unroll
    for (int n = 0; n < STR_OUT; ++n) o[n] = 0.f;

    for (int k0 = 0; k0 < Lk; k0 += ATT_KT) {
        const int nk = min(ATT_KT, Lk - k0);
        for (int i = tid; i < ATT_KT * d; i += 256) {
            const int r = i / d, c = i - r * d;
            const bool ok = r < nk;
            ks[r * dp + c] = ok ? ldf(k + ((long)b * Lk + k0 + r) * ldk + h * d + c) : 0.f;
            vs[i] = ok ? ldf(v + ((long)b * Lk + k0 + r) * ldv + h * d + c) : 0.f;
        }
        if constexpr (BIAS) {
            if (tid < 3 * ATT_KT) kr[tid] = tid / 3 < nk ? rb.rel_k[((long)b * Lk + k0) * 3 + tid] : 0;
        }
        __syncthreads();
        for (int i = tid; i < STR_QB * ATT_KT; i += 256) {
            const int r = i / ATT_KT, jj = i - r * ATT_KT;
            float s = 0.f;
            for (int c = 0; c < d; ++c) s += qs[r * dp + c] * ks[jj * dp + c];
            if constexpr (BIAS) {           // the mask is read inside the sequence only
                const float t1 = t1s[rp_idx(kr[3 * jj], qr[3 * r], rb.r1)];
                const float tx = txs[rp_idx(kr[3 * jj + 1], qr[3 * r + 1], rb.r2)];
                const float ty = tys[rp_idx(kr[3 * jj + 2], qr[3 * r + 2], rb.r2)];
                ps[r * lp + jj] = jj < nk ? rp_score(s, t1, tx, ty, scale, mask ? mask[(long)b * Lk + k0 + jj] : 0.f) : -INFINITY;
            } else {
                ps[r * lp + jj] = jj < nk ? s * scale + (mask ? mask[(long)b * Lk + k0 + jj] : 0.f) : -INFINITY;
            }
        }
        __syncthreads();
        for (int r = wave; r < STR_QB; r += 4) {
            const float x = ps[r * lp + lane];
            const float mx = wave_max(x);
            const float mo = ms[r], mn = fmaxf(mo, mx);
            const float alpha = expf(mo - mn);                   // first tile: exp(-inf) = 0
            const float p = expf(x - mn);                        // padded keys: exp(-inf) = 0
            ps[r * lp + lane] = p;
            const float sum = wave_sum(p);
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
                for (int jj = 0; jj < ATT_KT; ++jj) acc += ps[r * lp + jj] * vs[jj * d + c];
                o[n] = acc;
            }
        }
        __syncthreads();            // the next tile overwrites K, V, the key triples and the scores
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

}  // namespace vk
