// The backward of attention, O = softmax(Q K^T / sqrt(d) + mask) V per (batch, head), in fp32: what fine-tuning a BERT layer needs
// beside csrc/train.hip.  It differentiates the forward the library runs in fp32 (attention_kernel /
// attention_stream_kernel of attention.hip): the same score expression, and probabilities recomputed as expf(s - m) * (1 / l) from
// a row maximum m and a row sum l.  (attention_kernel forms P the same way; attention_stream_kernel divides its output by l
// instead, o / l, so there the recomputed P differs from the forward's implied one by the rounding of 1 / l.)  Three kernels, no atomics and no split accumulation: every output element has one writer
// and one fixed summation order, so the same input gives the same bits.
//
//   attgrad_stats_kernel   a workgroup per (batch, head, 16 queries) walks the keys 64 at a time exactly as attention_stream_kernel
//                          does (scores through LDS, a wave per row: m' = max(m, rowmax), l = exp(m - m') l + sum exp(s - m')), then
//                          writes m, 1 / l and D = sum_c dO[r, c] O[r, c] per row into the workspace
//   attgrad_dq_kernel      a workgroup owns 16 queries (Q, dO rows and their statistics in LDS) and walks the keys in order, 64 at
//                          a time (K, V tile in LDS): dS = p (dP - D) for the 16 x 64 tile through LDS, then a thread owns up to 8
//                          of the 16 x d elements of dQ in registers across the tiles.  dQ = scale * (the sum)
//   attgrad_dkv_kernel     the mirror image: a workgroup owns 16 keys (K, V rows in LDS) and walks the queries in order, 64 at a
//                          time (Q, dO and statistics in LDS); P^T and dS^T of the tile through LDS, a thread owns up to 8 elements
//                          of dK and of dV.  dV = the sum, dK = scale * (the sum)
//
// Tile: 16 owned rows x 64 walked rows, rows padded by one float: the pitch d + 1 (and 65 for the score images) is odd, so the 32
// lanes of a half-wave, which read 32 consecutive rows at one column with ds_read_b32 (bank = word % 32), hit 32 different
// banks; the owned row is one address for the wave, a broadcast.  LDS at d = 128: stats 46 KiB, dQ 87 KiB, dK/dV 91 KiB (one workgroup
// per CU); at d = 64: 25 / 46 / 50 KiB (three per CU).  fp32 FMAs throughout, as attention_stream_kernel: the fp32 matrix
// instruction runs at the vector rate on this chip.
//
// Rounding points (tests/finetune_util.py derives its bounds from them; u = 2^-24):
//   s        one fmaf chain over c ascending from 0, then fmaf(s, scale, mask)
//   m, l     as attention_stream_kernel: m exact; per 64-key tile alpha = expf(m_old - m_new), e = expf(s - m_new), the tile's sum in
//            the xor-shuffle tree over the 64 lanes, l = fmaf(alpha, l, sum); 1 / l is one division
//   p        expf(s - m) * (1 / l): the subtraction, expf (1 ulp) and the product round once each
//   D        lane c, c + 64, .. partial fmaf chains, then the xor-shuffle tree
//   dP       one fmaf chain over c;  dS = p * (dP - D): two roundings
//   dQ, dK, dV    one fmaf chain per element over the keys (queries) ascending; dQ and dK then one product with scale
// Integer data whose sums stay below 2^24 at a power-of-two key count and head dim is exact.
#include "vk_common.h"

namespace vk {

constexpr int AG_OWN = 16, AG_STEP = 64, AG_MAXD = 128;
constexpr int AG_ACC = AG_OWN * AG_MAXD / 256;      // accumulators per thread and output at the largest head dim

struct AttGradArgs {
    const float *q, *k, *v, *mask, *o, *dout;
    float *dq, *dk, *dv;
    float *stats;                                   // [3][B * heads * Lq]: m, 1 / l, D
    long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int B, heads, Lq, Lk, d;
    float scale;
};

static size_t ag_stats_lds(int d) { return ((size_t)(AG_OWN + AG_STEP) * (d + 1) + (size_t)AG_OWN * (AG_STEP + 1) + 2 * AG_OWN) * sizeof(float); }
static size_t ag_dq_lds(int d) {
    return ((size_t)(2 * AG_OWN + 2 * AG_STEP) * (d + 1) + (size_t)AG_OWN * (AG_STEP + 1) + 3 * AG_OWN) * sizeof(float);
}
static size_t ag_dkv_lds(int d) {
    return ((size_t)(2 * AG_OWN + 2 * AG_STEP) * (d + 1) + (size_t)2 * AG_OWN * (AG_STEP + 1) + 3 * AG_STEP + AG_OWN) * sizeof(float);
}

// rows [r0, r0 + n) of one head of a [B * L, ld] matrix into an LDS image of `rows` rows of pitch d + 1; rows from n on are zero
__device__ __forceinline__ void ag_stage(float *__restrict__ dst, const float *__restrict__ src, long ld, long row0, int hcol, int rows, int n,
                                         int d, int tid) {
    const int dp = d + 1;
    for (int i = tid; i < rows * d; i += 256) {
        const int r = i / d, c = i - r * d;
        dst[r * dp + c] = r < n ? src[(row0 + r) * ld + hcol + c] : 0.f;
    }
}

__global__ __launch_bounds__(256) void attgrad_stats_kernel(AttGradArgs a, int nqb) {
    extern __shared__ float ag_lds[];
    const int d = a.d, dp = d + 1, lp = AG_STEP + 1;
    float *qs = ag_lds, *ks = qs + AG_OWN * dp, *ps = ks + AG_STEP * dp, *ms = ps + AG_OWN * lp, *ls = ms + AG_OWN;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bh = blockIdx.x / nqb, q0 = (blockIdx.x - bh * nqb) * AG_OWN;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int nq = min(AG_OWN, a.Lq - q0);
    ag_stage(qs, a.q, a.ldq, (long)b * a.Lq + q0, h * d, AG_OWN, nq, d, tid);
    if (tid < AG_OWN) {
        ms[tid] = -INFINITY;
        ls[tid] = 0.f;
    }
    for (int k0 = 0; k0 < a.Lk; k0 += AG_STEP) {
        const int nk = min(AG_STEP, a.Lk - k0);
        ag_stage(ks, a.k, a.ldk, (long)b * a.Lk + k0, h * d, AG_STEP, nk, d, tid);
        __syncthreads();
        for (int i = tid; i < AG_OWN * AG_STEP; i += 256) {
            const int r = i / AG_STEP, jj = i - r * AG_STEP;
            float s = 0.f;
            for (int c = 0; c < d; ++c) s += qs[r * dp + c] * ks[jj * dp + c];
            ps[r * lp + jj] = jj < nk ? s * a.scale + (a.mask ? a.mask[(long)b * a.Lk + k0 + jj] : 0.f) : -INFINITY;
        }
        __syncthreads();
        for (int r = wave; r < AG_OWN; r += 4) {
            const float x = ps[r * lp + lane];
            float mx = x;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            const float mo = ms[r], mn = fmaxf(mo, mx);
            const float alpha = expf(mo - mn);                   // first tile: exp(-inf) = 0
            float sum = expf(x - mn);                            // padded keys: exp(-inf) = 0
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
            const float lo = ls[r];
            if (lane == 0) {
                ms[r] = mn;
                ls[r] = alpha * lo + sum;
            }
        }
        __syncthreads();            // the next tile overwrites K and the scores
    }
    const long n = (long)a.B * a.heads * a.Lq;
    for (int r = wave; r < nq; r += 4) {
        const long grow = (long)b * a.Lq + q0 + r;
        const float *orow = a.o + grow * a.ldo + h * d, *drow = a.dout + grow * a.lddo + h * d;
        float acc = 0.f;
        for (int c = lane; c < d; c += 64) acc += drow[c] * orow[c];
        acc = wave_sum(acc);
        if (lane == 0) {
            const long srow = (long)bh * a.Lq + q0 + r;
            a.stats[srow] = ms[r];
            a.stats[n + srow] = 1.0f / ls[r];
            a.stats[2 * n + srow] = acc;
        }
    }
}

// the statistics of rows [row0, row0 + n) of (batch, head) bh into st[3][rows]; rows from n on: m = 0, 1 / l = 0, D = 0
__device__ __forceinline__ void ag_stage_stats(float *__restrict__ st, const AttGradArgs &a, long bh, int row0, int rows, int n, int tid) {
    const long total = (long)a.B * a.heads * a.Lq;
    for (int i = tid; i < 3 * rows; i += 256) {
        const int w = i / rows, r = i - w * rows;
        st[i] = r < n ? a.stats[w * total + bh * a.Lq + row0 + r] : 0.f;
    }
}

__global__ __launch_bounds__(256) void attgrad_dq_kernel(AttGradArgs a, int nqb) {
    extern __shared__ float ag_lds[];
    const int d = a.d, dp = d + 1, lp = AG_STEP + 1;
    float *qs = ag_lds, *dos = qs + AG_OWN * dp, *ks = dos + AG_OWN * dp, *vs = ks + AG_STEP * dp, *ds = vs + AG_STEP * dp,
          *st = ds + AG_OWN * lp;
    const int tid = threadIdx.x;
    const int bh = blockIdx.x / nqb, q0 = (blockIdx.x - bh * nqb) * AG_OWN;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int nq = min(AG_OWN, a.Lq - q0);
    ag_stage(qs, a.q, a.ldq, (long)b * a.Lq + q0, h * d, AG_OWN, nq, d, tid);
    ag_stage(dos, a.dout, a.lddo, (long)b * a.Lq + q0, h * d, AG_OWN, nq, d, tid);
    ag_stage_stats(st, a, bh, q0, AG_OWN, nq, tid);
    float acc[AG_ACC];
#pragma unroll
    for (int n = 0; n < AG_ACC; ++n) acc[n] = 0.f;

    for (int k0 = 0; k0 < a.Lk; k0 += AG_STEP) {
        const int nk = min(AG_STEP, a.Lk - k0);
        ag_stage(ks, a.k, a.ldk, (long)b * a.Lk + k0, h * d, AG_STEP, nk, d, tid);
        ag_stage(vs, a.v, a.ldv, (long)b * a.Lk + k0, h * d, AG_STEP, nk, d, tid);
        __syncthreads();
        for (int i = tid; i < AG_OWN * AG_STEP; i += 256) {
            const int r = i / AG_STEP, jj = i - r * AG_STEP;
            float s = 0.f, dpv = 0.f;
            for (int c = 0; c < d; ++c) {
                s += qs[r * dp + c] * ks[jj * dp + c];
                dpv += dos[r * dp + c] * vs[jj * dp + c];
            }
            float dsv = 0.f;
            if (jj < nk && r < nq) {
                s = s * a.scale + (a.mask ? a.mask[(long)b * a.Lk + k0 + jj] : 0.f);
                const float p = expf(s - st[r]) * st[AG_OWN + r];
                dsv = p * (dpv - st[2 * AG_OWN + r]);
            }
            ds[r * lp + jj] = dsv;
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < AG_ACC; ++n) {
            const int i = tid + 256 * n;
            if (i < AG_OWN * d) {
                const int r = i / d, c = i - r * d;
                float t = acc[n];
                for (int jj = 0; jj < AG_STEP; ++jj) t += ds[r * lp + jj] * ks[jj * dp + c];
                acc[n] = t;
            }
        }
        __syncthreads();            // the next tile overwrites K, V and dS
    }
#pragma unroll
    for (int n = 0; n < AG_ACC; ++n) {
        const int i = tid + 256 * n;
        if (i < AG_OWN * d) {
            const int r = i / d, c = i - r * d;
            if (r < nq) a.dq[((long)b * a.Lq + q0 + r) * a.lddq + h * d + c] = acc[n] * a.scale;
        }
    }
}

__global__ __launch_bounds__(256) void attgrad_dkv_kernel(AttGradArgs a, int nkb) {
    extern __shared__ float ag_lds[];
    const int d = a.d, dp = d + 1, lp = AG_STEP + 1;
    float *ks = ag_lds, *vs = ks + AG_OWN * dp, *qs = vs + AG_OWN * dp, *dos = qs + AG_STEP * dp, *pt = dos + AG_STEP * dp,
          *dst = pt + AG_OWN * lp, *st = dst + AG_OWN * lp, *mk = st + 3 * AG_STEP;
    const int tid = threadIdx.x;
    const int bh = blockIdx.x / nkb, j0 = (blockIdx.x - bh * nkb) * AG_OWN;
    const int b = bh / a.heads, h = bh - b * a.heads;
    const int nk = min(AG_OWN, a.Lk - j0);
    ag_stage(ks, a.k, a.ldk, (long)b * a.Lk + j0, h * d, AG_OWN, nk, d, tid);
    ag_stage(vs, a.v, a.ldv, (long)b * a.Lk + j0, h * d, AG_OWN, nk, d, tid);
    if (tid < AG_OWN) mk[tid] = a.mask && tid < nk ? a.mask[(long)b * a.Lk + j0 + tid] : 0.f;
    float acck[AG_ACC], accv[AG_ACC];
#pragma unroll
    for (int n = 0; n < AG_ACC; ++n) acck[n] = accv[n] = 0.f;

    for (int q0 = 0; q0 < a.Lq; q0 += AG_STEP) {
        const int nq = min(AG_STEP, a.Lq - q0);
        ag_stage(qs, a.q, a.ldq, (long)b * a.Lq + q0, h * d, AG_STEP, nq, d, tid);
        ag_stage(dos, a.dout, a.lddo, (long)b * a.Lq + q0, h * d, AG_STEP, nq, d, tid);
        ag_stage_stats(st, a, bh, q0, AG_STEP, nq, tid);
        __syncthreads();
        for (int i = tid; i < AG_OWN * AG_STEP; i += 256) {
            const int j = i / AG_STEP, r = i - j * AG_STEP;
            float s = 0.f, dpv = 0.f;
            for (int c = 0; c < d; ++c) {
                s += qs[r * dp + c] * ks[j * dp + c];
                dpv += dos[r * dp + c] * vs[j * dp + c];
            }
            float p = 0.f, dsv = 0.f;
            if (j < nk && r < nq) {
                s = s * a.scale + mk[j];
                p = expf(s - st[r]) * st[AG_STEP + r];
                dsv = p * (dpv - st[2 * AG_STEP + r]);
            }
            pt[j * lp + r] = p;
            dst[j * lp + r] = dsv;
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < AG_ACC; ++n) {
            const int i = tid + 256 * n;
            if (i < AG_OWN * d) {
                const int j = i / d, c = i - j * d;
                float tk = acck[n], tv = accv[n];
                for (int r = 0; r < AG_STEP; ++r) {
                    tv += pt[j * lp + r] * dos[r * dp + c];
                    tk += dst[j * lp + r] * qs[r * dp + c];
                }
                acck[n] = tk;
                accv[n] = tv;
            }
        }
        __syncthreads();            // the next tile overwrites Q, dO, the statistics, P and dS
    }
#pragma unroll
    for (int n = 0; n < AG_ACC; ++n) {
        const int i = tid + 256 * n;
        if (i < AG_OWN * d) {
            const int j = i / d, c = i - j * d;
            if (j < nk) {
                a.dk[((long)b * a.Lk + j0 + j) * a.lddk + h * d + c] = acck[n] * a.scale;
                a.dv[((long)b * a.Lk + j0 + j) * a.lddv + h * d + c] = accv[n];
            }
        }
    }
}

static size_t attgrad_workspace_bytes(int B, int heads, int Lq) {
    if (B < 1 || heads < 1 || Lq < 1) return 0;
    return (size_t)3 * B * heads * Lq * sizeof(float);
}

// everything the launch refuses, without touching a device or reading through a pointer
static int attgrad_check(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const float *o, long ldo,
                         const float *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk, const float *dv, long lddv,
                         int B, int heads, int Lq, int Lk, int d, const void *workspace, size_t workspace_bytes) {
    VK_REQUIRE(q && k && v && o && dout && dq && dk && dv, VK_EINVAL, "attention_grad: null argument");
    VK_REQUIRE(B >= 1 && heads >= 1 && Lq >= 1 && Lk >= 1, VK_EINVAL, "attention_grad: bad geometry (B=%d heads=%d Lq=%d Lk=%d)", B, heads, Lq,
               Lk);
    VK_REQUIRE(d >= 1 && d <= AG_MAXD, VK_EINVAL, "attention_grad: head dim %d is outside 1..%d", d, AG_MAXD);
    const long width = (long)heads * d;
    const long lds[8] = {ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv};
    static const char *const names[8] = {"ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv"};
    for (int i = 0; i < 8; ++i)
        VK_REQUIRE(lds[i] >= width, VK_EINVAL, "attention_grad: %s=%ld is below heads * d = %ld", names[i], lds[i], width);
    VK_REQUIRE((long)B * heads * ceil_div(Lq > Lk ? Lq : Lk, AG_OWN) < (1L << 31), VK_EINVAL, "attention_grad: too many (batch, head, tile) items");
    const size_t need = attgrad_workspace_bytes(B, heads, Lq);
    VK_REQUIRE(workspace && workspace_bytes >= need, VK_EINVAL, "attention_grad: needs a workspace of %zu bytes, got %zu", need, workspace_bytes);
    VK_REQUIRE(((uintptr_t)workspace & 3) == 0, VK_EINVAL, "attention_grad: the workspace must be 4-byte aligned");
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

size_t vk_attention_grad_workspace_bytes(int B, int heads, int Lq) { return attgrad_workspace_bytes(B, heads, Lq); }

int vk_attention_grad_check(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const float *mask, const float *o,
                            long ldo, const float *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk, const float *dv,
                            long lddv, int B, int heads, int Lq, int Lk, int d, const void *workspace, size_t workspace_bytes) {
    (void)mask;                     // may be NULL: no key is masked
    return attgrad_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, workspace,
                         workspace_bytes);
}

int vk_attention_grad(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const float *mask, const float *o,
                      long ldo, const float *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, int B,
                      int heads, int Lq, int Lk, int d, void *workspace, size_t workspace_bytes, void *stream) {
    VK_TRY(attgrad_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, workspace,
                         workspace_bytes));
    const AttGradArgs a = {q, k, v, mask, o, dout, dq, dk, dv, (float *)workspace, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                           B, heads, Lq, Lk, d, 1.0f / sqrtf((float)d)};
    hipStream_t s = (hipStream_t)stream;
    const int nqb = ceil_div(Lq, AG_OWN), nkb = ceil_div(Lk, AG_OWN);
    VK_TRY(launch_lds(attgrad_stats_kernel, dim3(B * heads * nqb), dim3(256), ag_stats_lds(d), ag_stats_lds(AG_MAXD), s, a, nqb));
    VK_TRY(launch_lds(attgrad_dq_kernel, dim3(B * heads * nqb), dim3(256), ag_dq_lds(d), ag_dq_lds(AG_MAXD), s, a, nqb));
    VK_TRY(launch_lds(attgrad_dkv_kernel, dim3(B * heads * nkb), dim3(256), ag_dkv_lds(d), ag_dkv_lds(AG_MAXD), s, a, nkb));
    return VK_OK;
}

}  // extern "C"
