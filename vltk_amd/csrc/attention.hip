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
//
// attention_kernel and attention_mfma_kernel are written here; attention_tiled_kernel is attention_tiled.h's and
// attention_stream_kernel attention_stream.h's (each shared with one more unit), and the matrix-core kernels' common device pieces
// are attention_mma.h's.
#include <cstdlib>

#include "attention_stream.h"
#include "attention_tiled.h"

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
constexpr int ATT_MAXQB = 3, ATT_MAXKB = 4;     // 48 queries, 64 keys

template <typename T, int D>
__global__ __launch_bounds__(256) void attention_mfma_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                            const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                            T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int total,
                                                            float scale) {
    typedef typename Mma16<T>::frag frag;
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

    // ---- operand fragments straight from memory (a block past QB or KB lies past the sequence: zeros) ----
    frag qf[ATT_MAXQB][KD], kf[ATT_MAXKB][KD];
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb) att_row_frags<T, KD>(qf[qb], q + (long)b * Lq * ldq + h * D, ldq, qb * 16 + j, Lq, g);
#pragma unroll
    for (int kb = 0; kb < ATT_MAXKB; ++kb) att_row_frags<T, KD>(kf[kb], k + (long)b * Lk * ldk + h * D, ldk, kb * 16 + j, Lk, g);
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
    m16_f4 sc[ATT_MAXQB][ATT_MAXKB];
#pragma unroll
    for (int qb = 0; qb < ATT_MAXQB; ++qb)
#pragma unroll
        for (int kb = 0; kb < ATT_MAXKB; ++kb) {
            m16_f4 a = {0.f, 0.f, 0.f, 0.f};
            if (qb < QB && kb < KB) {
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = Mma16<T>::mma(qf[qb][ks], kf[kb][ks], a);
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
            m16_f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                if (k2 >= KS2) continue;
                const frag vf = *reinterpret_cast<const frag *>(vt + (db * 16 + j) * ATT_PP + k2 * 32 + g * 8);
                o = Mma16<T>::mma(pf[k2], vf, o);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = qb * 16 + g * 4 + e;
                if (live && row < Lq) out[((long)b * Lq + row) * ldo + h * D + db * 16 + j] = (T)o[e];
            }
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

template <typename T>
static int stream_launch(const AttArgs &a, float scale, hipStream_t s) {
    const int nqb = (a.Lq + STR_QB - 1) / STR_QB;
    return launch_lds(attention_stream_kernel<T, false>, dim3(a.B * a.heads * nqb), dim3(256), stream_lds_bytes(a.d), stream_lds_bytes(STR_MAXD), s,
                      VK_ATT_IO(T), a.d, nqb, scale);
}

// The one launcher: `route` is attention_route's answer for these arguments, so the dtype and the head dim are the kernel's.
static int launch_attention(int route, const AttArgs &a, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)a.d);
    VK_REQUIRE((long)a.B * a.heads * ((a.Lq + 15) / 16) < (1L << 31), VK_EINVAL, "attention: too many (batch, head, query block) items");
    int st = VK_EINVAL;
    switch (route) {
        case VK_ATT_ROUTE_MFMA: VK_DT16_D_SWITCH(a.dt, a.d, st = mfma_launch<T, D>(a, scale, s)); break;
        case VK_ATT_ROUTE_TILED: VK_DT16_D_SWITCH(a.dt, a.d, st = tiled_launch<T, D>(a, scale, s)); break;
        case VK_ATT_ROUTE_LDS: VK_DT_SWITCH(a.dt, "attention", st = lds_launch<T>(a, scale, s)); break;
        case VK_ATT_ROUTE_STREAM: VK_DT_SWITCH(a.dt, "attention", st = stream_launch<T>(a, scale, s)); break;
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
