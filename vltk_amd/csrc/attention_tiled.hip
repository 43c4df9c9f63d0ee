// Attention at any sequence length: the online-soft-max forms of lxmert.hip's two attention kernels, the
// pure routing function both entry points switch on, and vk_attention_tiled.
//
//   attention_tiled_kernel   bf16 / f16, head dim 32 / 64, any Lq, Lk: v_mfma_f32_16x16x32, one wave per (batch, head, block of
//                            16 or 32 queries), 64-key tiles, P rounded to the storage type for the second product
//   attention_stream_kernel  f32 / f16 / bf16, head dim <= 256, any alignment: fp32 FMAs over fp32 LDS tiles, P not rounded
//
// Both keep scores, running maximum m, running sum l and O in fp32: per tile m' = max(m, rowmax), a = exp(m - m'),
// p = exp(s - m'), O = a O + p V, l = a l + sum p; the output is O / l (a true division), rounded once.  A padding key of the last
// tile scores -inf; no tile is all padding, so m is finite after the first tile (a masked key scores about finfo.min, which is finite).
#include <cstdlib>

#include "vk_common.h"

namespace vk {

typedef _Float16 tat_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 tat_b8 __attribute__((ext_vector_type(8)));
typedef float tat_f4 __attribute__((ext_vector_type(4)));
template <typename T>
struct TatFrag;
template <>
struct TatFrag<_Float16> {
    typedef tat_h8 type;
    static __device__ __forceinline__ tat_f4 mma(tat_h8 a, tat_h8 b, tat_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <>
struct TatFrag<__bf16> {
    typedef tat_b8 type;
    static __device__ __forceinline__ tat_f4 mma(tat_b8 a, tat_b8 b, tat_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// The tiled kernel's exponential: v_exp_f32 on x * log2(e).  Its error (about 1e-6 relative at a soft-max's arguments) is far
// below the rounding of P to a 16-bit type; exp(0) = 1 and exp(-inf) = 0 exactly, and a result below the normal range is 0.
static __device__ __forceinline__ float tat_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

constexpr int TAT_KT = 64;                      // keys per tile (four 16-key score blocks, two 32-key slices of the second product)
constexpr int TAT_PP = 72;                      // row pitch (elements) of the P and V^T images: 64 keys + 8 (bank skew)

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
    typedef typename TatFrag<T>::type frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = TAT_KT / 16, PER_WAVE = (QB * 16 + D) * TAT_PP;
    extern __shared__ __attribute__((aligned(16))) unsigned char tat_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int item = blockIdx.x * 4 + wave;
    const bool live = item < total;
    const int ic = live ? item : total - 1;
    const int bh = ic / nqb, q0 = (ic - bh * nqb) * (QB * 16);
    const int b = bh / heads, h = bh - b * heads;
    T *pt = reinterpret_cast<T *>(tat_lds) + wave * PER_WAVE, *vt = pt + QB * 16 * TAT_PP;
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
    tat_f4 o[QB][NDB];
    float m[QB][4], l[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[qb][db] = tat_f4{0.f, 0.f, 0.f, 0.f};
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
                    vt32[((c * 8 + e) * TAT_PP) / 2 + kp] = (unsigned)ulo | ((unsigned)uhi << 16);
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
            tat_f4 sc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                tat_f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = TatFrag<T>::mma(qf[qb][ks], kf[kb][ks], a);
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
                    pt[row * TAT_PP + kb * 16 + j] = (T)p;
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
            for (int qb = 0; qb < QB; ++qb) pf[qb] = *reinterpret_cast<const frag *>(pt + (qb * 16 + j) * TAT_PP + k2 * 32 + g * 8);
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const frag vf = *reinterpret_cast<const frag *>(vt + (db * 16 + j) * TAT_PP + k2 * 32 + g * 8);
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) o[qb][db] = TatFrag<T>::mma(pf[qb], vf, o[qb][db]);
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
__device__ __forceinline__ float tat_ldf(const T *p) { return (float)*p; }

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
        qs[r * dp + c] = r < nq ? tat_ldf(q + ((long)b * Lq + q0 + r) * ldq + h * d + c) : 0.f;
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
            ks[r * dp + c] = ok ? tat_ldf(k + ((long)b * Lk + k0 + r) * ldk + h * d + c) : 0.f;
            vs[i] = ok ? tat_ldf(v + ((long)b * Lk + k0 + r) * ldv + h * d + c) : 0.f;
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

static bool env_off(const char *name) {
    const char *e = getenv(name);
    return e && e[0] == '0';
}

// The one routing rule (host only); vk_attention and vk_attention_tiled switch on it.
int attention_route(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16, int tiled_entry) {
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
    if (tiled_entry && !env_off("VK_ATTENTION_TILED")) {
        route = mfma_ok ? VK_ATT_ROUTE_TILED : VK_ATT_ROUTE_STREAM;
    } else {
        const size_t smem = ((size_t)(Lq + Lk) * (d + 1) + (size_t)Lk * d + (size_t)Lq * (Lk + 1)) * sizeof(float);
        if (mfma_ok && Lq <= 48 && Lk <= 64)
            route = VK_ATT_ROUTE_MFMA;
        else if (smem <= 160 * 1024)
            route = VK_ATT_ROUTE_LDS;
        else
            route = mfma_ok ? VK_ATT_ROUTE_TILED : VK_ATT_ROUTE_STREAM;
    }
    if (route == VK_ATT_ROUTE_STREAM && d > STR_MAXD) {
        set_error("attention: head dim %d is beyond the streaming kernel's limit of %d (Lq=%d Lk=%d)", d, STR_MAXD, Lq, Lk);
        return -VK_EINVAL;
    }
    return route;
}

template <typename T, int D>
static int tiled_launch(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo,
                        int B, int heads, int Lq, int Lk, float scale, hipStream_t s) {
#define VK_TAT(QB)                                                                                                              \
    do {                                                                                                                        \
        const int nqb = (Lq + QB * 16 - 1) / (QB * 16), total = B * heads * nqb;                                                \
        const size_t smem = (size_t)4 * (QB * 16 + D) * TAT_PP * sizeof(T);                                                     \
        VK_TRY(set_max_lds(attention_tiled_kernel<T, D, QB>, smem));                                                            \
        hipLaunchKernelGGL((attention_tiled_kernel<T, D, QB>), dim3((total + 3) / 4), dim3(256), smem, s, (const T *)q, ldq,    \
                           (const T *)k, ldk, (const T *)v, ldv, mask, (T *)out, ldo, heads, Lq, Lk, nqb, total, scale);         \
    } while (0)
    if (Lq <= 16) VK_TAT(1); else VK_TAT(2);
#undef VK_TAT
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

template <typename T>
static int stream_launch(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo,
                         int B, int heads, int Lq, int Lk, int d, float scale, hipStream_t s) {
    const int nqb = (Lq + STR_QB - 1) / STR_QB;
    VK_TRY(set_max_lds(attention_stream_kernel<T>, stream_lds_bytes(STR_MAXD)));
    hipLaunchKernelGGL(attention_stream_kernel<T>, dim3(B * heads * nqb), dim3(256), stream_lds_bytes(d), s, (const T *)q, ldq,
                       (const T *)k, ldk, (const T *)v, ldv, mask, (T *)out, ldo, heads, Lq, Lk, d, nqb, scale);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int launch_attention_long(int route, const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask,
                          void *out, int ldo, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)d);
    VK_REQUIRE((long)B * heads * ((Lq + 15) / 16) < (1L << 31), VK_EINVAL, "attention: too many (batch, head, query block) items");
    if (route == VK_ATT_ROUTE_TILED) {
        if (dt == VK_F16)
            return d == 64 ? tiled_launch<_Float16, 64>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, scale, s)
                           : tiled_launch<_Float16, 32>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, scale, s);
        return d == 64 ? tiled_launch<__bf16, 64>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, scale, s)
                       : tiled_launch<__bf16, 32>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, scale, s);
    }
    VK_REQUIRE(route == VK_ATT_ROUTE_STREAM, VK_EINVAL, "attention: route %d is not one of the long-sequence kernels", route);
    switch (dt) {
        case VK_F32: return stream_launch<float>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, d, scale, s);
        case VK_F16: return stream_launch<_Float16>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, d, scale, s);
        case VK_BF16: return stream_launch<__bf16>(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, d, scale, s);
        default: break;
    }
    VK_REQUIRE(false, VK_EINVAL, "attention: dtype must be f32, f16 or bf16");
    return VK_EINVAL;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_attention_route(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16, int tiled_entry) {
    return attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, aligned16, tiled_entry);
}

int vk_attention_tiled(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo,
                       int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream) {
    VK_REQUIRE(q && k && v && out, VK_EINVAL, "attention: null argument");
    VK_REQUIRE(B > 0 && heads > 0, VK_EINVAL, "attention: bad geometry (B=%d heads=%d)", B, heads);
    const int aligned = ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0;
    const int route = attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, aligned, 1);
    if (route < 0) return -route;
    if (route == VK_ATT_ROUTE_MFMA || route == VK_ATT_ROUTE_LDS)       // VK_ATTENTION_TILED=0: exactly vk_attention
        return vk_attention(q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, d, dt, stream);
    return launch_attention_long(route, q, ldq, k, ldk, v, ldv, mask, out, ldo, B, heads, Lq, Lk, d, dt, (hipStream_t)stream);
}

}  // extern "C"
