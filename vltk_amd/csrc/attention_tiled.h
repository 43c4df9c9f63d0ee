// attention_tiled_kernel, the online-soft-max attention on the matrix cores, with what its two translation units share: the
// argument struct of the entry points and the launchers.  attention.hip instantiates the plain forms, attention_dropout.hip the DROP
// forms: a kernel is instantiated in one unit only.  The fragment types, the constants, the exponential and pack16 are the shared
// ones of mfma16.h and attention_mma.h.  The kernel's body stays written out and compiles to the instructions it always had.  Keep in
// step with attention_mma.h: the row loads with att_row_frags, the V^T image with att_image_t, and the m / l update with
// att_online_row (the backward's pass 1 must reproduce this kernel's m and l bit for bit; the tests of the backward hold that).
#pragma once
#include "attention_mma.h"
#include "philox.h"

namespace vk {

// One WAVE per (batch, head, block of QB * 16 queries), four per workgroup; the lane layouts are attention_mfma_kernel's:
//   * Q fragments of the block stay in registers; a tile's K rows are the B fragments as they lie in memory;
//   * a score tile leaves a lane with S[q = 4g + e][key = j]: row maximum and row sum reduce over the four key blocks in
//     registers and over the 16 lanes of a group with four shuffles;
//   * O's accumulator rows are the same 4g + e, so the rescale factor of a row is already in the lanes that hold it;
//   * P (rounded to T) and V^T go through a per-wave LDS image; a lane transposes two keys at a time (32-bit LDS writes,
//     consecutive lanes on consecutive words).  Padded keys carry P = 0 and V = 0.
// Every wave of a workgroup runs the same number of tiles (idle waves redo the last item and store nothing), so the
// barriers are uniform.
//
// DROP (vk_attention_tiled_dropout; the one trailing argument is a DropArgs): transformers' dropout(softmax(s)) under the mask of
// philox.h.  m and l run over the undropped exp(s - m); a dropped element is zeroed before it is rounded to T for the P image; the
// survivors' scale is applied once, in O * rs / l.  A 16 x 64 score tile is 4 x 16 blocks of the mask: lane 16 g + jj makes ONE
// Philox call, for block (row block g, key block jj) of the tile, and folds it into 16 keep bits (philox_keep16, bit 8 (k & 3) +
// (q & 3)); the lane that holds S[4 g + e][16 kb + j] reads the bits of block (g, 4 kb + (j >> 2)) from lane 16 g + 4 kb + (j >> 2)
// of its own group: four ds_bpermute_b32 per lane and tile, no byte leaves a register otherwise.  The DROP forms are instantiated
// in attention_dropout.hip.  LDS is unchanged; VGPRs as the compiler reports them, plain -> DROP: d = 64: 153 -> 173 at QB = 2 (three
// -> two waves per SIMD), 120 -> 128 at QB = 1; d = 32: 107 -> 129 at QB = 2 (four -> three waves) and 88 -> 93.  DROP = false has no trailing
// argument and is the kernel as it was.
template <typename T, int D, int QB, bool DROP, typename... DA>
__global__ __launch_bounds__(256) void attention_tiled_kernel(const T *__restrict__ q, int ldq, const T *__restrict__ k, int ldk,
                                                             const T *__restrict__ v, int ldv, const float *__restrict__ mask,
                                                             T *__restrict__ out, int ldo, int heads, int Lq, int Lk, int nqb, int total,
                                                             float scale, DA... drop) {
    static_assert(sizeof...(DA) == (DROP ? 1 : 0), "a DropArgs behind the arguments of the DROP form, nothing otherwise");
    const DropArgs da = drop_args_of(drop...);
    typedef typename Mma16<T>::frag frag;
    constexpr int KD = D / 32, NDB = D / 16, KB = ATT_KT / 16, PER_WAVE = (QB * 16 + D) * ATT_PP;
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

    for (int k0 = 0; k0 < Lk; k0 += ATT_KT) {
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
                for (int e = 0; e < 8; ++e) vt32[((c * 8 + e) * ATT_PP) / 2 + kp] = pack16<T>(t0[e], t1[e]);
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
            m16_f4 sc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                m16_f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) a = Mma16<T>::mma(qf[qb][ks], kf[kb][ks], a);
                const bool ok = k0 + kb * 16 + j < Lk;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = ok ? a[e] * scale + mk[kb] : -INFINITY;
                sc[kb] = a;
            }
            uint32_t keep[KB] = {};
            if constexpr (DROP) {
                drop_tile_bits(keep, da, (uint64_t)bh * ((Lq + 3) >> 2), (uint64_t)((Lk + 3) >> 2), (q0 + qb * 16) >> 2, k0 >> 2, true, g, j);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) keep[kb] >>= 8 * (j & 3);        // bit e: row 4 g + e of this lane's key
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
                    if constexpr (DROP) pt[row * ATT_PP + kb * 16 + j] = (T)((keep[kb] >> e) & 1u ? p : 0.f);
                    else pt[row * ATT_PP + kb * 16 + j] = (T)p;
                }
#pragma unroll
                for (int s = 8; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
                m[qb][e] = mn;
                l[qb][e] = alpha * l[qb][e] + sum;               // contracts to att_online_row's fmaf
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
                for (int qb = 0; qb < QB; ++qb) o[qb][db] = Mma16<T>::mma(pf[qb], vf, o[qb][db]);
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
            for (int db = 0; db < NDB; ++db) {
                if constexpr (DROP) out[((long)b * Lq + row) * ldo + h * D + db * 16 + j] = (T)(o[qb][db][e] * da.rs / l[qb][e]);
                else out[((long)b * Lq + row) * ldo + h * D + db * 16 + j] = (T)(o[qb][db][e] / l[qb][e]);
            }
        }
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

// the DROP form (a DropArgs behind the stream) has the same grid, LDS and choice of QB
template <typename T, int D, int QB, typename... DA>
static int tiled_launch_qb(const AttArgs &a, float scale, hipStream_t s, DA... da) {
    const int nqb = (a.Lq + QB * 16 - 1) / (QB * 16), total = a.B * a.heads * nqb;
    const size_t smem = (size_t)4 * (QB * 16 + D) * ATT_PP * sizeof(T);
    return launch_lds(attention_tiled_kernel<T, D, QB, sizeof...(DA) != 0, DA...>, dim3((total + 3) / 4), dim3(256), smem, smem, s, VK_ATT_IO(T),
                      nqb, total, scale, da...);
}
template <typename T, int D, typename... DA>
static int tiled_launch(const AttArgs &a, float scale, hipStream_t s, DA... da) {
    return a.Lq <= 16 ? tiled_launch_qb<T, D, 1>(a, scale, s, da...) : tiled_launch_qb<T, D, 2>(a, scale, s, da...);
}

}  // namespace vk
