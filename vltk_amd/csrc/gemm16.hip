// The 16-bit half of mixed-precision fine-tuning: a round-to-nearest cast of fp32 to bf16 / fp16 and a GEMM
// on 16-bit operands with fp32 accumulation, in vk_gemm_f32's three transposition forms.  No atomics and no split-K: every output
// has one writer and a fixed summation order, so the same input gives the same bits on every run.  Nothing is written outside
// the n (M x N) elements an entry names.
//
//   cast16_kernel<T>       y = (T)x: the conversion instruction (nearest even; Inf stays Inf, NaN stays NaN, a value below the
//                          target's normal range becomes a subnormal of it).  Eight elements per lane (two 16-byte loads, one
//                          16-byte store) where both pointers are 16-byte aligned, single elements for the tail and otherwise.
//   gemm16_kernel<T, F>    C = op(A) . op(B) (+ bias) on v_mfma_f32_16x16x32.  256 threads = 2 x 2 waves, a wave owns F x F blocks
//                          of 16 x 16, so the tile is 32F x 32F: F = 4 (128 x 128) where such tiles fill half the CUs, F = 2
//                          (64 x 64) elsewhere: vk_gemm_f32's rule.  K goes through LDS in steps of 64.  Both operand images
//                          lie [row][k] with k contiguous, which is what the instruction reads (lane 16 g + j takes row / column j
//                          at k = 8 g .. 8 g + 7 of a 32-k slice: one ds_read_b128).  An operand whose memory runs along k (A as
//                          [M, K]; B as [N, K]) is copied in 16-byte chunks.  One whose memory runs along the row index (A as
//                          [K, M]; B as [K, N]: the TN form, and B of the NN form) is TRANSPOSED on its way in: a thread loads the
//                          same 8 rows at k and k + 1 (two 16-byte loads) and writes 8 words, each a (k, k + 1) pair of one row.
//                          The next step's global loads are issued before the MFMAs of the current one and land in LDS after
//                          them.  Edges: a chunk that crosses the matrix edge is loaded element by element and zero-filled, so
//                          nothing outside M x K / K x N is read, padding included; outside rows / columns are not stored.
//
// LDS: a row is 64 k = 128 bytes on a pitch of 144 bytes (36 words), and its eight 16-byte chunks are rotated by 2 ((row / 8) % 4)
// chunk positions.  Bytes per workgroup: 2 x 32F x 144 = 36864 (F = 4), 18432 (F = 2); the kernel runs two workgroups per CU.
//   fragment read   ds_read_b128, lanes j = 0..15 on rows 36 j words apart, rows 8..15 rotated by 8 words more: first banks (of
//                   64) 0, 36, 8, 44, 16, 52, 24, 60 | 40, 12, 48, 20, 56, 28, 0, 36: rows 14 and 15 share a 4-bank slot with
//                   rows 0 and 1 (2-way where they fall into one service group), the other twelve are alone.  Not measured.
//   chunk write     ds_write_b128, 8 consecutive lanes fill one row's 128 bytes, the next 8 the next row.
//   transposed write  ds_write_b32 of a half-wave = 4 row groups (rows 8 apart) x 8 consecutive k pairs: the row pitch is
//                   4 banks (of 32) per row and 0 per 8 rows, so without the rotation the 4 row groups would share banks;
//                   with it the 32 lanes cover the 8 chunk positions x 4 words = 32 different banks.
//
// Rounding points (u = 2^-24; the 16-bit operands are exact inputs):
//   acc = bias (or 0); per 32-k slice one instruction adds the slice's 32 exact products to acc in fp32; slices ascending in k.
//   Integer data whose sums stay below 2^24 is exact in any order.  C is acc (fp32 out) or acc rounded once to T.
#include "mfma16.h"

namespace vk {

constexpr int G16_BK = 64, G16_PP = 72;         // k per step; row pitch of an operand image, elements

struct Gemm16Args {
    const void *A, *B;
    const float *bias;
    void *C;
    int M, N, K;
    long lda, ldb, ldc;
    int transA, transB, out16;
};

template <typename T>
__global__ __launch_bounds__(256) void cast16_kernel(const float *__restrict__ x, T *__restrict__ y, long n, int vec) {
    typedef typename Mma16<T>::frag frag;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const long n8 = vec ? n / 8 : 0;
    for (long i = gid; i < n8; i += stride) {
        const float4 a = reinterpret_cast<const float4 *>(x)[2 * i], b = reinterpret_cast<const float4 *>(x)[2 * i + 1];
        frag o;
        o[0] = (T)a.x, o[1] = (T)a.y, o[2] = (T)a.z, o[3] = (T)a.w;
        o[4] = (T)b.x, o[5] = (T)b.y, o[6] = (T)b.z, o[7] = (T)b.w;
        reinterpret_cast<frag *>(y)[i] = o;
    }
    for (long i = n8 * 8 + gid; i < n; i += stride) y[i] = (T)x[i];
}

// One operand's 32F x 64 piece of a K step: global -> registers (fetch) -> the LDS image [row][G16_PP] (stash).
// `kcontig`: chunk c = tid + 256 it is (row c / 8, k 8 (c % 8) ..); else pair item c = tid + 256 it is (rows 8 mc .., k 2 kp and
// 2 kp + 1) with mc = 4 (c / 128) + c % 4 and kp = (c / 4) % 32, so that 4 consecutive lanes load 64 consecutive bytes.
template <typename T, int TILE>
struct G16Tile {
    typedef typename Mma16<T>::frag frag;
    static constexpr int PER = TILE / 32;
    frag r[PER];

    static __device__ __forceinline__ int chunk_pos(int kc, int row) { return (kc + 2 * ((row >> 3) & 3)) & 7; }

    __device__ __forceinline__ void fetch(const T *src, long ld, bool kcontig, int r0, int R, int k0, int K, int tid) {
        if (kcontig) {
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int c = tid + 256 * it, row = r0 + (c >> 3), k = k0 + (c & 7) * 8;
                r[it] = load8<T>(src + (long)row * ld + k, row < R ? K - k : 0);
            }
        } else {
#pragma unroll
            for (int it = 0; it < PER / 2; ++it) {
                const int c = tid + 256 * it, mc = 4 * (c >> 7) + (c & 3), kp = (c >> 2) & 31;
                const int m = r0 + mc * 8;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = k0 + 2 * kp + h;
                    r[2 * it + h] = load8<T>(src + (long)k * ld + m, k < K ? R - m : 0);
                }
            }
        }
    }
    __device__ __forceinline__ void stash(T *__restrict__ s, bool kcontig, int tid) const {
        if (kcontig) {
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int c = tid + 256 * it, row = c >> 3;
                *reinterpret_cast<frag *>(s + row * G16_PP + chunk_pos(c & 7, row) * 8) = r[it];
            }
        } else {
            unsigned *s32 = reinterpret_cast<unsigned *>(s);
#pragma unroll
            for (int it = 0; it < PER / 2; ++it) {
                const int c = tid + 256 * it, mc = 4 * (c >> 7) + (c & 3), kp = (c >> 2) & 31;
                const int word = chunk_pos(kp >> 2, mc * 8) * 4 + (kp & 3);
#pragma unroll
                for (int e = 0; e < 8; ++e) s32[(mc * 8 + e) * (G16_PP / 2) + word] = pack16<T>(r[2 * it][e], r[2 * it + 1][e]);
            }
        }
    }
};

template <typename T, int F>
__global__ __launch_bounds__(256, 2) void gemm16_kernel(Gemm16Args a) {
    typedef typename Mma16<T>::frag frag;
    constexpr int TILE = 32 * F;
    extern __shared__ __attribute__((aligned(16))) unsigned char g16_lds[];
    T *sa = reinterpret_cast<T *>(g16_lds), *sb = sa + TILE * G16_PP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int m0 = blockIdx.y * TILE, n0 = blockIdx.x * TILE;
    const int wm = (wave >> 1) * 16 * F, wn = (wave & 1) * 16 * F;
    const bool ka = a.transA == 0, kb = a.transB != 0;
    const T *A = static_cast<const T *>(a.A), *B = static_cast<const T *>(a.B);

    // D of the instruction: register e of lane 16 g + j is row 4 g + e, column j
    m16_f4 acc[F][F];
#pragma unroll
    for (int n = 0; n < F; ++n) {
        const int gc = n0 + wn + 16 * n + j;
        const float bv = a.bias && gc < a.N ? a.bias[gc] : 0.0f;
#pragma unroll
        for (int i = 0; i < F; ++i) acc[i][n] = m16_f4{bv, bv, bv, bv};
    }

    G16Tile<T, TILE> ta, tb;
    ta.fetch(A, a.lda, ka, m0, a.M, 0, a.K, tid);
    tb.fetch(B, a.ldb, kb, n0, a.N, 0, a.K, tid);
    for (int k0 = 0; k0 < a.K; k0 += G16_BK) {
        ta.stash(sa, ka, tid);
        tb.stash(sb, kb, tid);
        __syncthreads();
        if (k0 + G16_BK < a.K) {
            ta.fetch(A, a.lda, ka, m0, a.M, k0 + G16_BK, a.K, tid);
            tb.fetch(B, a.ldb, kb, n0, a.N, k0 + G16_BK, a.K, tid);
        }
#pragma unroll
        for (int ks = 0; ks < G16_BK / 32; ++ks) {
            frag fa[F], fb[F];
#pragma unroll
            for (int i = 0; i < F; ++i) {
                const int row = wm + 16 * i + j;
                fa[i] = *reinterpret_cast<const frag *>(sa + row * G16_PP + G16Tile<T, TILE>::chunk_pos(ks * 4 + g, row) * 8);
            }
#pragma unroll
            for (int n = 0; n < F; ++n) {
                const int row = wn + 16 * n + j;
                fb[n] = *reinterpret_cast<const frag *>(sb + row * G16_PP + G16Tile<T, TILE>::chunk_pos(ks * 4 + g, row) * 8);
            }
#pragma unroll
            for (int i = 0; i < F; ++i)
#pragma unroll
                for (int n = 0; n < F; ++n) acc[i][n] = Mma16<T>::mma(fa[i], fb[n], acc[i][n]);
        }
        __syncthreads();            // the next step overwrites the images
    }

#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
        for (int n = 0; n < F; ++n) {
            const int gc = n0 + wn + 16 * n + j;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int gr = m0 + wm + 16 * i + 4 * g + e;
                if (gr < a.M && gc < a.N) {
                    if (a.out16)
                        static_cast<T *>(a.C)[(long)gr * a.ldc + gc] = (T)acc[i][n][e];
                    else
                        static_cast<float *>(a.C)[(long)gr * a.ldc + gc] = acc[i][n][e];
                }
            }
        }
}

static bool is16(vk_dtype dt) { return dt == VK_F16 || dt == VK_BF16; }

static int gemm16_check(const void *A, long lda, int transA, const void *B, long ldb, int transB, const void *C, long ldc, int M, int N,
                        int K, vk_dtype dt, vk_dtype out_dt) {
    VK_REQUIRE(A && B && C, VK_EINVAL, "gemm_16: null argument");
    VK_REQUIRE(is16(dt), VK_EINVAL, "gemm_16: dt must be f16 or bf16 (fp32 operands are vk_gemm_f32's)");
    VK_REQUIRE(out_dt == VK_F32 || out_dt == dt, VK_EINVAL, "gemm_16: out_dt must be f32 or dt");
    VK_TRY(gemm_shape_check("gemm_16", M, N, K, lda, ldb, ldc, transA, transB));
    VK_REQUIRE(lda % 8 == 0 && ldb % 8 == 0, VK_EINVAL, "gemm_16: lda=%ld and ldb=%ld must be multiples of 8 elements (16-byte rows)", lda, ldb);
    VK_REQUIRE(out_dt == VK_F32 || ldc % 8 == 0, VK_EINVAL, "gemm_16: ldc=%ld of a 16-bit C must be a multiple of 8 elements", ldc);
    VK_REQUIRE((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0, VK_EINVAL, "gemm_16: A, B and C must be 16-byte aligned");
    VK_REQUIRE(ceil_div(M, 64) <= 65535, VK_EINVAL, "gemm_16: M=%d is beyond the grid", M);
    return VK_OK;
}

template <typename T>
static int gemm16_launch(const Gemm16Args &g, int n_cu, hipStream_t s) {
    if (large_tile(g.M, g.N, n_cu)) {
        const size_t smem = (size_t)2 * 128 * G16_PP * sizeof(T);
        return launch_lds(gemm16_kernel<T, 4>, dim3(ceil_div(g.N, 128), ceil_div(g.M, 128)), dim3(256), smem, smem, s, g);
    }
    const size_t smem = (size_t)2 * 64 * G16_PP * sizeof(T);
    return launch_lds(gemm16_kernel<T, 2>, dim3(ceil_div(g.N, 64), ceil_div(g.M, 64)), dim3(256), smem, smem, s, g);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_cast_16(const float *x, void *y, long n, vk_dtype dt, void *stream) {
    VK_REQUIRE(x && y, VK_EINVAL, "cast_16: null argument");
    VK_REQUIRE(n >= 1, VK_EINVAL, "cast_16: n=%ld must be positive", n);
    VK_REQUIRE(is16(dt), VK_EINVAL, "cast_16: dt must be f16 or bf16");
    const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const long groups = (n + 7) / 8;
    const int blocks = (int)((groups + 255) / 256 < 8192 ? (groups + 255) / 256 : 8192);
    if (dt == VK_BF16)
        hipLaunchKernelGGL(cast16_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, static_cast<__bf16 *>(y), n, vec);
    else
        hipLaunchKernelGGL(cast16_kernel<_Float16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, static_cast<_Float16 *>(y), n, vec);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_gemm_16_check(const void *A, long lda, int transA, const void *B, long ldb, int transB, const void *C, long ldc, int M, int N, int K,
                     vk_dtype dt, vk_dtype out_dt) {
    return gemm16_check(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, dt, out_dt);
}

int vk_gemm_16(const void *A, long lda, int transA, const void *B, long ldb, int transB, const float *bias, void *C, long ldc, int M, int N,
               int K, vk_dtype dt, vk_dtype out_dt, void *stream) {
    VK_TRY(gemm16_check(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, dt, out_dt));
    DeviceState *ds;
    VK_TRY(device_state(&ds));
    const Gemm16Args g = {A, B, bias, C, M, N, K, lda, ldb, ldc, transA, transB, out_dt != VK_F32};
    return dt == VK_BF16 ? gemm16_launch<__bf16>(g, ds->n_cu, (hipStream_t)stream) : gemm16_launch<_Float16>(g, ds->n_cu, (hipStream_t)stream);
}

}  // extern "C"
