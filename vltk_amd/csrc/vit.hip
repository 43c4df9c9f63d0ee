// The embedding stage of the Vision Transformer (transformers/models/vit/modeling_vit.py v5.15, ViTPatchEmbeddings.forward :62-69
// and ViTEmbeddings.forward :129-161), the one piece of that model the BERT ops do not already cover.  The patch projection is a
// Conv2d(C, H, P, stride = P): every output pixel reads its own P x P patch and no other, so it is a plain GEMM over patch rows.
// Two small kernels stand around the existing vk_linear:
//
//   vk_vit_patchify   pixel_values [B, C, Hi, Wi] fp32 NCHW -> rows [B * gh * gw, ldk] in the storage type; row b*gh*gw + i*gw + j
//                     holds patch (i, j) in the order (c, py, px), the flattening of the conv weight's .view(H, -1); the columns
//                     C*P*P .. ldk - 1 (the GEMM's K-tile padding, which it reads) are written as zero
//   vk_vit_assemble   x [B * (N + 1), H]: row b*(N+1) = cls + pos[0], row b*(N+1) + 1 + n = proj[b*N + n] + pos[1 + n];
//                     the sum in fp32, one rounding on the way out; proj's padding columns are never read
//
// Both are one thread per 16-byte output chunk (a chunk never straddles two rows: ldk * es and, on the chunk form, H * es are
// multiples of 16), adjacent threads on adjacent chunks.  No LDS, no atomics, every index in 64 bits.
#include "row_norm.h"      // ld_chunk, st_chunk

namespace vk {

struct PatchifyArgs {
    const float *pix;
    void *rows;
    int B, C, Hi, Wi, P, gh, gw, ldk;
    long n_rows;
};

// T: storage type; VEC: every chunk lies inside one patch row of the image and starts 16-byte aligned there (P a multiple of the
// chunk, Wi a multiple of 4, an aligned base), so it is read with float4 loads.  Otherwise each element finds its own pixel:
// P = 14 puts a patch row at an odd multiple of 8 bytes and lets a chunk run over the end of one.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const PatchifyArgs a) {
    constexpr int VW = 16 / sizeof(T);
    typedef T vecT __attribute__((ext_vector_type(VW)));
    const int cpr = a.ldk / VW;                              // chunks per output row
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_rows * cpr) return;
    const long row = t / cpr;
    const int k0 = (int)(t - row * cpr) * VW;
    const int PP = a.P * a.P, K = a.C * PP;
    const int j = (int)(row % a.gw), i = (int)((row / a.gw) % a.gh);
    const long b = row / ((long)a.gw * a.gh);
    const long plane = (long)a.Hi * a.Wi;
    const float *img = a.pix + b * a.C * plane + (long)i * a.P * a.Wi + (long)j * a.P;   // (b, 0, i*P, j*P)
    vecT o;
    if constexpr (VEC) {
        if (k0 < K) {                                        // K % VW == 0 here: the chunk is all pixels or all padding
            const int c = k0 / PP, r = k0 - c * PP, py = r / a.P, px = r - py * a.P;
            const float4 *src = reinterpret_cast<const float4 *>(img + c * plane + (long)py * a.Wi + px);
#pragma unroll
            for (int q = 0; q < VW / 4; ++q) {
                const float4 v = src[q];
                o[4 * q] = (T)v.x, o[4 * q + 1] = (T)v.y, o[4 * q + 2] = (T)v.z, o[4 * q + 3] = (T)v.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) o[e] = (T)0.f;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            const int k = k0 + e;
            float v = 0.f;
            if (k < K) {
                const int c = k / PP, r = k - c * PP, py = r / a.P, px = r - py * a.P;
                v = img[c * plane + (long)py * a.Wi + px];
            }
            o[e] = (T)v;
        }
    }
    *reinterpret_cast<vecT *>((T *)a.rows + row * a.ldk + k0) = o;
}

template <typename T>
static int patchify_launch(const PatchifyArgs &a, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const long chunks = a.n_rows * (a.ldk / VW), blocks = (chunks + 255) / 256;
    VK_REQUIRE(blocks < (1L << 31), VK_EINVAL, "vit_patchify: %ld chunks of output exceed one launch", chunks);
    const bool vec = a.P % VW == 0 && a.Wi % 4 == 0 && (uintptr_t)a.pix % 16 == 0;
    if (vec)
        hipLaunchKernelGGL((vit_patchify_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((vit_patchify_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

struct AssembleArgs {
    const void *proj, *cls, *pos;
    void *x;
    int B, N, H, ldp;
    long n_rows;
};

// VW: elements per chunk (16 / sizeof(T) on the chunk form, 1 on the scalar one); H % VW == 0.
template <typename T, int VW>
__global__ __launch_bounds__(256) void vit_assemble_kernel(const AssembleArgs a) {
    const int cpr = a.H / VW;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_rows * cpr) return;
    const long row = t / cpr;
    const int col = (int)(t - row * cpr) * VW;
    const long b = row / (a.N + 1);
    const int r = (int)(row - b * (a.N + 1));
    const T *src = r == 0 ? (const T *)a.cls : (const T *)a.proj + (b * a.N + (r - 1)) * a.ldp;
    const T *pos = (const T *)a.pos + (long)r * a.H;
    float u[VW], p[VW];
    ld_chunk<T, VW>(src + col, u);
    ld_chunk<T, VW>(pos + col, p);
#pragma unroll
    for (int e = 0; e < VW; ++e) u[e] += p[e];
    st_chunk<T, VW>((T *)a.x + row * a.H + col, u);
}

template <typename T>
static int assemble_launch(const AssembleArgs &a, hipStream_t s) {
    constexpr int VW = 16 / sizeof(T);
    const uintptr_t bases = (uintptr_t)a.proj | (uintptr_t)a.cls | (uintptr_t)a.pos | (uintptr_t)a.x;
    const bool vec = a.H % VW == 0 && a.ldp % VW == 0 && bases % 16 == 0;
    const long chunks = a.n_rows * (vec ? a.H / VW : a.H), blocks = (chunks + 255) / 256;
    VK_REQUIRE(blocks < (1L << 31), VK_EINVAL, "vit_assemble: %ld chunks of output exceed one launch", chunks);
    if (vec)
        hipLaunchKernelGGL((vit_assemble_kernel<T, VW>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((vit_assemble_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_vit_patchify(const float *pixel_values, int B, int C, int Hi, int Wi, int P, void *rows, int ldk, vk_dtype dt, void *stream) {
    VK_REQUIRE(pixel_values && rows, VK_EINVAL, "vit_patchify: null argument");
    VK_REQUIRE(B >= 1 && P >= 1 && C >= 1 && C <= 4, VK_EINVAL, "vit_patchify: bad geometry (B=%d C=%d P=%d; C in 1..4)", B, C, P);
    VK_REQUIRE(Hi >= P && Wi >= P && Hi % P == 0 && Wi % P == 0, VK_EINVAL,
               "vit_patchify: a %d x %d image is no positive multiple of the %d x %d patch", Hi, Wi, P, P);
    const long K = (long)C * P * P;
    VK_REQUIRE(ldk >= K, VK_EINVAL, "vit_patchify: row stride %d below the patch length %ld", ldk, K);
    VK_REQUIRE(((long)ldk * (long)dtype_size(dt)) % 16 == 0 && (uintptr_t)rows % 16 == 0, VK_EINVAL,
               "vit_patchify: output rows must be whole 16-byte chunks (ldk=%d) from a 16-byte aligned base", ldk);
    PatchifyArgs a;
    a.pix = pixel_values, a.rows = rows;
    a.B = B, a.C = C, a.Hi = Hi, a.Wi = Wi, a.P = P, a.gh = Hi / P, a.gw = Wi / P, a.ldk = ldk;
    a.n_rows = (long)B * a.gh * a.gw;
    VK_REQUIRE(a.n_rows < (1L << 31), VK_EINVAL, "vit_patchify: %ld patch rows", a.n_rows);
    VK_DT_SWITCH(dt, "vit_patchify", return patchify_launch<T>(a, (hipStream_t)stream));
}

int vk_vit_assemble(const void *proj, int ldp, const void *cls_token, const void *position, int B, int N, void *x, int H,
                    vk_dtype dt, void *stream) {
    VK_REQUIRE(proj && cls_token && position && x, VK_EINVAL, "vit_assemble: null argument");
    VK_REQUIRE(B > 0 && N > 0 && (long)B * ((long)N + 1) < (1L << 31), VK_EINVAL, "vit_assemble: bad geometry (B=%d N=%d)", B, N);
    VK_REQUIRE(H > 0, VK_EINVAL, "vit_assemble: H=%d", H);
    VK_REQUIRE(ldp >= H, VK_EINVAL, "vit_assemble: projection row stride %d below the row length %d", ldp, H);
    AssembleArgs a;
    a.proj = proj, a.cls = cls_token, a.pos = position, a.x = x;
    a.B = B, a.N = N, a.H = H, a.ldp = ldp;
    a.n_rows = (long)B * (N + 1);
    VK_DT_SWITCH(dt, "vit_assemble", return assemble_launch<T>(a, (hipStream_t)stream));
}

}  // extern "C"
