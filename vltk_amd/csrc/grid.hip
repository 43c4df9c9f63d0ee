// Grid features on gfx950: the Res5 map of a whole image, average-pooled to a fixed Gh x Gw grid of cells, and each
// cell's box (vk_grid_pool; the pooling stage of vk_forward_grid_begin, model.hip).
//
// The rule is this project's, not the reference's: the bins are adaptive_avg_pool2d's over the
// content part of the map, the sum of a cell is taken in fp64 in y-outer, x-inner order and divided once, so a host
// restatement gives the same bits.  No atomics, no cross-lane reduction: a lane owns its channels for the whole cell.
//
// fp64 sums and one IEEE division; built with -ffp-contract=off like the other files whose results are restated bit for bit.
#include <hip/hip_fp16.h>

#include "vk_common.h"
#include "conv_prims.h"

namespace vk {

struct GridCell {
    int ys, ye, xs, xe;
};

// Cell (i, j) of image n: map rows [ys, ye) and columns [xs, xe) of the content extent fh x fw (in map pixels).
__device__ __forceinline__ GridCell grid_cell(int h, int w, int Hm, int Wm, int S, int Gh, int Gw, int i, int j) {
    const long fh_l = ((long)h + S - 1) / S, fw_l = ((long)w + S - 1) / S;
    const int fh = (int)(fh_l < 1 ? 1 : (fh_l > Hm ? Hm : fh_l));
    const int fw = (int)(fw_l < 1 ? 1 : (fw_l > Wm ? Wm : fw_l));
    GridCell c;
    c.ys = (int)(((long)i * fh) / Gh);
    c.ye = (int)((((long)i + 1) * fh + Gh - 1) / Gh);
    c.xs = (int)(((long)j * fw) / Gw);
    c.xe = (int)((((long)j + 1) * fw + Gw - 1) / Gw);
    return c;
}

// 8 consecutive channels of one map pixel as floats: one 16-byte load (f16) or two (f32)
__device__ __forceinline__ void load8(const __half *p, float v[8]) {
    const uint4 raw = *reinterpret_cast<const uint4 *>(p);
    const __half2 *h2 = reinterpret_cast<const __half2 *>(&raw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float2 f = __half22float2(h2[k]);
        v[2 * k] = f.x;
        v[2 * k + 1] = f.y;
    }
}

__device__ __forceinline__ void load8(const float *p, float v[8]) {
    const floatx4 a = *reinterpret_cast<const floatx4 *>(p), b = *reinterpret_cast<const floatx4 *>(p + 4);
    v[0] = a.x;
    v[1] = a.y;
    v[2] = a.z;
    v[3] = a.w;
    v[4] = b.x;
    v[5] = b.y;
    v[6] = b.z;
    v[7] = b.w;
}

__device__ __forceinline__ float load1(const __half *p) { return __half2float(*p); }
__device__ __forceinline__ float load1(const float *p) { return *p; }

// One 256-thread workgroup per (cell, image): blockIdx.x = i * Gw + j, blockIdx.y = n.  VEC: C % 8 == 0 and a 16-byte aligned
// map -- a lane owns 8 consecutive channels, so the 256 lanes read 2048 channels of a pixel as full rows; otherwise a lane
// owns single channels.  Lane 0 writes the cell's box.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void grid_pool_kernel(const T *__restrict__ map, int Hm, int Wm, int C,
                                                        const int32_t *__restrict__ image_hw, const float *__restrict__ scales_yx,
                                                        int S, int Gh, int Gw, float *__restrict__ feat, int ldf,
                                                        float *__restrict__ boxes) {
    const int cell = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int i = cell / Gw, j = cell - i * Gw;
    const int h = image_hw[2 * n], w = image_hw[2 * n + 1];
    const GridCell g = grid_cell(h, w, Hm, Wm, S, Gh, Gw, i, j);
    const long row = (long)n * (Gh * Gw) + cell;
    if (tid == 0) {
        float x0 = (float)(g.xs * S), y0 = (float)(g.ys * S);
        float x1 = fminf((float)((long)g.xe * S), (float)w), y1 = fminf((float)((long)g.ye * S), (float)h);
        if (scales_yx) {       // boxes[:, 0::2] *= scale_yx[1]; boxes[:, 1::2] *= scale_yx[0]  (frcnn.py:1280-1283)
            const float sy = scales_yx[2 * n], sx = scales_yx[2 * n + 1];
            x0 *= sx;
            x1 *= sx;
            y0 *= sy;
            y1 *= sy;
        }
        float *b = boxes + row * 4;
        b[0] = x0;
        b[1] = y0;
        b[2] = x1;
        b[3] = y1;
    }
    const double count = (double)((g.ye - g.ys) * (g.xe - g.xs));
    const T *img = map + (long)n * Hm * Wm * C;
    float *dst = feat + row * ldf;
    if constexpr (VEC) {
        for (int c0 = tid * 8; c0 < C; c0 += 256 * 8) {
            double acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
            for (int y = g.ys; y < g.ye; ++y) {
                const T *p = img + ((long)y * Wm + g.xs) * C + c0;
#pragma unroll 4
                for (int x = g.xs; x < g.xe; ++x, p += C) {
                    float v[8];
                    load8(p, v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] += (double)v[k];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[c0 + k] = (float)(acc[k] / count);
        }
    } else {
        for (int c = tid; c < C; c += 256) {
            double acc = 0.;
            for (int y = g.ys; y < g.ye; ++y) {
                const T *p = img + ((long)y * Wm + g.xs) * C + c;
                for (int x = g.xs; x < g.xe; ++x, p += C) acc += (double)load1(p);
            }
            dst[c] = (float)(acc / count);
        }
    }
}

template <typename T>
static void launch_grid_typed(const void *map, int N, int Hm, int Wm, int C, const int32_t *image_hw, const float *scales_yx,
                              int S, int Gh, int Gw, float *feat, int ldf, float *boxes, hipStream_t s) {
    const bool vec = C % 8 == 0 && ((uintptr_t)map & 15) == 0;
    const dim3 grid(Gh * Gw, N), block(256);
    if (vec)
        hipLaunchKernelGGL((grid_pool_kernel<T, true>), grid, block, 0, s, (const T *)map, Hm, Wm, C, image_hw, scales_yx, S, Gh, Gw,
                           feat, ldf, boxes);
    else
        hipLaunchKernelGGL((grid_pool_kernel<T, false>), grid, block, 0, s, (const T *)map, Hm, Wm, C, image_hw, scales_yx, S, Gh, Gw,
                           feat, ldf, boxes);
}

}  // namespace vk

extern "C" {

int vk_grid_pool(const void *map, int N, int Hm, int Wm, int C, vk_dtype dt, const int32_t *image_hw, const float *scales_yx, int S,
                 int Gh, int Gw, float *feat_out, int ldf, float *boxes_out, void *stream) {
    VK_REQUIRE(map && image_hw && feat_out && boxes_out, VK_EINVAL, "grid_pool: null argument");
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32, VK_EINVAL, "grid_pool: the map must be f16 or f32");
    VK_REQUIRE(N >= 1 && N <= 65535 && Hm >= 1 && Wm >= 1 && C >= 1, VK_EINVAL, "grid_pool: bad map N=%d Hm=%d Wm=%d C=%d", N, Hm, Wm, C);
    VK_REQUIRE(S >= 1 && S <= 1024 && (long)Hm * S < (1L << 30) && (long)Wm * S < (1L << 30), VK_EINVAL, "grid_pool: bad stride S=%d", S);
    VK_REQUIRE(Gh >= 1 && Gw >= 1 && (long)Gh * Gw <= 1024, VK_EINVAL, "grid_pool: grid (%d, %d) must have 1..1024 cells", Gh, Gw);
    VK_REQUIRE(ldf >= C, VK_EINVAL, "grid_pool: ldf=%d is smaller than C=%d", ldf, C);
    hipStream_t s = (hipStream_t)stream;
    if (dt == VK_F16)
        vk::launch_grid_typed<__half>(map, N, Hm, Wm, C, image_hw, scales_yx, S, Gh, Gw, feat_out, ldf, boxes_out, s);
    else
        vk::launch_grid_typed<float>(map, N, Hm, Wm, C, image_hw, scales_yx, S, Gh, Gw, feat_out, ldf, boxes_out, s);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
