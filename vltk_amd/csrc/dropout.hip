// Hidden dropout fused with the residual add, for the trainers: out = (keep ? x * rs : 0) + residual on n
// contiguous floats, under the mask of philox.h (element i is byte i & 15 of granule i >> 4).  With residual = NULL it is also the
// backward of the same site: dy -> keep ? dy * rs : 0.  One rounding per product and one per sum (the file is built without FMA
// contraction and without packed fp32 instructions), so the result is bit-equal to the rule restated in fp32 on the host.
//
// The body: a wave takes 1024 contiguous floats per step as four 16-byte accesses per lane, lane l on float4 number 64 k + l of the
// step, so every access of a wave is 1 KiB contiguous.  Those 256 float4 are 64 granules: lane l makes ONE Philox call, for granule
// l of the step, folds its 16 bytes into 16 keep bits (philox_keep16) and the lanes exchange them: the float4 of access k lies in
// granule 16 k + (l >> 2), whose bits lane 16 k + (l >> 2) holds (one ds_bpermute_b32 per access), and is word l & 3 of it.
// The tail: what is left of n behind the last whole step, or everything where a pointer is not 16-byte aligned, one element per
// thread with a call of its own.  Both run in one launch: the leading workgroups take the body, the rest the tail.
// out may be x or the residual: an element is read and written by one thread.
#include "philox.h"
#include "vk_common.h"

namespace vk {

constexpr int DROP_STEP = 1024;            // floats per wave and step

typedef float drop_f4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float drop_one(float x, bool keep, float rs) { return keep ? x * rs : 0.f; }

template <bool RES>
__global__ __launch_bounds__(256) void dropout_add_kernel(const float *x, const float *res, float *out, long n, long steps, int body_blocks,
                                                         DropArgs da) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < body_blocks) {
        const drop_f4 *x4 = reinterpret_cast<const drop_f4 *>(x), *r4 = reinterpret_cast<const drop_f4 *>(res);
        drop_f4 *o4 = reinterpret_cast<drop_f4 *>(out);
        for (long st = (long)blockIdx.x * 4 + wave; st < steps; st += (long)body_blocks * 4) {
            const uint32_t mine = philox_keep16(philox4x32_10(da.seed, da.stream, (uint64_t)st * 64 + lane), da.t);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long v = st * (DROP_STEP / 4) + k * 64 + lane;
                const uint32_t bits = (uint32_t)__shfl((int)mine, 16 * k + (lane >> 2), 64) >> (lane & 3);
                const drop_f4 a = x4[v];
                drop_f4 y;
#pragma unroll
                for (int c = 0; c < 4; ++c) y[c] = drop_one(a[c], (bits >> (8 * c)) & 1u, da.rs);
                if (RES) {
                    const drop_f4 r = r4[v];
#pragma unroll
                    for (int c = 0; c < 4; ++c) y[c] = y[c] + r[c];
                }
                o4[v] = y;
            }
        }
        return;
    }
    const long first = steps * DROP_STEP, stride = (long)(gridDim.x - body_blocks) * 256;
    for (long i = first + (long)(blockIdx.x - body_blocks) * 256 + threadIdx.x; i < n; i += stride) {
        const Philox4 r = philox4x32_10(da.seed, da.stream, (uint64_t)i >> 4);
        const float y = drop_one(x[i], philox_byte(r, (int)(i & 15)) >= da.t, da.rs);
        out[i] = RES ? y + res[i] : y;
    }
}

}  // namespace vk

using namespace vk;

extern "C" {

int vk_dropout_add_f32(const float *x, const float *residual, float *out, long n, float p, uint64_t seed, uint64_t stream, void *hip_stream) {
    VK_REQUIRE(x && out, VK_EINVAL, "dropout_add_f32: null argument");
    VK_REQUIRE(n >= 1, VK_EINVAL, "dropout_add_f32: n=%ld must be positive", n);
    const int t = dropout_threshold(p);
    VK_REQUIRE(t >= 0, VK_EINVAL, "dropout_add_f32: the rate %g must lie in [0, 1) and round to at most 255 / 256", (double)p);
    const DropArgs da = {(uint32_t)t, dropout_scale(t), seed, stream};
    const bool aligned = (((uintptr_t)x | (uintptr_t)out | (uintptr_t)residual) & 15) == 0;
    const long steps = aligned ? n / DROP_STEP : 0, tail = n - steps * DROP_STEP;
    const int body_blocks = (int)((steps + 3) / 4 < 4096 ? (steps + 3) / 4 : 4096);
    const int tail_blocks = (int)((tail + 255) / 256 < 1024 ? (tail + 255) / 256 : 1024);
    const dim3 grid(body_blocks + tail_blocks);
    if (residual)
        hipLaunchKernelGGL(dropout_add_kernel<true>, grid, dim3(256), 0, (hipStream_t)hip_stream, x, residual, out, n, steps, body_blocks, da);
    else
        hipLaunchKernelGGL(dropout_add_kernel<false>, grid, dim3(256), 0, (hipStream_t)hip_stream, x, residual, out, n, steps, body_blocks, da);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
