// The row LayerNorm every encoder of the package shares, and the gather pieces in front of it.  One wave per row, four rows per
// workgroup; a lane owns the chunks lane, lane + 64, ... of the row: VW = 16 / sizeof(T) elements (one 16-byte access) on the
// chunk form, VW = 1 otherwise.  The kernels of layernorm.hip, visualbert.hip and layoutlm.hip differ only in how a chunk of the
// row comes to be (their loaders); everything after that is row_layernorm, so equal rows give equal bits in every entry.
// No LDS, no atomics.  DESIGN.md section 20a has the error bound.
#pragma once
#include "vk_common.h"

namespace vk {

constexpr int ROW_MAX_PER_LANE = 32;     // rows up to 2048 elements
constexpr int ROW_MAX_C = 64 * ROW_MAX_PER_LANE;

// VW consecutive elements as fp32, and back with one rounding each: one 16-byte access where VW = 16 / sizeof(T) (p then 16-byte
// aligned), one element where VW = 1.  A table index clamped into a table of n rows.
template <typename T, int VW>
__device__ __forceinline__ void ld_chunk(const T *p, float (&out)[VW]) {
    if constexpr (VW == 1) {
        out[0] = (float)*p;
    } else {
        typedef T vecT __attribute__((ext_vector_type(VW)));
        const vecT t = *reinterpret_cast<const vecT *>(p);
#pragma unroll
        for (int e = 0; e < VW; ++e) out[e] = (float)t[e];
    }
}
template <typename T, int VW>
__device__ __forceinline__ void st_chunk(T *p, const float (&v)[VW]) {
    if constexpr (VW == 1) {
        *p = (T)v[0];
    } else {
        typedef T vecT __attribute__((ext_vector_type(VW)));
        vecT o;
#pragma unroll
        for (int e = 0; e < VW; ++e) o[e] = (T)v[e];
        *reinterpret_cast<vecT *>(p) = o;
    }
}
__device__ __forceinline__ long clamp_row(long i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// The two places where the compiler's contraction rounded differently in the two forms when each kernel had its own copy of the
// loops, pinned so that every form keeps its bits: q + d * d of the variance (a chunk's packed multiplies round the square, a
// single element fuses it into the add) and r * scale + old of the accumulate (fused on a chunk, two roundings on an element).
template <int VW>
__device__ __forceinline__ float add_square(float q, float d) {
    if constexpr (VW == 1) {
        return __builtin_fmaf(d, d, q);
    } else {
#pragma clang fp contract(off)
        return q + d * d;
    }
}
template <int VW>
__device__ __forceinline__ float scale_add(float r, float scale, float old) {
    if constexpr (VW == 1) {
#pragma clang fp contract(off)
        return r * scale + old;
    } else {
        return __builtin_fmaf(r, scale, old);
    }
}

// One wave's row: yr[0:C] = scale * LayerNorm(row) (+ yr[0:C] when accumulate), C % VW == 0.  load(ch, out) yields the chunk ch
// of the row as fp32.  Mean and biased variance in fp32 over the loaded values (the lane's chunks in order, then six shuffle
// steps), (v - mean) / sqrt(var + eps) * gamma + beta like at::native::layer_norm, one rounding on the store.
template <typename T, int VW, typename Load>
__device__ __forceinline__ void row_layernorm(int C, int lane, Load load, const float *__restrict__ gamma,
                                              const float *__restrict__ beta, float eps, float scale, int accumulate, T *yr) {
    constexpr int MAXC = ROW_MAX_PER_LANE / VW;          // chunks per lane
    const int chunks = C / VW;
    float v[MAXC][VW];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = lane + 64 * i;
        if (ch < chunks) {
            load(ch, v[i]);
#pragma unroll
            for (int e = 0; e < VW; ++e) s += v[i][e];
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (lane + 64 * i < chunks) {
#pragma unroll
            for (int e = 0; e < VW; ++e) q = add_square<VW>(q, v[i][e] - mean);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = lane + 64 * i;
        if (ch < chunks) {
            float o[VW], old[VW];
            if (accumulate) ld_chunk<T, VW>(yr + ch * VW, old);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const float r = (v[i][e] - mean) * rstd * gamma[ch * VW + e] + beta[ch * VW + e];
                o[e] = accumulate ? scale_add<VW>(r, scale, old[e]) : r * scale;
            }
            st_chunk<T, VW>(yr + ch * VW, o);
        }
    }
}

// The launch rule.  The chunk form is taken only when the row length and every row stride (`dims`: all of them OR-ed) are
// multiples of vw = 16 / sizeof(T) and every base (`bases`: all of them OR-ed) is 16-byte aligned; four rows to a workgroup.
static inline bool row_chunked(int vw, int dims, uintptr_t bases) { return dims % vw == 0 && bases % 16 == 0; }
template <typename... P, typename... A>
static inline int row_launch(void (*kernel)(P...), long rows, hipStream_t s, A &&...args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, static_cast<A &&>(args)...);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk
