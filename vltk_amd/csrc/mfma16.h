// v_mfma_f32_16x16x32 on 16-bit operands for the training kernels (gemm16.hip, attention_grad16.hip), templated on the storage type
// the way AttFrag<T> is in attention.hip.  Lane l = 16 g + j holds, in element e = 0..7 of its fragment, A[row j][k = 8 g + e] and
// B[k = 8 g + e][column j]; register r of the result is D[row 4 g + r][column j].
#pragma once
#include "vk_common.h"

namespace vk {

typedef _Float16 m16_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 m16_b8 __attribute__((ext_vector_type(8)));
typedef float m16_f4 __attribute__((ext_vector_type(4)));

template <typename T>
struct Mma16;
template <>
struct Mma16<_Float16> {
    typedef m16_h8 frag;
    static __device__ __forceinline__ m16_f4 mma(m16_h8 a, m16_h8 b, m16_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <>
struct Mma16<__bf16> {
    typedef m16_b8 frag;
    static __device__ __forceinline__ m16_f4 mma(m16_b8 a, m16_b8 b, m16_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// two 16-bit values as one 32-bit word, `lo` in the low half
template <typename T>
__device__ __forceinline__ unsigned pack16(T lo, T hi) {
    unsigned short ulo, uhi;
    __builtin_memcpy(&ulo, &lo, 2);
    __builtin_memcpy(&uhi, &hi, 2);
    return (unsigned)ulo | ((unsigned)uhi << 16);
}

// 8 consecutive elements at p (16-byte aligned) of which the first `valid` lie inside the matrix: one 16-byte load where all do,
// element loads and zeros otherwise; nothing is read through p where valid <= 0.
template <typename T>
__device__ __forceinline__ typename Mma16<T>::frag load8(const T *p, int valid) {
    typedef typename Mma16<T>::frag frag;
    if (valid >= 8) return *reinterpret_cast<const frag *>(p);
    frag t = {};
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < valid) t[e] = p[e];
    return t;
}

}  // namespace vk
