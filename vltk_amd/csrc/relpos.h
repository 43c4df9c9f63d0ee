// What vk_attention_relpos (attention_relpos.hip) and its backward (attention_relpos_grad.hip) agree on: the folded table of a
// head, T1 | TX | TY side by side, the index of a (key, query) pair into one of them, and the score that carries the bias.
#pragma once
#include "vk_common.h"

namespace vk {

constexpr size_t RELPOS_LUT_MAX = 8 * 1024;     // LDS budget of one head's table: (2 r1 + 1) + 2 (2 r2 + 1) floats (128 / 256: 5132 bytes)

static inline int relpos_lut_len(int r1, int r2) { return (2 * r1 + 1) + 2 * (2 * r2 + 1); }

// the radii every entry refuses; `who` is the entry's name
static inline int relpos_lut_check(const char *who, int r1, int r2) {
    VK_REQUIRE(r1 >= 1 && r2 >= 1, VK_EINVAL, "%s: radii must be at least 1 (r1=%d r2=%d)", who, r1, r2);
    VK_REQUIRE((size_t)r1 + 2 * (size_t)r2 <= RELPOS_LUT_MAX / 8 && relpos_lut_len(r1, r2) * sizeof(float) <= RELPOS_LUT_MAX, VK_EINVAL,
               "%s: the table of radii %d / %d, %zu floats a head, is past the LDS budget of %zu bytes", who, r1, r2,
               (size_t)2 * r1 + 4 * (size_t)r2 + 3, RELPOS_LUT_MAX);
    return VK_OK;
}

// what the bias form of attention_stream_kernel takes as its one trailing argument; the plain form takes none
struct RelBias {
    const int32_t *rel_q, *rel_k;       // [B, Lq, 3] and [B, Lk, 3]: (pos, x, y)
    const float *lut;                   // [heads][relpos_lut_len(r1, r2)]
    int r1, r2;
};

template <typename... A>
static __device__ __forceinline__ RelBias rel_bias_of(A... a) {
    if constexpr (sizeof...(A) == 1) return (a, ...);
    else return RelBias{};
}

__device__ __forceinline__ int rp_idx(int dk, int dq, int r) { return min(max(dk - dq, -r), r) + r; }

// the score of a pair: its dot product, the three table reads, in this order of additions, then scale and mask
__device__ __forceinline__ float rp_score(float dot, float t1, float tx, float ty, float scale, float mask) {
    return (dot + (t1 + (tx + ty))) * scale + mask;
}

}  // namespace vk
