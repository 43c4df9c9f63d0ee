// What vk_attention_relpos (attention_relpos.hip) and its backward (attention_relpos_grad.hip) agree on: the folded table of a
// head, T1 | TX | TY side by side, and the index of a (key, query) pair into one of them.
#pragma once
#include "vk_common.h"

namespace vk {

constexpr size_t RELPOS_LUT_MAX = 8 * 1024;     // LDS budget of one head's table: (2 r1 + 1) + 2 (2 r2 + 1) floats (128 / 256: 5132 bytes)
constexpr int RP_KT = 64;                       // keys per tile

static inline int relpos_lut_len(int r1, int r2) { return (2 * r1 + 1) + 2 * (2 * r2 + 1); }

__device__ __forceinline__ int rp_idx(int dk, int dq, int r) { return min(max(dk - dq, -r), r) + r; }

}  // namespace vk
