// The DROP forms of attention_tiled_kernel (attention_tiled.h) and of ag16_dq_kernel / ag16_dkv_kernel (attention_grad16.h) with their
// entry points, vk_attention_tiled_dropout and vk_attention_grad_16_dropout.  A unit of its own, built without
// packed fp32 instructions as new kernels here are; the objects of attention.hip and attention_grad16.hip stay what they were.
#include "attention_grad16.h"
#include "attention_tiled.h"

namespace vk {

// vk_attention_tiled_dropout: the tiled kernel or a refusal (the DROP form exists for the 16-bit matrix-core kernel alone)
static int launch_attention_dropout(const AttArgs &a, const DropArgs &da, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)a.d);
    VK_REQUIRE((long)a.B * a.heads * ((a.Lq + 15) / 16) < (1L << 31), VK_EINVAL, "attention: too many (batch, head, query block) items");
    int st = VK_EINVAL;
    VK_DT16_D_SWITCH(a.dt, a.d, st = tiled_launch<T, D>(a, scale, s, da));
    VK_TRY(st);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

// vk_attention_tiled with dropout on the probabilities (the rule of philox.h; `stream` of the counter is `drop_stream`): the DROP
// form of attention_tiled_kernel, so only where the rule routes to it: bf16 / fp16, head dim 32 / 64, 16-byte aligned rows.
int vk_attention_tiled_dropout(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask, void *out, int ldo,
                               int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream, float p, uint64_t seed,
                               uint64_t drop_stream) {
    const AttArgs a = {q, k, v, mask, out, ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d, dt};
    VK_TRY(check_attention_args(a));
    const int t = dropout_threshold(p);
    VK_REQUIRE(t >= 0, VK_EINVAL, "attention_tiled_dropout: the rate %g must lie in [0, 1) and round to at most 255 / 256", (double)p);
    const int aligned = ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0;
    const int route = vk_attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, aligned, 1);      // the rule of attention.hip, asked as the tiled entry
    if (route < 0) return -route;
    VK_REQUIRE(route == VK_ATT_ROUTE_TILED, VK_EINVAL,
               "attention_tiled_dropout: only the tiled matrix-core kernel drops probabilities (bf16 / fp16, head dim 32 / 64, 16-byte "
               "aligned rows, leading dimensions in multiples of 8); these arguments route to kernel %d", route);
    const DropArgs da = {(uint32_t)t, dropout_scale(t), seed, drop_stream};
    return launch_attention_dropout(a, da, (hipStream_t)stream);
}

// The backward of vk_attention_tiled_dropout under the same (p, seed, drop_stream): o is the dropped forward's output.  The
// workspace and the checks are vk_attention_grad_16's.
size_t vk_attention_grad_16_dropout_workspace_bytes(int B, int heads, int Lq) { return ag16_workspace_bytes(B, heads, Lq); }

int vk_attention_grad_16_dropout_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask,
                                       const void *o, long ldo, const void *dout, long lddo, const float *dq, long lddq, const float *dk,
                                       long lddk, const float *dv, long lddv, int B, int heads, int Lq, int Lk, int d, vk_dtype dt,
                                       const void *workspace, size_t workspace_bytes, float p) {
    (void)mask;
    VK_TRY(ag16_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, dt, workspace,
                      workspace_bytes));
    VK_REQUIRE(dropout_threshold(p) >= 0, VK_EINVAL, "attention_grad_16_dropout: the rate %g must lie in [0, 1) and round to at most 255 / 256",
               (double)p);
    return VK_OK;
}

int vk_attention_grad_16_dropout(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o,
                                 long ldo, const void *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv,
                                 int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream,
                                 float p, uint64_t seed, uint64_t drop_stream) {
    VK_TRY(vk_attention_grad_16_dropout_check(q, ldq, k, ldk, v, ldv, mask, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk,
                                              d, dt, workspace, workspace_bytes, p));
    const AttGrad16Args a = {q, k, v, o, dout, mask, dq, dk, dv, (float *)workspace, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                             B, heads, Lq, Lk, 1.0f / sqrtf((float)d)};
    const int t = dropout_threshold(p);
    const DropArgs da = {(uint32_t)t, dropout_scale(t), seed, drop_stream};
    VK_DT16_D_SWITCH(dt, d, return ag16_launch<T, D>(a, (hipStream_t)stream, da));
}

}  // extern "C"
