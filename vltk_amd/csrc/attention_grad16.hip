// vk_attention_grad_16 and its helpers: the plain forms of the kernels of attention_grad16.h.
#include "attention_grad16.h"

using namespace vk;

extern "C" {

size_t vk_attention_grad_16_workspace_bytes(int B, int heads, int Lq) { return ag16_workspace_bytes(B, heads, Lq); }

int vk_attention_grad_16_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o,
                               long ldo, const void *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk,
                               const float *dv, long lddv, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, const void *workspace,
                               size_t workspace_bytes) {
    (void)mask;                     // may be NULL: no key is masked
    return ag16_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, dt, workspace,
                      workspace_bytes);
}

int vk_attention_grad_16(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o, long ldo,
                         const void *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, int B, int heads,
                         int Lq, int Lk, int d, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream) {
    VK_TRY(ag16_check(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, heads, Lq, Lk, d, dt, workspace,
                      workspace_bytes));
    const AttGrad16Args a = {q, k, v, o, dout, mask, dq, dk, dv, (float *)workspace, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                             B, heads, Lq, Lk, 1.0f / sqrtf((float)d)};
    VK_DT16_D_SWITCH(dt, d, return ag16_launch<T, D>(a, (hipStream_t)stream));
}

}  // extern "C"
