// Per-class NMS selection on gfx950 (roi_outputs.selection = "per_class"): the selection rule of the
// bottom-up-attention feature extraction -- NMS per class, a box's confidence is its best class that survives NMS, boxes at
// or above score_thresh are kept, the count bounded to [min_detections, max_detections].
//
// Built from the reference's own arithmetic (vltk/modeling/frcnn.py):
//   ROIOutputs._predict_objs (soft-max over C+1)                    :1252-1255   class_probs_kernel
//   ROIOutputs._predict_boxes + _clip_box on all R*C boxes          :1242-1250, :121, :147-153   (decoded inside the NMS kernel)
//   torchvision.ops.nms, once per (image, class)                    :132         per_class_nms_kernel
//   scales, gathers                                                 :1280-1291   per_class_final_kernel
// Only the loop over classes, the max over surviving classes and the count rule are this project's (parity with the
// original extraction scripts is unpinned).
//
// Data layout.  Scores stay row-major [K, ld] (one row per RoI, as the soft-max writes them) and the all-class deltas stay the
// GEMM's row-major [K, 4C]: a workgroup of class c reads column c of the scores and columns 4c..4c+3 of the deltas of its
// image's R rows: 4 bytes of each 128-byte line of the scores and 16 of each line of the deltas (32 and 8 classes share a line;
// see per_class_nms_kernel for where they run).  The R*C decoded boxes never go to HBM: a class's
// R boxes are decoded, checked for non-finite values, clipped and kept in LDS, contiguous, for the sort and the sweep.
//
// fp32 box math, reference op order, no FMA contraction (-ffp-contract=off for this file).
#include <cfloat>

#include "vk_common.h"
#include "conv_prims.h"

namespace vk {

constexpr int PC_XCDS = 8;      // accelerator dies of an MI355X; only the order of the classes depends on it, no result does

static __device__ __forceinline__ float pc_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// One wavefront per RoI: out[k][c] = soft-max(logits[k][0:n])[c] for every c < n.  The maximum, the sum (lane partition and
// butterfly order) and the division are those of softmax_argmax_kernel (roi_out.hip), so column c of a row holds the bits
// that kernel reports as the row's obj_prob when c is its arg-max.
__global__ __launch_bounds__(256) void class_probs_kernel(const float *__restrict__ logits, int ld, int K, int n,
                                                          float *__restrict__ out, int ld_out) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= K) return;
    const float *x = logits + (long)k * ld;
    float m = -INFINITY;
    for (int c = lane; c < n; c += 64) {
        float v = x[c];
        if (v > m) m = v;
    }
    m = pc_wave_max(m);
    float s = 0.f;
    for (int c = lane; c < n; c += 64) s += expf(x[c] - m);
    s = wave_sum(s);
    float *o = out + (long)k * ld_out;
    for (int c = lane; c < n; c += 64) o[c] = expf(x[c] - m) / s;
}

// pc_box, the box of (row, class), is in vk_common.h: detections.hip decodes with the same function.

// One wavefront per (class, image): blockIdx.y = n, and blockIdx.x -> class so that the workgroups one XCD receives
// (consecutive workgroup ids go round the 8 XCDs) hold a contiguous run of classes: the classes that share a cache line of
// the strided columns then meet in one XCD's L2 instead of each XCD fetching the line for itself.  LDS: keys[Rp2] u64 | box[R][4] f32 | removed[R] i32 |
// score bits[R] u32 (what a survivor merges, kept from the load that built the keys).
// Greedy NMS in roi_final_kernel's arithmetic (scores descending, ties to the lower row; areas without +1; suppressed iff
// (double)(inter / (a_i + a_j - inter)) > thresh).  Every survivor r raises best[r] to (score bits << 32) | (C - c): a 64-bit
// unsigned maximum orders by score first (non-negative floats order like their bits) and, among equal scores, by the smaller
// class; 0 stays "survives in no class".
__global__ __launch_bounds__(64) void per_class_nms_kernel(PerClassArgs a, int Rp2) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem_raw);
    float *sbox = reinterpret_cast<float *>(keys + Rp2);
    int *removed = reinterpret_cast<int *>(sbox + (size_t)a.R * 4);
    uint32_t *sbits = reinterpret_cast<uint32_t *>(removed + a.R);

    const int n = blockIdx.y, lane = threadIdx.x;
    const int c = (int)(blockIdx.x % PC_XCDS) * (int)(gridDim.x / PC_XCDS) + (int)(blockIdx.x / PC_XCDS);
    const int cnt = max(0, min(a.counts[n], a.R));
    if (c >= a.C || cnt == 0) return;              // grid.x is C rounded up to a multiple of PC_XCDS
    int np2 = 2;                                   // the sort runs over the image's own count, not the capacity
    while (np2 < cnt) np2 <<= 1;
    const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
    const long k0 = (long)n * a.R;

    bool bad = false;
    for (int r = lane; r < np2; r += 64) {
        if (r < cnt) {
            float b[4];
            if (!pc_box(a, k0 + r, c, img_w, img_h, b)) bad = true;
            sbox[4 * r + 0] = b[0];
            sbox[4 * r + 1] = b[1];
            sbox[4 * r + 2] = b[2];
            sbox[4 * r + 3] = b[3];
            removed[r] = 0;
            const float sc = a.scores[(k0 + r) * a.ld_scores + c];
            sbits[r] = sc > 0.f ? __float_as_uint(sc) : 0u;                // probabilities: -0 and NaN count as 0
            keys[r] = ((unsigned long long)desc_key32(sc) << 32) | (uint32_t)r;
        } else {
            keys[r] = ~0ull;
        }
    }
    if (bad) atomicOr(a.nonfinite, 1);
    __syncthreads();

    for (int k2 = 2; k2 <= np2; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = lane; i < np2; i += 64) {
                int ixj = i ^ j2;
                if (ixj > i) {
                    unsigned long long x = keys[i], y = keys[ixj];
                    bool up = (i & k2) == 0;
                    if ((x > y) == up) {
                        keys[i] = y;
                        keys[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }

    const double thr = a.thresh;
    for (int i = 0; i < cnt; ++i) {
        __syncthreads();
        if (removed[i]) continue;
        const int ri = (int)(keys[i] & 0xFFFFFFFFull);
        if (lane == 0) atomicMax(a.best + k0 + ri, ((unsigned long long)sbits[ri] << 32) | (uint32_t)(a.C - c));
        const float ix1 = sbox[4 * ri], iy1 = sbox[4 * ri + 1], ix2 = sbox[4 * ri + 2], iy2 = sbox[4 * ri + 3];
        const float ia = (ix2 - ix1) * (iy2 - iy1);
        for (int j = i + 1 + lane; j < cnt; j += 64) {
            if (removed[j]) continue;
            const int rj = (int)(keys[j] & 0xFFFFFFFFull);
            const float jx1 = sbox[4 * rj], jy1 = sbox[4 * rj + 1], jx2 = sbox[4 * rj + 2], jy2 = sbox[4 * rj + 3];
            const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
            const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
            const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
            const float inter = w * h;
            const float ja = (jx2 - jx1) * (jy2 - jy1);
            const float ovr = inter / (ia + ja - inter);
            if ((double)ovr > thr) removed[j] = 1;
        }
    }
}

// One workgroup per image, in the shape of roi_final_kernel.  LDS: keys[Rp2] u64 | n_ge i32.  Rank by max_conf descending
// (ties to the lower row), n_out = min(max(#{max_conf >= score_thresh}, mind), maxd, count), gather the first n_out.
__global__ __launch_bounds__(256) void per_class_final_kernel(PerClassArgs a, int Rp2) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem_raw);
    int *n_ge = reinterpret_cast<int *>(keys + Rp2);

    const int n = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int cnt = max(0, min(a.counts[n], a.R));
    const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
    const long k0 = (long)n * a.R;

    if (tid == 0) *n_ge = 0;
    __syncthreads();
    int ge = 0;
    for (int r = tid; r < Rp2; r += T) {
        float conf = 0.f;
        if (r < cnt) {
            conf = __uint_as_float((uint32_t)(a.best[k0 + r] >> 32));
            keys[r] = ((unsigned long long)desc_key32(conf) << 32) | (uint32_t)r;
            if ((double)conf >= a.score_thresh) ++ge;
        } else {
            keys[r] = ~0ull;
        }
        if (a.max_conf && r < a.R) a.max_conf[k0 + r] = conf;
    }
    if (ge) atomicAdd(n_ge, ge);
    __syncthreads();

    for (int k2 = 2; k2 <= Rp2; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = tid; i < Rp2; i += T) {
                int ixj = i ^ j2;
                if (ixj > i) {
                    unsigned long long x = keys[i], y = keys[ixj];
                    bool up = (i & k2) == 0;
                    if ((x > y) == up) {
                        keys[i] = y;
                        keys[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }

    const int nk = min(min(max(*n_ge, a.mind), a.maxd), cnt);

    const float sy = a.scales_yx ? a.scales_yx[2 * n] : 1.f, sx = a.scales_yx ? a.scales_yx[2 * n + 1] : 1.f;
    const long o0 = (long)n * a.D;
    for (int d = tid; d < a.D; d += T) {
        float b[4] = {0.f, 0.f, 0.f, 0.f}, op = 0.f, ap = 0.f;
        int64_t oc = 0, ac = 0, kid = 0;
        if (d < nk) {
            const int r = (int)(keys[d] & 0xFFFFFFFFull);
            const unsigned long long best = a.best[k0 + r];
            const uint32_t low = (uint32_t)(best & 0xFFFFFFFFull);
            const int cls = low ? a.C - (int)low : 0;
            pc_box(a, k0 + r, cls, img_w, img_h, b);        // the bits the NMS kernel held for (r, cls)
            if (a.scales_yx) {   // boxes[:,0::2] *= scale_yx[1]; boxes[:,1::2] *= scale_yx[0]  (:1280-1283)
                b[0] *= sx;
                b[2] *= sx;
                b[1] *= sy;
                b[3] *= sy;
            }
            op = __uint_as_float((uint32_t)(best >> 32));
            oc = cls;
            ap = a.attr_prob ? a.attr_prob[k0 + r] : 0.f;
            ac = a.attr_cls ? a.attr_cls[k0 + r] : 0;
            kid = r;
        }
        a.out.boxes[(o0 + d) * 4 + 0] = b[0];
        a.out.boxes[(o0 + d) * 4 + 1] = b[1];
        a.out.boxes[(o0 + d) * 4 + 2] = b[2];
        a.out.boxes[(o0 + d) * 4 + 3] = b[3];
        a.out.obj_probs[o0 + d] = op;
        a.out.obj_ids[o0 + d] = oc;
        a.out.attr_probs[o0 + d] = ap;
        a.out.attr_ids[o0 + d] = ac;
        if (a.keep_ids) a.keep_ids[o0 + d] = kid;
    }
    if (tid == 0) a.out.preds_per_image[n] = nk;
    const int F4 = a.F / 4;
    for (int d = 0; d < a.D; ++d) {
        floatx4 *dst = reinterpret_cast<floatx4 *>(a.out.roi_features + (o0 + d) * a.F);
        if (d < nk) {
            const int r = (int)(keys[d] & 0xFFFFFFFFull);
            const floatx4 *src = reinterpret_cast<const floatx4 *>(a.features + (k0 + r) * a.F);
            for (int i = tid; i < F4; i += T) dst[i] = src[i];
        } else {
            const floatx4 z = {0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < F4; i += T) dst[i] = z;
        }
    }
}

// Every (row, class) box as the NMS kernel holds it in LDS, written out: out [N*R, C, 4].  Rows >= counts[n] are zero.  Not
// on the forward's path (which never materialises the R*C boxes); for callers and tests that want the device's own bits.
__global__ __launch_bounds__(256) void class_boxes_kernel(PerClassArgs a, float *__restrict__ out) {
    const int n = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.R * a.C) return;
    const int r = (int)(i / a.C), c = (int)(i % a.C);
    const int cnt = max(0, min(a.counts[n], a.R));
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < cnt) {
        const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
        if (!pc_box(a, (long)n * a.R + r, c, img_w, img_h, b) && a.nonfinite) atomicOr(a.nonfinite, 1);
    }
    float *o = out + (((long)n * a.R + r) * a.C + c) * 4;
    o[0] = b[0];
    o[1] = b[1];
    o[2] = b[2];
    o[3] = b[3];
}

int launch_class_boxes(PerClassArgs &a, int N, float *out, hipStream_t s) {
    VK_REQUIRE(N >= 1 && N <= 65535 && a.R >= 1 && a.R <= 1024 && a.C >= 1, VK_EINVAL, "class_boxes: N=%d R=%d C=%d", N, a.R, a.C);
    VK_REQUIRE(a.ld_box >= (a.agnostic ? 4 : 4 * a.C), VK_EINVAL, "class_boxes: ld_box=%d is shorter than a row", a.ld_box);
    hipLaunchKernelGGL(class_boxes_kernel, dim3((unsigned)ceil_div(a.R * a.C, 256), N), dim3(256), 0, s, a, out);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int launch_class_probs(const float *logits, int ld, int K, int n, float *out, int ld_out, hipStream_t s) {
    if (K == 0) return VK_OK;
    hipLaunchKernelGGL(class_probs_kernel, dim3(ceil_div(K, 4)), dim3(256), 0, s, logits, ld, K, n, out, ld_out);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

// a.best is zeroed here; a.nonfinite is the caller's to zero (it may already hold an earlier stage's flag)
int launch_per_class_select(PerClassArgs &a, int N, hipStream_t s) {
    VK_REQUIRE(N >= 1 && N <= 65535, VK_EINVAL, "per_class: N=%d must be in 1..65535", N);
    VK_REQUIRE(a.R >= 1 && a.R <= 1024, VK_EINVAL, "per_class: R=%d must be in 1..1024", a.R);
    VK_REQUIRE(a.D >= 1 && a.D <= a.R, VK_EINVAL, "per_class: max_detections=%d must be in 1..R", a.D);
    VK_REQUIRE(a.C >= 1, VK_EINVAL, "per_class: C=%d classes", a.C);
    VK_REQUIRE(a.F % 4 == 0, VK_EINVAL, "per_class: F must be a multiple of 4");
    VK_REQUIRE(a.ld_scores >= a.C && a.ld_box >= (a.agnostic ? 4 : 4 * a.C), VK_EINVAL, "per_class: row strides ld_scores=%d ld_box=%d "
               "are shorter than the rows", a.ld_scores, a.ld_box);
    int Rp2 = 2;
    while (Rp2 < a.R) Rp2 <<= 1;
    VK_CHECK_HIP(hipMemsetAsync(a.best, 0, sizeof(unsigned long long) * (size_t)N * a.R, s));
    const size_t smem_nms = (size_t)Rp2 * 8 + (size_t)a.R * 16 + (size_t)a.R * 4 + (size_t)a.R * 4;
    hipLaunchKernelGGL(per_class_nms_kernel, dim3(ceil_div(a.C, PC_XCDS) * PC_XCDS, N), dim3(64), smem_nms, s, a, Rp2);
    VK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(per_class_final_kernel, dim3(N), dim3(256), (size_t)Rp2 * 8 + 16, s, a, Rp2);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk
