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
// see select_class, select_prims.h, for where they run).  The R*C decoded boxes never go to HBM: a class's
// R boxes are decoded, checked for non-finite values, clipped and kept in LDS, contiguous, for the sort and the sweep.
//
// fp32 box math, reference op order, no FMA contraction (-ffp-contract=off for this file).
#include <cfloat>

#include "vk_common.h"
#include "select_prims.h"

namespace vk {

constexpr int PC_FINAL_THREADS = 256;

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
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < n; c += 64) s += expf(x[c] - m);
    s = wave_sum(s);
    float *o = out + (long)k * ld_out;
    for (int c = lane; c < n; c += 64) o[c] = expf(x[c] - m) / s;
}

// pc_box, the box of (row, class), is in vk_common.h: detections.hip decodes with the same function.

// One wavefront per (class, image): blockIdx.y = n, blockIdx.x -> class by select_class (select_prims.h).  LDS: SelectLds with
// score bits[R] u32 as its fourth piece (what a survivor merges, kept from the load that built the keys).
// Greedy NMS by sweep_mark, the sweep of roi_final_kernel (scores descending, ties to the lower row; suppression by
// nms_suppresses).  Every survivor r raises best[r] to (score bits << 32) | (C - c): a 64-bit unsigned maximum orders by score
// first (non-negative floats order like their bits) and, among equal scores, by the smaller class; 0 stays "survives in no
// class".
__global__ __launch_bounds__(64) void per_class_nms_kernel(PerClassArgs a, int Rp2) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const SelectLds lds(smem_raw, Rp2, a.R);
    unsigned long long *keys = lds.keys;
    float *sbox = lds.box;
    int *removed = lds.removed;
    uint32_t *sbits = reinterpret_cast<uint32_t *>(lds.extra);

    const int n = blockIdx.y, lane = threadIdx.x;
    const int c = select_class();
    const int cnt = max(0, min(a.counts[n], a.R));
    if (c >= a.C || cnt == 0) return;
    const int np2 = next_pow2(cnt);                // the sort runs over the image's own count, not the capacity
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
            keys[r] = score_key(sc, (uint32_t)r);
        } else {
            keys[r] = KEY_BEHIND_ALL;
        }
    }
    if (bad) atomicOr(a.nonfinite, 1);
    __syncthreads();

    lds_sort_keys<64>(keys, np2);

    const double thr = a.thresh;
    for (int i = 0; i < cnt; ++i) {
        __syncthreads();
        if (removed[i]) continue;
        const int ri = (int)key_low(keys[i]);
        if (lane == 0) atomicMax(a.best + k0 + ri, ((unsigned long long)sbits[ri] << 32) | (uint32_t)(a.C - c));
        sweep_mark<64, true>(keys, sbox, removed, i, ri, cnt, thr);
    }
}

// One workgroup per image, in the shape of roi_final_kernel.  LDS: keys[Rp2] u64 | n_ge i32.  Rank by max_conf descending
// (ties to the lower row), n_out = min(max(#{max_conf >= score_thresh}, mind), maxd, count), gather the first n_out.
__global__ __launch_bounds__(PC_FINAL_THREADS) void per_class_final_kernel(PerClassArgs a, int Rp2) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem_raw);
    int *n_ge = reinterpret_cast<int *>(keys + Rp2);
    constexpr int T = PC_FINAL_THREADS;

    const int n = blockIdx.x, tid = threadIdx.x;
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
            keys[r] = score_key(conf, (uint32_t)r);
            if ((double)conf >= a.score_thresh) ++ge;
        } else {
            keys[r] = KEY_BEHIND_ALL;
        }
        if (a.max_conf && r < a.R) a.max_conf[k0 + r] = conf;
    }
    if (ge) atomicAdd(n_ge, ge);
    __syncthreads();

    lds_sort_keys<T>(keys, Rp2);

    const int nk = min(min(max(*n_ge, a.mind), a.maxd), cnt);

    const long o0 = (long)n * a.D;
    for (int d = tid; d < a.D; d += T) {
        OutRow o;
        if (d < nk) {
            const int r = (int)key_low(keys[d]);
            const unsigned long long best = a.best[k0 + r];
            const uint32_t low = (uint32_t)(best & 0xFFFFFFFFull);
            const int cls = low ? a.C - (int)low : 0;
            pc_box(a, k0 + r, cls, img_w, img_h, o.box);        // the bits the NMS kernel held for (r, cls)
            o.obj_prob = __uint_as_float((uint32_t)(best >> 32));
            o.obj_id = cls;
            o.attr_prob = a.attr_prob ? a.attr_prob[k0 + r] : 0.f;
            o.attr_id = a.attr_cls ? a.attr_cls[k0 + r] : 0;
            o.keep_id = r;
        }
        store_output_row(a.out, a.keep_ids, o0 + d, d < nk, o, a.scales_yx, n);
    }
    if (tid == 0) a.out.preds_per_image[n] = nk;
    copy_feature_rows<T>(a.features + k0 * a.F, a.out.roi_features + o0 * a.F, a.F, a.D, nk, [&](int d) { return (int)key_low(keys[d]); });
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
    VK_TRY(check_select_shape("per_class", a.R, a.D, a.R, "R"));
    VK_REQUIRE(a.C >= 1, VK_EINVAL, "per_class: C=%d classes", a.C);
    VK_REQUIRE(a.F % 4 == 0, VK_EINVAL, "per_class: F must be a multiple of 4");
    VK_REQUIRE(a.ld_scores >= a.C && a.ld_box >= (a.agnostic ? 4 : 4 * a.C), VK_EINVAL, "per_class: row strides ld_scores=%d ld_box=%d "
               "are shorter than the rows", a.ld_scores, a.ld_box);
    const int Rp2 = next_pow2(a.R);
    VK_CHECK_HIP(hipMemsetAsync(a.best, 0, sizeof(unsigned long long) * (size_t)N * a.R, s));
    hipLaunchKernelGGL(per_class_nms_kernel, dim3(select_class_grid(a.C), N), dim3(64), SelectLds::bytes(Rp2, a.R, a.R), s, a, Rp2);
    VK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(per_class_final_kernel, dim3(N), dim3(PC_FINAL_THREADS), (size_t)Rp2 * 8 + 16, s, a, Rp2);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk
