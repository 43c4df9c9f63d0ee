// Region features for caller-supplied boxes on gfx950: the two ends of vk_forward_boxes_begin (C4), and of the FPN
// detector's host-composed given-box forward (vk_given_boxes_ingest / vk_given_box_outputs, the ingest with levels).  The
// RoI pool, the head and the box predictor between them are the detection path's own launches.
//
// Replaces (reference vltk/modeling/frcnn.py), for boxes given instead of the RPN's proposals:
//   _clip_box (assert finite, clamp to the image)                  :147-153
//   convert_boxes_to_pooler_format                                 :426-441
//   assign_boxes_to_levels (FPN form only, box_level)              :444-460
//   ROIOutputs._predict_objs / _predict_attrs, the scales multiply :1252-1260, :1280-1283
// with every box kept, in input order: no box regression and no NMS (do_nms :116-143 is not applied).
//
// fp32 box math, no FMA contraction (-ffp-contract=off for this file), IEEE division.
#include "vk_common.h"
#include "select_prims.h"

namespace vk {

// The pyramid-level rule of the FPN form of the ingest (box_level, vk_common.h); unused in the C4 form.
struct LevelRule {
    int32_t *levels;
    int min_level, max_level;
    float canonical_size;
    int canonical_level;
};

// One thread per (n, b) of the [N, B] box grid.  Rows b >= counts[n] are padding: a zero box in prop_boxes and a
// zero-size RoI at the image origin (in-image for RoIPool / RoIAlign, its features are never returned).  LEVELS: also
// the row's pyramid level, from the clipped box (padding rows: the lowest level).
template <bool LEVELS>
__device__ __forceinline__ void ingest_row(const float *__restrict__ boxes, const int32_t *__restrict__ counts,
                                           const int32_t *__restrict__ image_hw, const float *__restrict__ scales_yx, int B,
                                           int total, float *__restrict__ prop_boxes, float *__restrict__ rois,
                                           int32_t *__restrict__ nonfinite, const LevelRule &lr) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const int n = k / B, b = k - n * B;
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    if (b < counts[n]) {
        const float *src = boxes + (long)k * 4;
        x0 = src[0];
        y0 = src[1];
        x1 = src[2];
        y1 = src[3];
        if (scales_yx) {   // original-image pixels -> network input: the inverse of frcnn.py:1280-1283
            const float sy = scales_yx[2 * n], sx = scales_yx[2 * n + 1];
            x0 = x0 / sx;
            x1 = x1 / sx;
            y0 = y0 / sy;
            y1 = y1 / sy;
        }
        if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1))) atomicOr(nonfinite, 1);   // frcnn.py:148
        const float h = (float)image_hw[2 * n], w = (float)image_hw[2 * n + 1];
        x0 = fminf(fmaxf(x0, 0.f), w);
        y0 = fminf(fmaxf(y0, 0.f), h);
        x1 = fminf(fmaxf(x1, 0.f), w);
        y1 = fminf(fmaxf(y1, 0.f), h);
    }
    float *o = prop_boxes + (long)k * 4;
    o[0] = x0;
    o[1] = y0;
    o[2] = x1;
    o[3] = y1;
    float *r = rois + (long)k * 5;
    r[0] = (float)n;
    r[1] = x0;
    r[2] = y0;
    r[3] = x1;
    r[4] = y1;
    if constexpr (LEVELS)   // assign_boxes_to_levels frcnn.py:444-460 on the RoI row just written
        lr.levels[k] = box_level(x0, y0, x1, y1, lr.min_level, lr.max_level, lr.canonical_size, lr.canonical_level);
}

// the C4 model's ingest (RoIPool on res4: no levels)
__global__ __launch_bounds__(256) void given_boxes_ingest_kernel(const float *__restrict__ boxes, const int32_t *__restrict__ counts,
                                                                 const int32_t *__restrict__ image_hw,
                                                                 const float *__restrict__ scales_yx, int B, int total,
                                                                 float *__restrict__ prop_boxes, float *__restrict__ rois,
                                                                 int32_t *__restrict__ nonfinite) {
    ingest_row<false>(boxes, counts, image_hw, scales_yx, B, total, prop_boxes, rois, nonfinite, LevelRule{});
}

// the FPN detector's ingest (RoIAlign over p2..p5: one level per row)
__global__ __launch_bounds__(256) void given_boxes_ingest_levels_kernel(const float *__restrict__ boxes,
                                                                        const int32_t *__restrict__ counts,
                                                                        const int32_t *__restrict__ image_hw,
                                                                        const float *__restrict__ scales_yx, int B, int total,
                                                                        float *__restrict__ prop_boxes, float *__restrict__ rois,
                                                                        int32_t *__restrict__ nonfinite, LevelRule lr) {
    ingest_row<true>(boxes, counts, image_hw, scales_yx, B, total, prop_boxes, rois, nonfinite, lr);
}

// One 128-thread workgroup per output row (b, n): the row's scalars from thread 0, its F-float feature row with 16-byte
// loads and stores (zeros for b >= counts[n]); row 0's thread 0 also writes preds_per_image[n] = counts[n].
__global__ __launch_bounds__(128) void given_box_outputs_kernel(const float *__restrict__ obj_prob, const int32_t *__restrict__ obj_cls,
                                                                const float *__restrict__ attr_prob,
                                                                const int32_t *__restrict__ attr_cls,
                                                                const float *__restrict__ prop_boxes,
                                                                const int32_t *__restrict__ counts,
                                                                const float *__restrict__ scales_yx,
                                                                const float *__restrict__ feat, int F, int B, vk_outputs out) {
    const int b = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int cnt = counts[n];
    const bool valid = b < cnt;
    const long k = (long)n * B + b;
    if (tid == 0) {
        OutRow o;
        if (valid) {
            for (int c = 0; c < 4; ++c) o.box[c] = prop_boxes[k * 4 + c];
            o.obj_prob = obj_prob[k];
            o.obj_id = obj_cls[k];
            o.attr_prob = attr_prob[k];
            o.attr_id = attr_cls[k];
        }
        store_output_row(out, nullptr, k, valid, o, scales_yx, n);      // the scales multiply of the selection kernels
        if (b == 0) out.preds_per_image[n] = cnt;
    }
    const int F4 = F / 4;
    floatx4 *dst = reinterpret_cast<floatx4 *>(out.roi_features + k * F);
    if (valid) {
        const floatx4 *src = reinterpret_cast<const floatx4 *>(feat + k * F);
        for (int i = tid; i < F4; i += 128) dst[i] = src[i];
    } else {
        const floatx4 z = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < F4; i += 128) dst[i] = z;
    }
}

int launch_given_boxes_ingest(const float *boxes, const int32_t *counts, const int32_t *image_hw, const float *scales_yx, int N,
                              int B, float *prop_boxes, float *rois, int32_t *nonfinite, hipStream_t s) {
    VK_REQUIRE(N >= 1 && B >= 1 && B <= 1024, VK_EINVAL, "given_boxes_ingest: N=%d B=%d", N, B);
    const int total = N * B;
    hipLaunchKernelGGL(given_boxes_ingest_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, boxes, counts, image_hw, scales_yx, B,
                       total, prop_boxes, rois, nonfinite);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int launch_given_boxes_ingest_levels(const float *boxes, const int32_t *counts, const int32_t *image_hw, const float *scales_yx,
                                     int N, int B, float *prop_boxes, float *rois, int32_t *levels, int min_level, int max_level,
                                     float canonical_size, int canonical_level, int32_t *nonfinite, hipStream_t s) {
    VK_REQUIRE(N >= 1 && B >= 1 && B <= 1024, VK_EINVAL, "given_boxes_ingest: N=%d B=%d", N, B);
    VK_REQUIRE(min_level <= max_level, VK_EINVAL, "given_boxes_ingest: levels %d..%d", min_level, max_level);
    const int total = N * B;
    const LevelRule lr{levels, min_level, max_level, canonical_size, canonical_level};
    hipLaunchKernelGGL(given_boxes_ingest_levels_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, boxes, counts, image_hw,
                       scales_yx, B, total, prop_boxes, rois, nonfinite, lr);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int launch_given_box_outputs(const float *obj_prob, const int32_t *obj_cls, const float *attr_prob, const int32_t *attr_cls,
                             const float *prop_boxes, const int32_t *counts, const float *scales_yx, const float *feat, int F,
                             int N, int B, const vk_outputs &out, hipStream_t s) {
    VK_REQUIRE(N >= 1 && B >= 1 && B <= 1024, VK_EINVAL, "given_box_outputs: N=%d B=%d", N, B);
    VK_REQUIRE(F > 0 && F % 4 == 0, VK_EINVAL, "given_box_outputs: F=%d must be a multiple of 4", F);
    hipLaunchKernelGGL(given_box_outputs_kernel, dim3(B, N), dim3(128), 0, s, obj_prob, obj_cls, attr_prob, attr_cls, prop_boxes,
                       counts, scales_yx, feat, F, B, out);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk

// ---- the two ends as C entry points, for callers that compose the forward themselves (the FPN detector, frcnn_fpn.py) ----
extern "C" {

int vk_given_boxes_ingest(const float *boxes, const int32_t *counts, const int32_t *image_hw, const float *scales_yx, int N, int B,
                          float *prop_boxes, float *rois, int32_t *levels, int min_level, int max_level, float canonical_box_size,
                          int canonical_level, int32_t *nonfinite, void *stream) {
    VK_REQUIRE(boxes && counts && image_hw && prop_boxes && rois && nonfinite, VK_EINVAL, "given_boxes_ingest: null argument");
    VK_REQUIRE(N >= 1 && B >= 1 && B <= 1024, VK_EINVAL, "given_boxes_ingest: N=%d must be >= 1 and B=%d in 1..1024", N, B);
    if (!levels)
        return vk::launch_given_boxes_ingest(boxes, counts, image_hw, scales_yx, N, B, prop_boxes, rois, nonfinite, (hipStream_t)stream);
    VK_REQUIRE(min_level <= max_level, VK_EINVAL, "given_boxes_ingest: min_level=%d > max_level=%d", min_level, max_level);
    return vk::launch_given_boxes_ingest_levels(boxes, counts, image_hw, scales_yx, N, B, prop_boxes, rois, levels, min_level,
                                                max_level, canonical_box_size, canonical_level, nonfinite, (hipStream_t)stream);
}

int vk_given_box_outputs(const float *obj_prob, const int32_t *obj_cls, const float *attr_prob, const int32_t *attr_cls,
                         const float *prop_boxes, const int32_t *counts, const float *scales_yx, const float *feat, int F, int N,
                         int B, const vk_outputs *out, void *stream) {
    VK_REQUIRE(obj_prob && obj_cls && attr_prob && attr_cls && prop_boxes && counts && feat && out, VK_EINVAL,
               "given_box_outputs: null argument");
    VK_REQUIRE(out->obj_ids && out->obj_probs && out->attr_ids && out->attr_probs && out->boxes && out->preds_per_image &&
                   out->roi_features,
               VK_EINVAL, "given_box_outputs: null output array");
    VK_REQUIRE(N >= 1 && B >= 1 && B <= 1024, VK_EINVAL, "given_box_outputs: N=%d must be >= 1 and B=%d in 1..1024", N, B);
    VK_REQUIRE(F > 0 && F % 4 == 0, VK_EINVAL, "given_box_outputs: F=%d must be a positive multiple of 4", F);
    VK_REQUIRE((((uintptr_t)feat | (uintptr_t)out->roi_features) & 15) == 0, VK_EINVAL,
               "given_box_outputs: feat and roi_features must be 16-byte aligned");
    return vk::launch_given_box_outputs(obj_prob, obj_cls, attr_prob, attr_cls, prop_boxes, counts, scales_yx, feat, F, N, B, *out,
                                        (hipStream_t)stream);
}

}  // extern "C"
