// What the selection kernels of the box path share (rpn.hip, roi_out.hip, per_class.hip, detections.hip, given_boxes.hip;
// include after vk_common.h, inside .hip files only): the rank key, the LDS sort, the NMS pair test and the inner loop of the
// greedy sweep, the writer of a vk_outputs row, the feature-row copy, the LDS carve and the extents the launchers check.
// Only the Makefile's NOFMA objects include this header: all of them build with -ffp-contract=off, so the arithmetic below
// rounds every multiply and add on its own, as the reference does.  "The selection modes agree bit for bit on shared
// arithmetic" (DESIGN.md sections 15, 16, 18, 30) holds because every kernel runs the code below, not a restatement.
#pragma once
#include "conv_prims.h"

namespace vk {

// ---- the key ----
// Sort key of a score for an ascending sort that ranks scores descending (-0 ranks as +0).
__device__ __forceinline__ uint32_t desc_key32(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}
// The 64-bit rank key: the low word holds the row (or whatever names the entry), so ties go to the lower one (stable).
__device__ __forceinline__ unsigned long long pack_key(uint32_t key32, uint32_t low) { return ((unsigned long long)key32 << 32) | low; }
__device__ __forceinline__ unsigned long long score_key(float score, uint32_t low) { return pack_key(desc_key32(score), low); }
__device__ __forceinline__ uint32_t key_low(unsigned long long key) { return (uint32_t)(key & 0xFFFFFFFFull); }
constexpr unsigned long long KEY_BEHIND_ALL = ~0ull;      // pads a sort to its power of two: behind every real key

// ---- the sort ----
// Bitonic sort, ascending, of keys[0:n] in LDS by a workgroup of T threads (the kernel's __launch_bounds__); n a power of
// two.  The keys must be visible to the workgroup on entry; one barrier ends each pass, the last one included.
template <int T>
__device__ __forceinline__ void lds_sort_keys(unsigned long long *keys, int n) {
    const int tid = threadIdx.x;
    for (int k2 = 2; k2 <= n; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = tid; i < n; i += T) {
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
}

// ---- the NMS pair test ----
// torchvision's CPU nms (do_nms frcnn.py:116-143): areas without +1, IoU in fp32, compared as a double.
__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2) { return (x2 - x1) * (y2 - y1); }
// whether box i (ia its box_area) suppresses box j
__device__ __forceinline__ bool nms_suppresses(float ix1, float iy1, float ix2, float iy2, float ia, float jx1, float jy1, float jx2,
                                               float jy2, double thr) {
    const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
    const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = inter / (ia + box_area(jx1, jy1, jx2, jy2) - inter);
    return (double)ovr > thr;
}

// ---- the greedy sweep's inner loop ----
// Position i of the order, whose box is row ri of box[][4], is kept: mark every live position behind it that it suppresses.
// BY_KEY: position j's box is row key_low(keys[j]) (the boxes lie in row order); otherwise row j (the boxes lie in sorted
// order; keys is not read).  The caller's barrier comes before the next position looks at removed[].
template <int T, bool BY_KEY>
__device__ __forceinline__ void sweep_mark(const unsigned long long *keys, const float *box, int *removed, int i, int ri, int cnt,
                                           double thr) {
    const float ix1 = box[4 * ri], iy1 = box[4 * ri + 1], ix2 = box[4 * ri + 2], iy2 = box[4 * ri + 3];
    const float ia = box_area(ix1, iy1, ix2, iy2);
    for (int j = i + 1 + threadIdx.x; j < cnt; j += T) {
        if (removed[j]) continue;
        const int rj = BY_KEY ? (int)key_low(keys[j]) : j;
        if (nms_suppresses(ix1, iy1, ix2, iy2, ia, box[4 * rj], box[4 * rj + 1], box[4 * rj + 2], box[4 * rj + 3], thr)) removed[j] = 1;
    }
}

// ---- the outputs ----
// One row of a vk_outputs; as initialised here it is what a slot at or beyond preds_per_image holds.
struct OutRow {
    float box[4] = {0.f, 0.f, 0.f, 0.f}, obj_prob = 0.f, attr_prob = 0.f;
    int64_t obj_id = 0, attr_id = 0, keep_id = 0;
};
// Row `slot` of the outputs, a row of image n.  scales_yx [N][2] or null: applied to a selected row only.
__device__ __forceinline__ void store_output_row(const vk_outputs &out, int64_t *keep_ids, long slot, bool selected, OutRow r,
                                                 const float *scales_yx, int n) {
    if (selected && scales_yx) {   // boxes[:,0::2] *= scale_yx[1]; boxes[:,1::2] *= scale_yx[0]  (:1280-1283)
        const float sy = scales_yx[2 * n], sx = scales_yx[2 * n + 1];
        r.box[0] *= sx;
        r.box[2] *= sx;
        r.box[1] *= sy;
        r.box[3] *= sy;
    }
    out.boxes[slot * 4 + 0] = r.box[0];
    out.boxes[slot * 4 + 1] = r.box[1];
    out.boxes[slot * 4 + 2] = r.box[2];
    out.boxes[slot * 4 + 3] = r.box[3];
    out.obj_probs[slot] = r.obj_prob;
    out.obj_ids[slot] = r.obj_id;
    out.attr_probs[slot] = r.attr_prob;
    out.attr_ids[slot] = r.attr_id;
    if (keep_ids) keep_ids[slot] = r.keep_id;
}

// roi_features of one image, out [D][F] from feat [R][F]: slot d < nk takes row src(d), the slots behind it are zeroed.
// Row by row, 16 bytes per thread of the T.
template <int T, typename Src>
__device__ __forceinline__ void copy_feature_rows(const float *feat, float *out, int F, int D, int nk, Src src) {
    const int F4 = F / 4;
    for (int d = 0; d < D; ++d) {
        floatx4 *dst = reinterpret_cast<floatx4 *>(out + (long)d * F);
        if (d < nk) {
            const floatx4 *s = reinterpret_cast<const floatx4 *>(feat + (long)src(d) * F);
            for (int i = threadIdx.x; i < F4; i += T) dst[i] = s[i];
        } else {
            const floatx4 z = {0.f, 0.f, 0.f, 0.f};
            for (int i = threadIdx.x; i < F4; i += T) dst[i] = z;
        }
    }
}

// ---- the LDS of a sort-and-sweep kernel ----
// keys[Rp2] u64 | box[R][4] f32 | removed[R] i32 | extra[n_extra] 4-byte words (roi_final_kernel: kept[D];
// per_class_nms_kernel: score bits[R]; det_nms_kernel: none).  The kernel takes its pointers and the launcher its byte count
// from the same offsets.  The base is the one dynamic array, 16-byte aligned.
struct SelectLds {
    unsigned long long *keys;
    float *box;
    int *removed;
    int *extra;
    static __host__ __device__ size_t box_at(int Rp2) { return (size_t)Rp2 * 8; }
    static __host__ __device__ size_t removed_at(int Rp2, int R) { return box_at(Rp2) + (size_t)R * 16; }
    static __host__ __device__ size_t extra_at(int Rp2, int R) { return removed_at(Rp2, R) + (size_t)R * 4; }
    static size_t bytes(int Rp2, int R, int n_extra) { return extra_at(Rp2, R) + (size_t)n_extra * 4; }
    __device__ SelectLds(char *base, int Rp2, int R)
        : keys(reinterpret_cast<unsigned long long *>(base)), box(reinterpret_cast<float *>(base + box_at(Rp2))),
          removed(reinterpret_cast<int *>(base + removed_at(Rp2, R))), extra(reinterpret_cast<int *>(base + extra_at(Rp2, R))) {}
};

// ---- one wavefront per (class, image) ----
constexpr int SELECT_XCDS = 8;      // accelerator dies of an MI355X; only the order of the classes depends on it, no result does
// blockIdx.x -> class, so that the workgroups one XCD receives (consecutive workgroup ids go round the XCDs) hold a
// contiguous run of classes: the classes that share a cache line of the strided score and delta columns then meet in one
// XCD's L2 instead of each XCD fetching the line for itself.  gridDim.x is select_class_grid(C); classes >= C do not exist.
__device__ __forceinline__ int select_class() {
    return (int)(blockIdx.x % SELECT_XCDS) * (int)(gridDim.x / SELECT_XCDS) + (int)(blockIdx.x / SELECT_XCDS);
}
static inline int select_class_grid(int C) { return ceil_div(C, SELECT_XCDS) * SELECT_XCDS; }

// ---- the extents the three launchers hold R and max_detections to (d_max, named d_max_name in the message) ----
static inline int check_select_shape(const char *who, int R, int D, int d_max, const char *d_max_name) {
    VK_REQUIRE(R >= 1 && R <= 1024, VK_EINVAL, "%s: R=%d must be in 1..1024", who, R);
    VK_REQUIRE(D >= 1 && D <= d_max, VK_EINVAL, "%s: max_detections=%d must be in 1..%s", who, D, d_max_name);
    return VK_OK;
}

}  // namespace vk
