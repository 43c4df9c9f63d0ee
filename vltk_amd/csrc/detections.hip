// Detector-style selection on gfx950 (roi_outputs.selection = "detections"): the rule of detectron2's
// fast_rcnn_inference_single_image -- every (proposal, class) pair whose score is above score_thresh is a candidate, NMS
// runs per class, the best max_detections (box, class, score) triples of the image are the output.  A proposal may come out
// under several classes and an image may yield nothing.
//
// The rule is detectron2's; every piece of arithmetic inside it is the reference's own, shared with per_class.hip:
// the scores are class_probs_kernel's, a (row, class) box is pc_box's (vk_common.h), the sweep is per_class_nms_kernel's
// (scores descending, ties to the lower row; areas without +1; suppressed iff (double)(inter / (a_i + a_j - inter)) > thresh).
//
// Threshold first.  Three kernels:
//   det_compact_kernel  one pass along the rows of the scores [K, ld] and the deltas [K, 4C]: decodes and finite-checks every
//                       (row, class) box and appends the rows with (double)score > score_thresh to the list of their
//                       (image, class).  The order within a list depends on scheduling; nothing after it does: every
//                       consumer sorts by a key that holds the row.
//   det_nms_kernel      one wavefront per (image, class): reads the list's length and returns when it is zero; otherwise
//                       sorts and sweeps the candidates alone (equal to NMS over all rows followed by the threshold: a box
//                       can only be suppressed by a box ranked before it, whose score is at least as high).  The survivors'
//                       keys (desc_key32(score) << 32) | (row << 20 | class) are appended to the image's list.
//   det_final_kernel    one workgroup per image: the n_out = min(#survivors, max_detections) smallest keys -- the keys are
//                       unique within an image, so there is no tie at the cut -- by a bitonic sort in LDS while the survivors
//                       fit (VK_DETECTIONS_LDS_KEYS), by a radix select over the global list when they do not; then the
//                       gather of per_class_final_kernel.
// Every output is a pure function of the inputs: the two lists are only ever read as sets.
//
// fp32 box math, reference op order, no FMA contraction (-ffp-contract=off for this file).
#include <cfloat>

#include "vk_common.h"
#include "conv_prims.h"

namespace vk {

constexpr int DET_XCDS = 8;                        // as PC_XCDS (per_class.hip): orders the classes, changes no result
constexpr int DET_LDS_KEYS = VK_DETECTIONS_LDS_KEYS;
constexpr int DET_FINAL_THREADS = 1024;
static_assert(DET_LDS_KEYS >= 1024 && (DET_LDS_KEYS & (DET_LDS_KEYS - 1)) == 0, "holds max_detections keys, a power of two");

// Thread i of image blockIdx.y: (row, class) = (i / C, i % C) over the image's own rows, so a wavefront walks along a row
// of the scores and of the deltas.
__global__ __launch_bounds__(256) void det_compact_kernel(DetArgs d) {
    const PerClassArgs &a = d.pc;
    const int n = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int cnt = max(0, min(a.counts[n], a.R));
    bool bad = false;
    if (i < (long)cnt * a.C) {
        const int r = (int)(i / a.C), c = (int)(i % a.C);
        const long row = (long)n * a.R + r;
        const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
        float b[4];
        bad = !pc_box(a, row, c, img_w, img_h, b);
        const float sc = a.scores[row * a.ld_scores + c];
        if ((double)sc > a.score_thresh) {                     // strict; false for NaN
            const long pair = (long)n * a.C + c;
            const int slot = atomicAdd(d.cand_cnt + pair, 1);
            if (slot < a.R) d.cand[pair * a.R + slot] = (uint16_t)r;      // a pair has at most one candidate per row
        }
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(a.nonfinite, 1);
}

// One wavefront per (class, image), classes laid over the XCDs as in per_class_nms_kernel.
// LDS: keys[Rp2] u64 | box[R][4] f32 (in sorted order) | removed[R] i32.
__global__ __launch_bounds__(64) void det_nms_kernel(DetArgs d, int Rp2) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const PerClassArgs &a = d.pc;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem_raw);
    float *sbox = reinterpret_cast<float *>(keys + Rp2);
    int *removed = reinterpret_cast<int *>(sbox + (size_t)a.R * 4);

    const int n = blockIdx.y, lane = threadIdx.x;
    const int c = (int)(blockIdx.x % DET_XCDS) * (int)(gridDim.x / DET_XCDS) + (int)(blockIdx.x / DET_XCDS);
    if (c >= a.C) return;                          // grid.x is C rounded up to a multiple of DET_XCDS
    const long pair = (long)n * a.C + c;
    const int m = min(d.cand_cnt[pair], a.R);
    if (m <= 0) return;                            // nothing of this class can be reported
    int np2 = 2;
    while (np2 < m) np2 <<= 1;
    const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
    const long k0 = (long)n * a.R;
    const uint16_t *list = d.cand + pair * a.R;

    for (int i = lane; i < np2; i += 64) {
        if (i < m) {
            const int r = list[i];
            const float sc = a.scores[(k0 + r) * a.ld_scores + c];
            keys[i] = ((unsigned long long)desc_key32(sc) << 32) | (uint32_t)r;
        } else {
            keys[i] = ~0ull;
        }
    }
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

    for (int i = lane; i < m; i += 64) {           // position i of the order holds its own box
        float b[4];
        pc_box(a, k0 + (int)(keys[i] & 0xFFFFFFFFull), c, img_w, img_h, b);      // finite: the compaction pass checked it
        sbox[4 * i + 0] = b[0];
        sbox[4 * i + 1] = b[1];
        sbox[4 * i + 2] = b[2];
        sbox[4 * i + 3] = b[3];
        removed[i] = 0;
    }

    const double thr = a.thresh;
    for (int i = 0; i < m; ++i) {
        __syncthreads();
        if (removed[i]) continue;
        const float ix1 = sbox[4 * i], iy1 = sbox[4 * i + 1], ix2 = sbox[4 * i + 2], iy2 = sbox[4 * i + 3];
        const float ia = (ix2 - ix1) * (iy2 - iy1);
        for (int j = i + 1 + lane; j < m; j += 64) {
            if (removed[j]) continue;
            const float jx1 = sbox[4 * j], jy1 = sbox[4 * j + 1], jx2 = sbox[4 * j + 2], jy2 = sbox[4 * j + 3];
            const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
            const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
            const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
            const float inter = w * h;
            const float ja = (jx2 - jx1) * (jy2 - jy1);
            const float ovr = inter / (ia + ja - inter);
            if ((double)ovr > thr) removed[j] = 1;
        }
    }
    __syncthreads();

    // the survivors of the pair, recorded as keys in the image's list: one reservation for the class
    int mine = 0;
    for (int i = lane; i < m; i += 64) mine += removed[i] ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (mine == 0) return;                         // (cannot happen: the best candidate always survives)
    int base = 0;
    if (lane == 0) base = atomicAdd(d.surv_cnt + n, mine);
    base = __shfl(base, 0);
    const long RC = (long)a.R * a.C;
    unsigned long long *out = d.surv + (long)n * RC;
    int off = 0;
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        const bool alive = i < m && !removed[i];
        const unsigned long long mask = __ballot(alive);
        const int pre = __popcll(mask & ((1ull << lane) - 1ull));
        const long at = (long)base + off + pre;
        if (alive && at < RC) {
            const unsigned long long k = keys[i];
            out[at] = (k & 0xFFFFFFFF00000000ull) | ((k & 0xFFFFFFFFull) << 20) | (unsigned long long)c;
        }
        off += __popcll(mask);
    }
}

// One workgroup per image.  LDS: keys[DET_LDS_KEYS] u64, the radix histogram, three words.
__global__ __launch_bounds__(DET_FINAL_THREADS) void det_final_kernel(DetArgs d) {
    __shared__ unsigned long long keys[DET_LDS_KEYS];
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_want, s_n;
    const PerClassArgs &a = d.pc;

    const int n = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const long RC = (long)a.R * a.C;
    const long m = min((long)max(d.surv_cnt[n], 0), RC);
    int nk = (int)min(m, (long)a.D);
    const unsigned long long *list = d.surv + (long)n * RC;
    const float img_h = (float)a.image_hw[2 * n], img_w = (float)a.image_hw[2 * n + 1];
    const long k0 = (long)n * a.R;

    int ns;                                        // keys in LDS, to be sorted
    if (m <= DET_LDS_KEYS) {
        ns = (int)m;
        for (int i = tid; i < ns; i += T) keys[i] = list[i];
    } else {
        // radix select, most significant byte first: after the last pass `prefix` is the nk-th smallest key itself
        unsigned long long prefix = 0ull;
        int want = nk;                             // rank, from 1, among the keys that share the prefix
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += T) hist[i] = 0u;
            __syncthreads();
            const unsigned long long above = shift == 56 ? 0ull : ~0ull << (shift + 8);
            for (long i = tid; i < m; i += T) {
                const unsigned long long k = list[i];
                if ((k & above) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, b = 0;
                for (; b < 255; ++b) {
                    if (acc + (int)hist[b] >= want) break;
                    acc += (int)hist[b];
                }
                s_prefix = prefix | ((unsigned long long)b << shift);
                s_want = want - acc;
            }
            __syncthreads();
            prefix = s_prefix;
            want = s_want;
        }
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (long i = tid; i < m; i += T) {
            const unsigned long long k = list[i];
            if (k <= prefix) {
                const int at = atomicAdd(&s_n, 1);             // any order: sorted below
                if (at < DET_LDS_KEYS) keys[at] = k;
            }
        }
        __syncthreads();
        ns = min(s_n, DET_LDS_KEYS);               // == nk: the keys are unique
    }
    nk = min(nk, ns);                              // (no change: both paths hold at least nk keys)
    int np2 = 2;
    while (np2 < ns) np2 <<= 1;
    for (int i = ns + tid; i < np2; i += T) keys[i] = ~0ull;
    __syncthreads();

    for (int k2 = 2; k2 <= np2; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = tid; i < np2; i += T) {
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

    const float sy = a.scales_yx ? a.scales_yx[2 * n] : 1.f, sx = a.scales_yx ? a.scales_yx[2 * n + 1] : 1.f;
    const long o0 = (long)n * a.D;
    for (int dd = tid; dd < a.D; dd += T) {
        float b[4] = {0.f, 0.f, 0.f, 0.f}, op = 0.f, ap = 0.f;
        int64_t oc = 0, ac = 0, kid = 0;
        if (dd < nk) {
            const uint32_t low = (uint32_t)(keys[dd] & 0xFFFFFFFFull);
            const int r = (int)(low >> 20), cls = (int)(low & 0xFFFFFu);
            pc_box(a, k0 + r, cls, img_w, img_h, b);            // the bits the NMS kernel held for (r, cls)
            if (a.scales_yx) {   // boxes[:,0::2] *= scale_yx[1]; boxes[:,1::2] *= scale_yx[0]  (:1280-1283)
                b[0] *= sx;
                b[2] *= sx;
                b[1] *= sy;
                b[3] *= sy;
            }
            op = a.scores[(k0 + r) * a.ld_scores + cls];
            oc = cls;
            ap = a.attr_prob ? a.attr_prob[k0 + r] : 0.f;
            ac = a.attr_cls ? a.attr_cls[k0 + r] : 0;
            kid = r;
        }
        a.out.boxes[(o0 + dd) * 4 + 0] = b[0];
        a.out.boxes[(o0 + dd) * 4 + 1] = b[1];
        a.out.boxes[(o0 + dd) * 4 + 2] = b[2];
        a.out.boxes[(o0 + dd) * 4 + 3] = b[3];
        a.out.obj_probs[o0 + dd] = op;
        a.out.obj_ids[o0 + dd] = oc;
        a.out.attr_probs[o0 + dd] = ap;
        a.out.attr_ids[o0 + dd] = ac;
        if (a.keep_ids) a.keep_ids[o0 + dd] = kid;
    }
    if (tid == 0) {
        a.out.preds_per_image[n] = nk;
        if (d.n_survivors) d.n_survivors[n] = (int32_t)m;
    }
    const int F4 = a.F / 4;
    for (long j = tid; j < (long)a.D * F4; j += T) {
        const int dd = (int)(j / F4), i = (int)(j % F4);
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (dd < nk) {
            const int r = (int)((uint32_t)(keys[dd] & 0xFFFFFFFFull) >> 20);
            v = reinterpret_cast<const floatx4 *>(a.features + (k0 + r) * a.F)[i];
        }
        reinterpret_cast<floatx4 *>(a.out.roi_features + (o0 + dd) * a.F)[i] = v;
    }
}

static size_t det_cnt_bytes(int N, int C) { return align_up(sizeof(int32_t) * ((size_t)N * C + N), 256); }
static size_t det_cand_bytes(int N, int R, int C) { return align_up(sizeof(uint16_t) * (size_t)N * C * R, 256); }

size_t det_workspace_bytes(int N, int R, int C) {
    return det_cnt_bytes(N, C) + det_cand_bytes(N, R, C) + align_up(sizeof(unsigned long long) * (size_t)N * R * C, 256);
}

void det_carve(DetArgs &d, char *base, int N, int R, int C) {
    d.cand_cnt = reinterpret_cast<int32_t *>(base);
    d.surv_cnt = d.cand_cnt + (size_t)N * C;
    d.cand = reinterpret_cast<uint16_t *>(base + det_cnt_bytes(N, C));
    d.surv = reinterpret_cast<unsigned long long *>(base + det_cnt_bytes(N, C) + det_cand_bytes(N, R, C));
}

// the two counters are zeroed here; pc.nonfinite is the caller's to zero (it may already hold an earlier stage's flag)
int launch_detections_select(DetArgs &d, int N, hipStream_t s) {
    const PerClassArgs &a = d.pc;
    VK_REQUIRE(N >= 1 && N <= 65535, VK_EINVAL, "detections: N=%d must be in 1..65535", N);
    VK_REQUIRE(a.R >= 1 && a.R <= 1024, VK_EINVAL, "detections: R=%d must be in 1..1024", a.R);
    VK_REQUIRE(a.D >= 1 && a.D <= 1024, VK_EINVAL, "detections: max_detections=%d must be in 1..1024", a.D);
    VK_REQUIRE(a.C >= 1 && a.C < (1 << 20), VK_EINVAL, "detections: C=%d must be in 1..2^20-1", a.C);
    VK_REQUIRE(a.F >= 4 && a.F % 4 == 0, VK_EINVAL, "detections: F must be a positive multiple of 4");
    VK_REQUIRE(a.ld_scores >= a.C && a.ld_box >= (a.agnostic ? 4 : 4 * a.C), VK_EINVAL, "detections: row strides ld_scores=%d ld_box=%d "
               "are shorter than the rows", a.ld_scores, a.ld_box);
    VK_REQUIRE(d.cand_cnt && d.surv_cnt && d.cand && d.surv && a.nonfinite, VK_EINVAL, "detections: null workspace");
    int Rp2 = 2;
    while (Rp2 < a.R) Rp2 <<= 1;
    VK_CHECK_HIP(hipMemsetAsync(d.cand_cnt, 0, sizeof(int32_t) * ((size_t)N * a.C + N), s));
    const long RC = (long)a.R * a.C;
    hipLaunchKernelGGL(det_compact_kernel, dim3((unsigned)((RC + 255) / 256), N), dim3(256), 0, s, d);
    VK_CHECK_HIP(hipGetLastError());
    const size_t smem_nms = (size_t)Rp2 * 8 + (size_t)a.R * 16 + (size_t)a.R * 4;
    hipLaunchKernelGGL(det_nms_kernel, dim3(ceil_div(a.C, DET_XCDS) * DET_XCDS, N), dim3(64), smem_nms, s, d, Rp2);
    VK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(det_final_kernel, dim3(N), dim3(DET_FINAL_THREADS), 0, s, d);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // namespace vk
