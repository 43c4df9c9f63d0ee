// Internal helpers shared by the translation units of libvltk_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vltk_hip.h"

namespace vk {

void set_error(const char *fmt, ...);

#define VK_CHECK_HIP(expr)                                                                    \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            vk::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return VK_EHIP;                                                                   \
        }                                                                                     \
    } while (0)

#define VK_REQUIRE(cond, code, ...)       \
    do {                                  \
        if (!(cond)) {                    \
            vk::set_error(__VA_ARGS__);   \
            return (code);                \
        }                                 \
    } while (0)

#define VK_TRY(expr)              \
    do {                          \
        int _s = (expr);          \
        if (_s != VK_OK) return _s; \
    } while (0)

// CALL with T = float, _Float16 or __bf16 as dt says; any other dt is refused in the entry's name (`who`, a string literal).
#define VK_DT_SWITCH(dt, who, CALL)                                                     \
    switch (dt) {                                                                       \
        case VK_F32: { typedef float T; CALL; } break;                                  \
        case VK_F16: { typedef _Float16 T; CALL; } break;                               \
        case VK_BF16: { typedef __bf16 T; CALL; } break;                                \
        default: VK_REQUIRE(false, VK_EINVAL, who ": dtype must be f32, f16 or bf16");  \
    }

static inline size_t dtype_size(vk_dtype dt) {
    switch (dt) {
        case VK_F32: return 4;
        case VK_F16: return 2;
        case VK_I64: return 8;
        case VK_I32: return 4;
        case VK_BF16: return 2;
    }
    return 0;
}

constexpr int VK_MAX_DEVICES = 64;      // slots of per-device launcher state (DeviceState)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// the extent of a bitonic sort over v keys: the power of two at or above v, at least 2
__host__ __device__ static inline int next_pow2(int v) {
    int p = 2;
    while (p < v) p <<= 1;
    return p;
}

// ---- what the launchers of vk_gemm_f32 (train.hip) and vk_gemm_16 (gemm16.hip) share ----
// The shape and leading-dimension rules of C [M, N] = op(A) . op(B), refused in the entry's name (`who`: "gemm_f32", "gemm_16").
static inline int gemm_shape_check(const char *who, int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB) {
    VK_REQUIRE(M >= 1 && N >= 1 && K >= 1, VK_EINVAL, "%s: sizes must be positive, got M=%d N=%d K=%d", who, M, N, K);
    VK_REQUIRE((transA == 0 || transA == 1) && (transB == 0 || transB == 1), VK_EINVAL, "%s: transA=%d transB=%d must be 0 or 1", who, transA,
               transB);
    VK_REQUIRE(lda >= (transA ? M : K), VK_EINVAL, "%s: lda=%ld is below A's row width %d", who, lda, transA ? M : K);
    VK_REQUIRE(ldb >= (transB ? K : N), VK_EINVAL, "%s: ldb=%ld is below B's row width %d", who, ldb, transB ? K : N);
    VK_REQUIRE(ldc >= N, VK_EINVAL, "%s: ldc=%ld is below C's row width %d", who, ldc, N);
    return VK_OK;
}
// The tile of both: 128 x 128 where such tiles fill half the CUs, 64 x 64 elsewhere.
static inline bool large_tile(int M, int N, int n_cu) { return (long)ceil_div(M, 128) * ceil_div(N, 128) * 2 >= n_cu; }

// ---- convolution as implicit GEMM (conv_mfma.hip) --------------------------
constexpr int CONV_BM = 128;        // output pixels per workgroup tile
constexpr int CONV_KTILE_BYTES = 128;  // bytes of K per row per K-tile (64 f16 / 32 f32)
constexpr int CONV_COUT_ALIGN = 128;   // packed weight rows are padded to this

struct ConvArgs {
    const void *x;       // NHWC input (or the padded NHWC4 image in stem mode)
    const void *w;       // packed weights [cout_pad][ktiles * KTILE_BYTES]
    const float *bias;   // [cout_pad]
    const void *res;     // residual [M, ldy] or nullptr
    void *y;             // output [M, ldy]
    int N, H, W, Cin;    // input geometry (stem mode: padded Hp, Wp, 4)
    int Ho, Wo, Cout, ldy;
    int kh, kw, stride, pad, dil;
    int groups;          // 0 / 1: dense; > 1: slice-diagonal weights (vk_pack_conv_weight), Cin == Cout
    int concurrent;      // launched beside another stream's kernels (timing bucket 6)
    float *pool_part;    // fused spatial mean (Res5 `.mean(dim=[2,3])`): per-tile column sums go here, y is not written
    const void *x2;      // dual-source 1x1 (conv3 + projection shortcut in one GEMM): second input [M, Cin2], K = Cin | Cin2
    int Cin2;
    int relu;
    int stem;            // 1: K-tiles are runs of consecutive input pixels (7x7 s2 stem)
    const int32_t *m_dev;   // conv_gemm4 only: the row count M is read on the device (N * Ho * Wo bounds it and sizes the grid)
    const int32_t *x2_idx;  // conv_gemm4 only: output row m reads row x2_idx[m] of x2
    const int32_t *x_idx;   // conv3x3_panel only, where conv3x3_panel_phase_indexed: output row m reads row x_idx[m] of x [x_rows, Cin]
    long x_rows;            // with x_idx: the rows of x (every index lies in [0, x_rows))
    const int32_t *y_idx;   // conv3x3_panel only, where conv3x3_panel_out_indexed: output row m goes to row y_idx[m] of y [y_rows, ldy], nowhere if that is outside [0, y_rows); no residual
    long y_rows;            // with y_idx: the rows of y
    const int32_t *res_idx; // conv_ws only, where conv_ws_res_indexed: output row m adds row res_idx[m] of res
    vk_dtype dt, out_dt;
};
int launch_conv(const ConvArgs &a, hipStream_t stream);
int conv_route(const ConvArgs &a);            // the VK_ROUTE_* launch_conv switches on (host only); -VK_EINVAL: no kernel takes the form
int conv_route_checked(const ConvArgs &a);    // the same, and -VK_E* where the generic kernel refuses the layer (vk_conv_route)
bool conv256_eligible(const ConvArgs &a);                 // conv_mfma256.hip
int launch_conv256(const ConvArgs &a, hipStream_t stream);
bool conv3x3_panel_eligible(const ConvArgs &a);           // conv3x3_panel.hip (LDS-resident input panel, 9 taps per fetch)
int launch_conv3x3_panel(const ConvArgs &a, hipStream_t stream);
int conv3x3_panel_phase_images(const ConvArgs &a);        // leading images of a panel launch that take its phase-interleaved form
int conv3x3_panel_phase_tile_rows(const ConvArgs &a);     // rows of a tile of that part: 512, 256 (VK_PANEL_TALL=0) or 0 (no phase part)
int conv3x3_panel_phase_reuse(const ConvArgs &a);         // 1: that part's 512-row tiles share a fragment window per tap row; 0: VK_PANEL_REUSE=0 or no such tile
int conv3x3_panel_phase_indexed(const ConvArgs &a);       // 1: the WHOLE launch runs that form, which takes x_idx; 0: it does not (N % 16, the three switches) or VK_PANEL_INDEXED=0
int conv3x3_panel_out_indexed(const ConvArgs &a);         // 1: the WHOLE launch runs that form, which takes y_idx; 0: it does not, or VK_PANEL_OUT_INDEXED=0
bool conv_gemm4_eligible(const ConvArgs &a);              // conv_gemm4.hip (1x1, K >= 1024, one or two inputs: 256x256 tile, four waves of 128x128)
int launch_conv_gemm4(const ConvArgs &a, hipStream_t stream);
int acquire_tile_counter(unsigned **ctr);     // a zeroed device word for one launch's dynamic tile tail; its last fetch zeroes it again (conv_gemm4.hip)
bool conv256_dual_ok(const ConvArgs &a);                  // conv_mfma256.hip (dual-source 1x1 with a long K: 256x256 tile)
bool conv_duo_eligible(const ConvArgs &a);                // conv_mfma_duo.hip (1x1 convs: 128x256 tile, two workgroups per CU)
int launch_conv_duo(const ConvArgs &a, hipStream_t stream);
bool conv_ws_eligible(const ConvArgs &a);                 // conv_ws.hip (1x1, K <= 512: weight-stationary, weights in registers)
int launch_conv_ws(const ConvArgs &a, hipStream_t stream);
bool conv_ws_res_indexed(const ConvArgs &a);              // the layer runs on conv_ws's build that reads ConvArgs::res_idx
bool conv3x3_blk_eligible(const ConvArgs &a);             // conv3x3_blk.hip (narrow channel blocks: ResNeXt grouped 3x3, dense 64 -> 64)
int launch_conv3x3_blk(const ConvArgs &a, hipStream_t stream);
// bneck_fused.hip: a whole res2 BottleneckBlock (64 bottleneck channels, stride 1) as one kernel
bool bneck_fused_eligible(int cin, int cmid, int cout, int stride, int groups, bool proj, long N, int H, int W, vk_dtype dt);
bool bneck_fused_forced();      // VK_BNECK_FUSED set at all, even to "0": a direct launch goes ahead where the route is switched off (comparison tests)
int launch_bneck_fused(const void *x, int N, int H, int W, int cin, bool proj, const void *w1, const float *b1, const void *w2,
                       const float *b2, const void *w3, const float *b3, void *y, bool concurrent, hipStream_t stream);
bool conv_duo_dual_ok(const ConvArgs &a);
bool conv_duo_pool_ok(const ConvArgs &a);                 // fused-mean form (pool_part set)
size_t conv_duo_pool_part_bytes(long M, int Cout);
bool conv_pool_sums_f64(long N, int HW, int Cin, int Cout, bool dual);   // which form the fused mean's workspace holds (conv_ws.hip)
bool conv_ws_pool_ok(const ConvArgs &a);
int launch_pool_finish(const float *part, int N, int HoWo, int Cin, int Cout, bool dual, float *out, hipStream_t stream);

// optional per-launch event timing (set by vk_forward when enabled; thread-local)
struct KernelTimer {
    struct Rec {
        int bucket;
        double flops;
        hipEvent_t e0, e1;
        int M, cout, cin, k, stride;
        double bytes;
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;   // free events
    std::vector<hipEvent_t> all;    // every event ever created (destroyed with the timer)
    int64_t launches[VK_NUM_KERNEL_BUCKETS] = {};
    double ms[VK_NUM_KERNEL_BUCKETS] = {};
    double flops[VK_NUM_KERNEL_BUCKETS] = {};
    double bytes[VK_NUM_KERNEL_BUCKETS] = {};   // algorithmic: input + output (+ residual) + weights, once each
    hipEvent_t get();
    void collect();   // accumulates every launch whose end event has completed; the rest stay pending
    ~KernelTimer();
};
extern thread_local KernelTimer *g_timer;

// One timed launch: begin() before it, end() after it with the launch's timer bucket and algorithmic counts.  Both do nothing
// when g_timer is null.
struct Timed {
    KernelTimer *tm = g_timer;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int begin(hipStream_t stream);
    int end(hipStream_t stream, int bucket, double flops, int M, int cout, int cin, int k, int stride, double bytes);
};

// ---- launcher state, per device (runtime.hip) ----
// A process may hold handles on several devices: everything a launcher keeps between launches lives here, one record per
// device, created on the first launch on that device (under a lock) and kept for the life of the process.
constexpr int BN_TRASH_BYTES = 1 << 16;
struct DeviceState {
    int n_cu;                         // hipDeviceProp_t::multiProcessorCount, as reported (launchers do their own rounding)
    const char *zero_page;            // 256 zero bytes, never written (conv3x3_blk, conv_mfma256)
    char *bn_trash;                   // BN_TRASH_BYTES of write-only scratch (bneck_fused stores into it)
    unsigned *tile_ring;              // 256 words, zeroed once (acquire_tile_counter)
    std::atomic<unsigned> tile_next;  // the ring's cursor
};
int device_state(DeviceState **out);  // the current HIP device's record
// hipFuncAttributeMaxDynamicSharedMemorySize, once per (device, kernel); later calls are a lookup
int set_max_lds(const void *kernel, size_t bytes);
template <typename... A>
static inline int set_max_lds(void (*kernel)(A...), size_t bytes) { return set_max_lds(reinterpret_cast<const void *>(kernel), bytes); }
// One launch of a kernel that needs more LDS than the default limit: the limit goes to lds_cap (>= smem; a build-wide maximum
// where several launches of one instantiation differ in smem), then the launch and its error check.
template <typename... P, typename... A>
static inline int launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t smem, size_t lds_cap, hipStream_t s, A &&...args) {
    VK_TRY(set_max_lds(kernel, lds_cap));
    hipLaunchKernelGGL(kernel, grid, block, smem, s, static_cast<A &&>(args)...);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

// ---- the environment (runtime.hip: the one translation unit that calls getenv; the switches are listed in DESIGN.md) ----
const char *env_text(const char *name);      // the text, nullptr when unset
bool env_set(const char *name);              // set at all, even to ""
char env_first(const char *name);            // first character; '\0' when unset or empty
bool env_off(const char *name);              // env_first(name) == '0'
int env_int(const char *name, int dflt);     // atoi of the text when set, else dflt

#ifdef VK_ABLATION
// One stamped launch (tools/*_stamps.py): open() before the launch of a stamp instantiation, finish() after it.
struct Stamps {
    unsigned long *dev = nullptr;
    size_t words = 0;
    int open(size_t words, hipStream_t stream);      // `words` 64-bit stamps, zeroed on the stream
    // waits for the stream, frees the stamps and appends to `path`: the header line, then per row the first `cols` of its
    // `stride` words, after the row index (per_wg == 0) or after row / per_wg and row % per_wg
    int finish(hipStream_t stream, const char *path, const char *header, size_t rows, int stride, int cols, int per_wg);
};
#endif

// ---- pack.hip (host only) ----
void to_dt(const float *src, size_t n, vk_dtype dt, void *dst);       // float -> f16 / bf16 (nearest even) / f32

// ---- stage_api.hip: the builders of a launch's arguments, shared by the stage-level entry points and the model (model.hip) ----
static inline void conv_out_hw(int H, int W, int k, int s, int p, int d, int *Ho, int *Wo) {
    *Ho = (H + 2 * p - (d * (k - 1) + 1)) / s + 1;
    *Wo = (W + 2 * p - (d * (k - 1) + 1)) / s + 1;
}
// the layer as the dispatcher sees it; the pointers (and Cin2 with x2) are the caller's to set
void fill_conv_args(ConvArgs &a, int N, int H, int W, int cin, int cout, int ldy, int k, int stride, int pad, int dil, int groups,
                    int relu, vk_dtype dt, vk_dtype out_dt);
// stem_pack, then stem_pool or the 7x7 conv + max-pool (vk_stem, and the model's backbone)
int stem_impl(const float *x, int N, int H, int W, const void *w, const float *b, int cout, int caffe, void *y, vk_dtype dt,
              void *img_pad, void *stem_out, hipStream_t s, int32_t *nonfinite = nullptr);
struct PerClassArgs;
struct RoiFinalArgs;
void fill_per_class_args(PerClassArgs &a, const float *scores, int ld_scores, const float *deltas, int ld_box, int agnostic,
                         const float *proposals, const int32_t *counts, const float *features, const float *attr_prob,
                         const int32_t *attr_cls, int F, int R, int C, const int32_t *image_hw, const float *scales_yx,
                         const float *weights4, const vk_select_params *sp, const vk_outputs *out, int64_t *keep_ids,
                         int32_t *nonfinite);
void fill_roi_final_args(RoiFinalArgs &a, const float *obj_prob, const int32_t *obj_cls, const float *attr_prob,
                         const int32_t *attr_cls, const float *box_deltas, int ld_box, int delta_mode, const float *proposals,
                         const int32_t *counts, const float *features, int F, int R, const int32_t *image_hw,
                         const float *scales_yx, const float *weights4, const vk_roi_params *rp, const vk_outputs *out,
                         int64_t *keep_ids, int32_t *nonfinite);
// what a vk_select_params must satisfy in the per-class / detections mode; `who` prefixes the error text
int check_select_params(const vk_select_params *sp, const char *who);
int check_detections_params(const vk_select_params *sp, const char *who);

// ---- pool.hip ----
int launch_stem_pack(const float *x, void *y, int N, int H, int W, int Hp, int Wp, vk_dtype dt, hipStream_t s, int32_t *nonfinite = nullptr);
int launch_maxpool(const void *x, void *y, int N, int H, int W, int C, int caffe, vk_dtype dt, hipStream_t s);
bool stem_pool_eligible(int cout, vk_dtype dt);           // stem_pool.hip: 7x7 conv + BN + ReLU + max-pool as one kernel (f16, 64 channels)
int launch_stem_pool(const void *x, int N, int Hp, int Wp, int H1, int W1, const void *w, const float *bias, int caffe, void *y,
                     hipStream_t stream);

// ---- roi_out.hip ----
struct RoiFinalArgs {
    const float *obj_prob;
    const int32_t *obj_cls;
    const float *attr_prob;
    const int32_t *attr_cls;
    const float *box_deltas;
    int ld_box;
    int delta_mode;   // 0: full [K,4C] (index cls*4), 1: already the chosen/agnostic 4 deltas
    const float *proposals;
    const int32_t *counts;
    const float *features;
    int F, R, D;
    const int32_t *image_hw;
    const float *scales_yx;
    float wx, wy, ww, wh, clampv;
    int n_thresh;
    double thresh[VK_MAX_NMS_THRESH];
    int mind, maxd;
    vk_outputs out;
    int64_t *keep_ids;
    int32_t *nonfinite;
};
int launch_softmax_argmax(const float *logits, int ld, int K, int n_soft, int n_max, float *prob, int32_t *cls,
                          int32_t *raw_argmax, hipStream_t s);
int launch_concat_embed(const float *feat, const void *emb, const int32_t *cls, int F, int E, int K, void *out,
                        vk_dtype dt, hipStream_t s);
int launch_chosen_deltas(const void *x, int ldx, const void *w, const float *bias, const int32_t *cls, int agnostic, int F,
                         int K, float *out, vk_dtype dt, hipStream_t s);
int launch_roi_final(RoiFinalArgs &a, int N, hipStream_t s);
int launch_make_rois(const float *boxes, int N, int R, float *rois, hipStream_t s);

// One element of any storage type as fp32, and back; the sum and the maximum of a value over the 64 lanes of a wave, left in
// every lane.  Shared by attention.hip, row_norm.h, losses.hip, train.hip, roi_out.hip and per_class.hip.
template <typename T>
__device__ __forceinline__ float ldf(const T *p) { return (float)*p; }
template <typename T>
__device__ __forceinline__ void stf(T *p, float v) { *p = (T)v; }
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Box2BoxTransform.apply_deltas (frcnn.py:548-584) for one box, reference op order.  The one copy of the RoI decode:
// roi_out.hip (the arg-max class's box) and per_class.hip (every class's box) both call it, and both files build with
// -ffp-contract=off, so the two selection modes decode a (proposal, deltas) pair to the same bits.
__device__ __forceinline__ void apply_deltas_roi(const float a[4], const float d[4], float wx, float wy, float ww,
                                                 float wh, float clampv, float o[4]) {
    float widths = a[2] - a[0];
    float heights = a[3] - a[1];
    float ctr_x = a[0] + 0.5f * widths;
    float ctr_y = a[1] + 0.5f * heights;
    float dx = d[0] / wx;
    float dy = d[1] / wy;
    float dw = d[2] / ww;
    float dh = d[3] / wh;
    dw = dw > clampv ? clampv : dw;
    dh = dh > clampv ? clampv : dh;
    float pcx = dx * widths + ctr_x;
    float pcy = dy * heights + ctr_y;
    float pw = expf(dw) * widths;
    float ph = expf(dh) * heights;
    o[0] = pcx - 0.5f * pw;
    o[1] = pcy - 0.5f * ph;
    o[2] = pcx + 0.5f * pw;
    o[3] = pcy + 0.5f * ph;
}

// ---- per_class.hip (roi_outputs.selection = "per_class": vk_forward_begin_select, vk_per_class_select, vk_class_probs) ----
struct PerClassArgs {
    const float *scores;      // [K, ld_scores] class probabilities; the first C columns are used
    int ld_scores;
    const float *deltas;      // [K, ld_box]: 4 deltas per class (class c at column 4c), or 4 in all when agnostic
    int ld_box, agnostic;
    const float *proposals;   // [N, R, 4]
    const int32_t *counts;    // [N]
    const float *features;    // [K, F]
    const float *attr_prob;   // [K] or nullptr
    const int32_t *attr_cls;
    int F, R, D, C;
    const int32_t *image_hw;
    const float *scales_yx;
    float wx, wy, ww, wh, clampv;
    double thresh, score_thresh;
    int mind, maxd;
    unsigned long long *best;   // [K] scratch: (score bits << 32) | (C - c) of the best surviving class, 0 = none
    float *max_conf;            // [K] out (optional): max_conf[r], 0 for rows >= counts[n]
    vk_outputs out;
    int64_t *keep_ids;
    int32_t *nonfinite;
};
int launch_class_probs(const float *logits, int ld, int K, int n, float *out, int ld_out, hipStream_t s);
int launch_per_class_select(PerClassArgs &a, int N, hipStream_t s);
// out [N*R, C, 4]: every (row, class) box as the NMS kernel holds it; uses deltas, proposals, counts, image_hw, the weights
int launch_class_boxes(PerClassArgs &a, int N, float *out, hipStream_t s);

// The box of (row, class): decode + the finite-ness the reference asserts before the clip + _clip_box.  The one copy:
// per_class.hip and detections.hip both call it (both build with -ffp-contract=off), so a (row, class) box holds the
// same bits in every kernel of either selection.
__device__ __forceinline__ bool pc_box(const PerClassArgs &a, long row, int c, float img_w, float img_h, float b[4]) {
    const float *p = a.proposals + row * 4;
    const float pr[4] = {p[0], p[1], p[2], p[3]};
    const float *dp = a.deltas + row * a.ld_box + (a.agnostic ? 0 : 4 * c);
    const float d[4] = {dp[0], dp[1], dp[2], dp[3]};
    apply_deltas_roi(pr, d, a.wx, a.wy, a.ww, a.wh, a.clampv, b);
    const bool finite = isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]);
    b[0] = fminf(fmaxf(b[0], 0.f), img_w);
    b[1] = fminf(fmaxf(b[1], 0.f), img_h);
    b[2] = fminf(fmaxf(b[2], 0.f), img_w);
    b[3] = fminf(fmaxf(b[3], 0.f), img_h);
    return finite;
}

// ---- detections.hip (roi_outputs.selection = "detections": vk_forward_begin_select, vk_detections_select) ----
// pc: scores, deltas, proposals, counts, features, attr_*, F, R, C, image_hw, scales_yx, the weights, thresh, score_thresh,
// D (= max_detections), out, keep_ids, nonfinite as in the per-class mode; mind, maxd, best and max_conf are unused.
struct DetArgs {
    PerClassArgs pc;
    int32_t *cand_cnt;             // [N * C] candidates of (image, class); followed by surv_cnt, zeroed by the launcher
    int32_t *surv_cnt;             // [N] NMS survivors of the image
    uint16_t *cand;                // [N * C][R] candidate rows, in no particular order
    unsigned long long *surv;      // [N][R * C] survivor keys (desc_key32(score) << 32) | (r << 20 | c), in no particular order
    int32_t *n_survivors;          // [N] out (optional)
};
// bytes of the region that cand_cnt .. surv are carved from (det_carve), 256-byte aligned pieces
size_t det_workspace_bytes(int N, int R, int C);
void det_carve(DetArgs &d, char *base, int N, int R, int C);
int launch_detections_select(DetArgs &d, int N, hipStream_t s);

// assign_boxes_to_levels frcnn.py:444-460 for one box: floor(canonical_level + log2(sqrt(area) / canonical_size + 1e-8)),
// clamped to [min_level, max_level], minus min_level.  The one copy of the rule: fpn.hip's assign_levels_kernel and
// given_boxes.hip's ingest both call it, and both files build with -ffp-contract=off, so their levels are bit-equal.
__device__ __forceinline__ int32_t box_level(float x0, float y0, float x1, float y1, int min_level, int max_level,
                                             float canonical_size, int canonical_level) {
    const float area = (x1 - x0) * (y1 - y0);
    float lv = floorf((float)canonical_level + log2f(sqrtf(area) / canonical_size + 1e-8f));
    lv = fminf(fmaxf(lv, (float)min_level), (float)max_level);      // NaN (negative area) clamps like torch.clamp: stays NaN -> cast
    return (int32_t)lv - min_level;
}

// ---- given_boxes.hip (vk_forward_boxes_begin, vk_given_boxes_ingest, vk_given_box_outputs) ----
// boxes [N,B,4] (rows >= counts[n] ignored) -> / scales_yx -> non-finite flag -> _clip_box -> prop_boxes [N,B,4], rois [N*B,5]
int launch_given_boxes_ingest(const float *boxes, const int32_t *counts, const int32_t *image_hw, const float *scales_yx, int N,
                              int B, float *prop_boxes, float *rois, int32_t *nonfinite, hipStream_t s);
// the same, plus each row's pyramid level (box_level of the clipped box) into levels [N*B]: the FPN detector's RoI input
// in one launch (in place of vk_make_rois + vk_assign_levels)
int launch_given_boxes_ingest_levels(const float *boxes, const int32_t *counts, const int32_t *image_hw, const float *scales_yx,
                                     int N, int B, float *prop_boxes, float *rois, int32_t *levels, int min_level, int max_level,
                                     float canonical_size, int canonical_level, int32_t *nonfinite, hipStream_t s);
// vk_outputs [N,B] from the per-row predictions, the clipped boxes times the scales and the feature rows
int launch_given_box_outputs(const float *obj_prob, const int32_t *obj_cls, const float *attr_prob, const int32_t *attr_cls,
                             const float *prop_boxes, const int32_t *counts, const float *scales_yx, const float *feat, int F,
                             int N, int B, const vk_outputs &out, hipStream_t s);

}  // namespace vk
