// The stage-level C entry points of libvltk_hip.so: everything callable without a model handle (the tests and the FPN
// detector, vltk_amd/frcnn_fpn.py, compose from these), and the one builder of each launch's argument block, which the
// C4 model (model.hip) calls too -- so what a stage-level call passes to a kernel is what the model passes.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "vk_common.h"

using namespace vk;

namespace vk {

// The layer of a stage-level launch as the dispatcher sees it: the one place vk_conv2d, vk_conv1x1_dual, vk_linear,
// vk_conv1x1_meanpool and vk_conv_route build their ConvArgs, so what the query describes is what the launch passes.  The
// pointers (and Cin2 with x2) are the caller's to set.
void fill_conv_args(ConvArgs &a, int N, int H, int W, int cin, int cout, int ldy, int k, int stride, int pad, int dil, int groups,
                    int relu, vk_dtype dt, vk_dtype out_dt) {
    memset(&a, 0, sizeof(a));
    a.N = N;
    a.H = H;
    a.W = W;
    a.Cin = cin;
    conv_out_hw(H, W, k, stride, pad, dil, &a.Ho, &a.Wo);
    a.Cout = cout;
    a.ldy = ldy;
    a.kh = a.kw = k;
    a.stride = stride;
    a.pad = pad;
    a.dil = dil;
    a.groups = groups;
    a.relu = relu;
    a.dt = dt;
    a.out_dt = out_dt;
}

static void stem_geom(int H, int W, int *H1, int *W1, int *Hp, int *Wp) {
    conv_out_hw(H, W, 7, 2, 3, 1, H1, W1);
    *Hp = std::max(H + 6, 2 * *H1 + 6);
    *Wp = (std::max(W + 6, 2 * *W1 + 6) + 1) & ~1;
}

int stem_impl(const float *x, int N, int H, int W, const void *w, const float *b, int cout, int caffe, void *y, vk_dtype dt,
              void *img_pad, void *stem_out, hipStream_t s, int32_t *nonfinite) {
    int H1, W1, Hp, Wp;
    stem_geom(H, W, &H1, &W1, &Hp, &Wp);
    VK_TRY(launch_stem_pack(x, img_pad, N, H, W, Hp, Wp, dt, s, nonfinite));
    if (stem_pool_eligible(cout, dt)) return launch_stem_pool(img_pad, N, Hp, Wp, H1, W1, w, b, caffe, y, s);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = img_pad;
    a.w = w;
    a.bias = b;
    a.y = stem_out;
    a.N = N;
    a.H = Hp;
    a.W = Wp;
    a.Cin = 4;
    a.Ho = H1;
    a.Wo = W1;
    a.Cout = cout;
    a.ldy = (cout + 7) / 8 * 8;
    a.kh = a.kw = 7;
    a.stride = 2;
    a.pad = 0;
    a.dil = 1;
    a.relu = 1;
    a.stem = 1;
    a.dt = a.out_dt = dt;
    VK_TRY(launch_conv(a, s));
    return launch_maxpool(stem_out, y, N, H1, W1, cout, caffe, dt, s);
}

// BBOX_XFORM_CLIP of Box2BoxTransform (frcnn.py:548-584): the bound on dw / dh, written once
static const float kDeltaClamp = (float)std::log(1000.0 / 16.0);

// The one place a PerClassArgs is built: the model's two all-class selections (model.hip) and the stage-level
// vk_per_class_select / vk_detections_select / vk_class_boxes call it and then set only what is their own (best, max_conf, the
// det_carve pieces, n_survivors).  sp == nullptr (vk_class_boxes) leaves D, the thresholds, mind and maxd zero; out == nullptr
// leaves the output block zero.
void fill_per_class_args(PerClassArgs &a, const float *scores, int ld_scores, const float *deltas, int ld_box, int agnostic,
                         const float *proposals, const int32_t *counts, const float *features, const float *attr_prob,
                         const int32_t *attr_cls, int F, int R, int C, const int32_t *image_hw, const float *scales_yx,
                         const float *weights4, const vk_select_params *sp, const vk_outputs *out, int64_t *keep_ids,
                         int32_t *nonfinite) {
    memset(&a, 0, sizeof(a));
    a.scores = scores;
    a.ld_scores = ld_scores;
    a.deltas = deltas;
    a.ld_box = ld_box;
    a.agnostic = agnostic ? 1 : 0;
    a.proposals = proposals;
    a.counts = counts;
    a.features = features;
    a.attr_prob = attr_prob;
    a.attr_cls = attr_cls;
    a.F = F;
    a.R = R;
    a.C = C;
    a.image_hw = image_hw;
    a.scales_yx = scales_yx;
    a.wx = weights4[0];
    a.wy = weights4[1];
    a.ww = weights4[2];
    a.wh = weights4[3];
    a.clampv = kDeltaClamp;
    if (sp) {
        a.D = sp->roi.max_detections;
        a.thresh = sp->roi.nms_thresh[0];
        a.score_thresh = sp->score_thresh;
        a.mind = sp->roi.min_detections;
        a.maxd = sp->roi.max_detections;
    }
    if (out) a.out = *out;
    a.keep_ids = keep_ids;
    a.nonfinite = nonfinite;
}

// The one place a RoiFinalArgs is built (ROIOutputs.inference frcnn.py:1262-1294): the model's class-max end and vk_roi_outputs.
// delta_mode as in RoiFinalArgs: 0 for all-class deltas [K, 4C], 1 for the 4 chosen / agnostic ones.
void fill_roi_final_args(RoiFinalArgs &a, const float *obj_prob, const int32_t *obj_cls, const float *attr_prob,
                         const int32_t *attr_cls, const float *box_deltas, int ld_box, int delta_mode, const float *proposals,
                         const int32_t *counts, const float *features, int F, int R, const int32_t *image_hw,
                         const float *scales_yx, const float *weights4, const vk_roi_params *rp, const vk_outputs *out,
                         int64_t *keep_ids, int32_t *nonfinite) {
    memset(&a, 0, sizeof(a));
    a.obj_prob = obj_prob;
    a.obj_cls = obj_cls;
    a.attr_prob = attr_prob;
    a.attr_cls = attr_cls;
    a.box_deltas = box_deltas;
    a.ld_box = ld_box;
    a.delta_mode = delta_mode;
    a.proposals = proposals;
    a.counts = counts;
    a.features = features;
    a.F = F;
    a.R = R;
    a.D = rp->max_detections;
    a.image_hw = image_hw;
    a.scales_yx = scales_yx;
    a.wx = weights4[0];
    a.wy = weights4[1];
    a.ww = weights4[2];
    a.wh = weights4[3];
    a.clampv = kDeltaClamp;
    a.n_thresh = rp->num_nms_thresh;
    for (int i = 0; i < rp->num_nms_thresh; ++i) a.thresh[i] = rp->nms_thresh[i];
    a.mind = rp->min_detections;
    a.maxd = rp->max_detections;
    a.out = *out;
    a.keep_ids = keep_ids;
    a.nonfinite = nonfinite;
}

int check_select_params(const vk_select_params *sp, const char *who) {
    const vk_roi_params &rp = sp->roi;
    VK_REQUIRE(rp.num_nms_thresh == 1, VK_EINVAL, "%s: per-class selection takes one NMS threshold, got a list of %d", who, rp.num_nms_thresh);
    VK_REQUIRE(sp->score_thresh >= 0.0 && sp->score_thresh <= 1.0, VK_EINVAL, "%s: score_thresh=%g must be in [0, 1]", who, sp->score_thresh);
    VK_REQUIRE(rp.min_detections <= rp.max_detections, VK_EINVAL, "%s: min_detections=%d exceeds max_detections=%d", who,
               rp.min_detections, rp.max_detections);
    return VK_OK;
}

int check_detections_params(const vk_select_params *sp, const char *who) {
    const vk_roi_params &rp = sp->roi;
    VK_REQUIRE(rp.num_nms_thresh == 1, VK_EINVAL, "%s: the detections selection takes one NMS threshold, got a list of %d", who, rp.num_nms_thresh);
    VK_REQUIRE(sp->score_thresh >= 0.0 && sp->score_thresh <= 1.0, VK_EINVAL, "%s: score_thresh=%g must be in [0, 1]", who, sp->score_thresh);
    VK_REQUIRE(rp.min_detections == 0, VK_EINVAL, "%s: min_detections=%d must be 0 with the detections selection: a detector reports "
               "nothing when nothing clears score_thresh, so there is no minimum count to fill (clear the config's MIN_DETECTIONS)",
               who, rp.min_detections);
    VK_REQUIRE(rp.max_detections >= 1 && rp.max_detections <= 1024, VK_EINVAL, "%s: max_detections=%d must be in 1..1024", who,
               rp.max_detections);
    return VK_OK;
}

}  // namespace vk

extern "C" {

int vk_conv2d(const void *x, int N, int H, int W, int cin, const void *w_packed, const float *bias_packed,
              const void *residual, void *y, int cout, int ldy, int kh, int kw, int stride, int pad, int dil, int groups,
              int relu, vk_dtype dt, vk_dtype out_dt, void *stream) {
    VK_REQUIRE(kh == kw && kh >= 1 && stride >= 1 && dil >= 1 && pad >= 0 && groups >= 1, VK_EINVAL, "conv2d: bad geometry");
    ConvArgs a;
    fill_conv_args(a, N, H, W, cin, cout, ldy, kh, stride, pad, dil, groups, relu, dt, out_dt);
    VK_REQUIRE(a.Ho > 0 && a.Wo > 0 && N > 0, VK_EINVAL, "conv2d: empty output");
    a.x = x;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    return launch_conv(a, (hipStream_t)stream);
}

int vk_conv_route(int N, int H, int W, int cin, int cin2, int has_residual, int fused_mean, int cout, int ldy, int kh, int kw,
                  int stride, int pad, int dil, int groups, int relu, vk_dtype dt, vk_dtype out_dt) {
    if (!(kh == kw && kh >= 1 && stride >= 1 && dil >= 1 && pad >= 0 && groups >= 1 && cin2 >= 0)) {
        set_error("conv_route: bad geometry");
        return -VK_EINVAL;
    }
    static const char here = 0;              // the rules only ask whether a pointer is set
    ConvArgs a;
    fill_conv_args(a, N, H, W, cin, cout, ldy, kh, stride, pad, dil, groups, relu, dt, out_dt);
    if (!(a.Ho > 0 && a.Wo > 0 && N > 0)) {
        set_error("conv_route: empty output");
        return -VK_EINVAL;
    }
    a.x = a.w = &here;
    a.res = has_residual ? &here : nullptr;
    a.x2 = cin2 > 0 ? &here : nullptr;
    a.Cin2 = cin2;
    a.pool_part = fused_mean ? (float *)&here : nullptr;
    return conv_route_checked(a);
}

int vk_panel_phase_images(int N, int H, int W, int dil) {
    ConvArgs a;
    fill_conv_args(a, N, H, W, 128, 256, 256, 3, 1, dil, dil, 1, 0, VK_F16, VK_F16);
    return conv3x3_panel_phase_images(a);
}

int vk_panel_phase_tile_rows(int N, int H, int W, int dil, int cout) {
    ConvArgs a;
    fill_conv_args(a, N, H, W, 128, cout, cout, 3, 1, dil, dil, 1, 0, VK_F16, VK_F16);
    return conv3x3_panel_phase_tile_rows(a);
}

int vk_panel_phase_reuse(int N, int H, int W, int dil, int cout) {
    ConvArgs a;
    fill_conv_args(a, N, H, W, 128, cout, cout, 3, 1, dil, dil, 1, 0, VK_F16, VK_F16);
    return conv3x3_panel_phase_reuse(a);
}

int vk_panel_phase_indexed(int N, int H, int W, int dil, int cout) {
    ConvArgs a;
    fill_conv_args(a, N, H, W, 128, cout, cout, 3, 1, dil, dil, 1, 0, VK_F16, VK_F16);
    return conv3x3_panel_phase_indexed(a);
}

int vk_conv2d_rows(const void *x, long x_rows, const int32_t *x_idx, int N, int H, int W, int cin, const void *w_packed,
                   const float *bias_packed, const void *residual, void *y, int cout, int dil, int relu, void *stream) {
    VK_REQUIRE(x_idx && x_rows > 0 && N > 0 && H > 0 && W > 0 && dil >= 1, VK_EINVAL, "conv2d_rows: bad arguments");
    ConvArgs a;
    fill_conv_args(a, N, H, W, cin, cout, cout, 3, 1, dil, dil, 1, relu, VK_F16, VK_F16);
    a.x = x;
    a.x_idx = x_idx;
    a.x_rows = x_rows;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    return launch_conv(a, (hipStream_t)stream);
}

int vk_panel_out_indexed(int N, int H, int W, int dil, int cout) {
    ConvArgs a;
    fill_conv_args(a, N, H, W, 128, cout, cout, 3, 1, dil, dil, 1, 0, VK_F16, VK_F16);
    return conv3x3_panel_out_indexed(a);
}

int vk_conv2d_rows_out(const void *x, long x_rows, const int32_t *x_idx, int N, int H, int W, int cin, const void *w_packed,
                       const float *bias_packed, const void *residual, void *y, long y_rows, const int32_t *y_idx, int cout, int dil,
                       int relu, void *stream) {
    VK_REQUIRE(y_idx && (!x_idx || x_rows > 0) && N > 0 && H > 0 && W > 0 && dil >= 1, VK_EINVAL, "conv2d_rows_out: bad arguments");
    ConvArgs a;
    fill_conv_args(a, N, H, W, cin, cout, cout, 3, 1, dil, dil, 1, relu, VK_F16, VK_F16);
    a.x = x;
    a.x_idx = x_idx;
    a.x_rows = x_idx ? x_rows : 0;
    a.y_idx = y_idx;
    a.y_rows = y_rows;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    return launch_conv(a, (hipStream_t)stream);
}

int vk_conv1x1_dual(const void *x1, int cin1, const void *x2, int cin2, long M, const void *w_packed, const float *bias_packed,
                    const void *residual, void *y, int cout, int relu, void *stream) {
    VK_REQUIRE(x1 && x2 && M > 0 && M < (1L << 31), VK_EINVAL, "conv1x1_dual: bad arguments");
    ConvArgs a;
    fill_conv_args(a, 1, 1, (int)M, cin1, cout, cout, 1, 1, 0, 1, 1, relu, VK_F16, VK_F16);
    a.x = x1;
    a.x2 = x2;
    a.Cin2 = cin2;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    return launch_conv(a, (hipStream_t)stream);
}

int vk_conv1x1_rows(const void *x1, int cin1, const void *x2, int cin2, long M, const int32_t *m_dev, const int32_t *x2_idx,
                    const void *w_packed, const float *bias_packed, void *y, int cout, int relu, void *stream) {
    VK_REQUIRE(x1 && w_packed && bias_packed && y && M > 0 && M < (1L << 31), VK_EINVAL, "conv1x1_rows: bad arguments");
    VK_REQUIRE(!x2_idx || x2, VK_EINVAL, "conv1x1_rows: a row index needs a second input");
    ConvArgs a;
    fill_conv_args(a, 1, 1, (int)M, cin1, cout, cout, 1, 1, 0, 1, 1, relu, VK_F16, VK_F16);
    a.x = x1;
    a.x2 = x2;
    a.Cin2 = x2 ? cin2 : 0;
    a.w = w_packed;
    a.bias = bias_packed;
    a.y = y;
    VK_REQUIRE(conv_route(a) == VK_ROUTE_GEMM4, VK_EINVAL, "conv1x1_rows: the layer does not run as VK_ROUTE_GEMM4 at %ld rows", M);
    a.m_dev = m_dev;
    a.x2_idx = x2_idx;
    return launch_conv_gemm4(a, (hipStream_t)stream);
}

int vk_conv1x1_res_rows(const void *x, int cin, long M, const void *w_packed, const float *bias_packed, const void *residual,
                        const int32_t *res_idx, void *y, int cout, int relu, void *stream) {
    VK_REQUIRE(x && w_packed && bias_packed && residual && y && M > 0 && M < (1L << 31), VK_EINVAL, "conv1x1_res_rows: bad arguments");
    ConvArgs a;
    fill_conv_args(a, 1, 1, (int)M, cin, cout, cout, 1, 1, 0, 1, 1, relu, VK_F16, VK_F16);
    a.x = x;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    VK_REQUIRE(conv_ws_res_indexed(a), VK_EINVAL,
               "conv1x1_res_rows: not a layer of the VK_ROUTE_WS kernel's K = 512 build with two waves per SIMD (cin %d, cout %d)", cin, cout);
    a.res_idx = res_idx;
    return launch_conv_ws(a, (hipStream_t)stream);
}

int vk_linear(const void *x, long M, int K, const void *w_packed, const float *bias_packed, const void *residual, void *y, int N, int ldy,
              int act, vk_dtype dt, vk_dtype out_dt, void *stream) {
    VK_REQUIRE(x && w_packed && bias_packed && y && M > 0 && M < (1L << 31), VK_EINVAL, "linear: bad arguments");
    ConvArgs a;
    fill_conv_args(a, 1, 1, (int)M, K, N, ldy, 1, 1, 0, 1, 1, act, dt, out_dt);
    a.x = x;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.y = y;
    return launch_conv(a, (hipStream_t)stream);
}

// The fused-shortcut rule is restated in oracle/frcnn_oracle.py (fp16 emulation): keep the two in step.
int vk_fuse_shortcut(int cin, int cin_shortcut, int cout, int stride, vk_dtype dt) {
    static const bool off = env_set("VK_NO_FUSED_SHORTCUT");
    return !off && dt == VK_F16 && stride == 1 && cout % 256 == 0 && cin % 32 == 0 && cin_shortcut % 32 == 0;
}

int vk_bottleneck64_eligible(int cin, int cmid, int cout, int stride, int dil, int groups, int proj, int fused_shortcut, long N,
                             int H, int W, vk_dtype dt) {
    return stride == 1 && dil == 1 && (!proj || fused_shortcut) &&
           bneck_fused_eligible(cin, cmid, cout, stride, groups, proj != 0, N, H, W, dt);
}

int vk_bottleneck64(const void *x, int N, int H, int W, int cin, int proj, const void *w1, const float *b1, const void *w2,
                    const float *b2, const void *w3, const float *b3, void *y, void *stream) {
    VK_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && y && N > 0 && H > 0 && W > 0, VK_EINVAL, "bottleneck64: bad arguments");
    VK_REQUIRE((cin == 256 && !proj) || (cin == 64 && proj), VK_EINVAL, "bottleneck64: cin must be 256 (identity) or 64 (projection)");
    VK_REQUIRE(bneck_fused_eligible(cin, 64, 256, 1, 1, proj != 0, N, H, W, VK_F16) || bneck_fused_forced(), VK_EINVAL,
               "bottleneck64: tensor beyond the 32-bit byte offsets");
    VK_REQUIRE((long)N * H * W * 512 < (1L << 32) - (1L << 20), VK_EINVAL, "bottleneck64: tensor beyond the 32-bit byte offsets");
    return launch_bneck_fused(x, N, H, W, cin, proj != 0, w1, b1, w2, b2, w3, b3, y, false, (hipStream_t)stream);
}

size_t vk_conv1x1_meanpool_workspace_bytes(int N, int HW, int cout) { return conv_duo_pool_part_bytes((long)N * HW, cout); }

int vk_conv1x1_meanpool(const void *x, int N, int HW, int cin, const void *w_packed, const float *bias_packed,
                        const void *residual, int cout, int relu, float *out_mean, void *workspace, size_t workspace_bytes,
                        void *stream) {
    VK_REQUIRE(x && out_mean && workspace && N > 0 && HW > 0, VK_EINVAL, "conv1x1_meanpool: bad arguments");
    VK_REQUIRE(workspace_bytes >= vk_conv1x1_meanpool_workspace_bytes(N, HW, cout), VK_EINVAL, "conv1x1_meanpool: workspace too small");
    ConvArgs a;
    fill_conv_args(a, N, 1, HW, cin, cout, cout, 1, 1, 0, 1, 1, relu, VK_F16, VK_F16);
    a.x = x;
    a.w = w_packed;
    a.bias = bias_packed;
    a.res = residual;
    a.pool_part = (float *)workspace;
    VK_TRY(launch_conv(a, (hipStream_t)stream));
    return launch_pool_finish((const float *)workspace, N, HW, cin, cout, false, out_mean, (hipStream_t)stream);
}

size_t vk_stem_workspace_bytes(int N, int H, int W, int cout, vk_dtype dt) {
    int H1, W1, Hp, Wp;
    stem_geom(H, W, &H1, &W1, &Hp, &Wp);
    return align_up((size_t)N * Hp * Wp * 4 * dtype_size(dt), 256) + align_up((size_t)N * H1 * W1 * cout * dtype_size(dt), 256);
}

int vk_stem(const float *x, int N, int H, int W, const void *w_packed, const float *bias_packed, int cout,
            int caffe_maxpool, void *y, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream) {
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32, VK_EINVAL, "stem: bad dtype");
    VK_REQUIRE(cout % 8 == 0, VK_EINVAL, "stem: cout must be a multiple of 8");
    VK_REQUIRE(H >= 16 && W >= 16, VK_EINVAL, "stem: image %dx%d too small", H, W);
    VK_REQUIRE(workspace && workspace_bytes >= vk_stem_workspace_bytes(N, H, W, cout, dt), VK_EINVAL, "stem: workspace too small");
    int H1, W1, Hp, Wp;
    stem_geom(H, W, &H1, &W1, &Hp, &Wp);
    char *img_pad = (char *)workspace;
    char *stem_out = img_pad + align_up((size_t)N * Hp * Wp * 4 * dtype_size(dt), 256);
    return stem_impl(x, N, H, W, w_packed, bias_packed, cout, caffe_maxpool, y, dt, img_pad, stem_out, (hipStream_t)stream);
}

int vk_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream) {
    VK_REQUIRE(dst_dev && src_dev, VK_EINVAL, "memcpy_d2d: null pointer");
    VK_CHECK_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VK_OK;
}

// ---- pieces of FastRCNNOutputLayers.forward (frcnn.py:1726-1740) / ROIPooler input format (:426-441) for callers that
// compose a box head themselves (the FPN detector, vltk_amd/frcnn_fpn.py) ----
int vk_make_rois(const float *boxes, int N, int R, float *rois, void *stream) {
    VK_REQUIRE(boxes && rois && N > 0 && R > 0, VK_EINVAL, "make_rois: bad arguments");
    return launch_make_rois(boxes, N, R, rois, (hipStream_t)stream);
}

int vk_softmax_argmax(const float *logits, int ld, int K, int n_softmax, int n_argmax, float *prob_out, int32_t *cls_out,
                      int32_t *raw_argmax_out, void *stream) {
    VK_REQUIRE(logits && prob_out && cls_out && K >= 0 && n_softmax >= 1 && n_argmax >= 1 && n_argmax <= n_softmax && ld >= n_softmax,
               VK_EINVAL, "softmax_argmax: bad arguments");
    return launch_softmax_argmax(logits, ld, K, n_softmax, n_argmax, prob_out, cls_out, raw_argmax_out, (hipStream_t)stream);
}

int vk_concat_embed(const float *features, int F, const void *emb, int E, const int32_t *cls, int K, void *out, vk_dtype dt,
                    void *stream) {
    VK_REQUIRE(features && out && F > 0 && E >= 0 && K >= 0 && (E == 0 || (emb && cls)), VK_EINVAL, "concat_embed: bad arguments");
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32, VK_EINVAL, "concat_embed: dtype must be f16 or f32");
    return launch_concat_embed(features, emb, cls, F, E, K, out, dt, (hipStream_t)stream);
}

int vk_chosen_deltas(const void *x, int ldx, const void *w_rows, const float *bias, const int32_t *cls, int cls_agnostic, int F,
                     int K, float *out, vk_dtype dt, void *stream) {
    VK_REQUIRE(x && w_rows && bias && out && (cls || cls_agnostic) && F > 0 && ldx >= F && K >= 0, VK_EINVAL, "chosen_deltas: bad arguments");
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32, VK_EINVAL, "chosen_deltas: dtype must be f16 or f32");
    return launch_chosen_deltas(x, ldx, w_rows, bias, cls, cls_agnostic, F, K, out, dt, (hipStream_t)stream);
}

int vk_roi_outputs(const float *obj_logits, int ld_obj, const float *attr_logits, int ld_attr, const float *box_deltas,
                   int ld_box, int chosen_only, const float *proposals, const int32_t *counts, const float *features, int F,
                   int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                   const float *weights4_host, const vk_roi_params *rp, const vk_outputs *out, int64_t *keep_ids_out,
                   int32_t *nonfinite_flag, void *stream) {
    VK_REQUIRE(obj_logits && box_deltas && proposals && counts && features && image_hw && rp && out && nonfinite_flag, VK_EINVAL,
               "roi_outputs: null argument");
    VK_REQUIRE(rp->num_nms_thresh >= 1 && rp->num_nms_thresh <= VK_MAX_NMS_THRESH, VK_EINVAL, "roi_outputs: 1..%d nms thresholds", VK_MAX_NMS_THRESH);
    hipStream_t s = (hipStream_t)stream;
    const int K = N * R;
    // scratch for the per-RoI scores (freed after the stream drains; stage-level entry point only)
    char *scratch = nullptr;
    const size_t per = align_up((size_t)K * 4, 256);
    VK_CHECK_HIP(hipMalloc((void **)&scratch, per * 4));
    float *obj_prob = (float *)scratch, *attr_prob = (float *)(scratch + per);
    int32_t *obj_cls = (int32_t *)(scratch + 2 * per), *attr_cls = (int32_t *)(scratch + 3 * per);
    int st = launch_softmax_argmax(obj_logits, ld_obj, K, C + 1, C, obj_prob, obj_cls, nullptr, s);
    if (st == VK_OK && attr_logits) st = launch_softmax_argmax(attr_logits, ld_attr, K, A, A, attr_prob, attr_cls, nullptr, s);
    if (st == VK_OK) {
        RoiFinalArgs a;
        fill_roi_final_args(a, obj_prob, obj_cls, attr_logits ? attr_prob : nullptr, attr_logits ? attr_cls : nullptr, box_deltas, ld_box,
                            chosen_only ? 1 : 0, proposals, counts, features, F, R, image_hw, scales_yx_dev, weights4_host, rp, out,
                            keep_ids_out, nonfinite_flag);
        st = launch_roi_final(a, N, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (st != VK_OK) return st;
    VK_CHECK_HIP(e);
    return VK_OK;
}

int vk_class_probs(const float *logits, int ld, int K, int n, float *out, int ld_out, void *stream) {
    VK_REQUIRE(logits && out && K >= 0 && n >= 1 && ld >= n && ld_out >= n, VK_EINVAL, "class_probs: bad arguments");
    return launch_class_probs(logits, ld, K, n, out, ld_out, (hipStream_t)stream);
}

int vk_class_boxes(const float *box_deltas, int ld_box, int cls_agnostic, const float *proposals, const int32_t *counts, int N, int R,
                   int C, const int32_t *image_hw, const float *weights4_host, float *out, int32_t *nonfinite_flag, void *stream) {
    VK_REQUIRE(box_deltas && proposals && counts && image_hw && weights4_host && out, VK_EINVAL, "class_boxes: null argument");
    PerClassArgs a;
    fill_per_class_args(a, nullptr, 0, box_deltas, ld_box, cls_agnostic, proposals, counts, nullptr, nullptr, nullptr, 0, R, C, image_hw,
                        nullptr, weights4_host, nullptr, nullptr, nullptr, nonfinite_flag);
    return launch_class_boxes(a, N, out, (hipStream_t)stream);
}

int vk_per_class_select(const float *obj_scores, int ld_scores, const float *attr_logits, int ld_attr, const float *box_deltas,
                        int ld_box, int cls_agnostic, const float *proposals, const int32_t *counts, const float *features, int F,
                        int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                        const float *weights4_host, const vk_select_params *sp, const vk_outputs *out, int64_t *keep_ids_out,
                        float *max_conf_out, int32_t *nonfinite_flag, void *stream) {
    VK_REQUIRE(obj_scores && box_deltas && proposals && counts && features && image_hw && weights4_host && sp && out && nonfinite_flag,
               VK_EINVAL, "per_class_select: null argument");
    VK_REQUIRE(sp->mode == VK_SELECT_PER_CLASS, VK_EINVAL, "per_class_select: mode=%d is not VK_SELECT_PER_CLASS", sp->mode);
    VK_TRY(check_select_params(sp, "per_class_select"));
    VK_REQUIRE(N >= 1 && N <= 65535 && R >= 1 && R <= 1024 && C >= 1, VK_EINVAL, "per_class_select: N=%d R=%d C=%d (R at most 1024)", N, R, C);
    VK_REQUIRE(sp->roi.max_detections >= 1 && sp->roi.max_detections <= R, VK_EINVAL, "per_class_select: max_detections=%d must be in 1..R=%d",
               sp->roi.max_detections, R);
    VK_REQUIRE(F >= 4 && F % 4 == 0, VK_EINVAL, "per_class_select: F=%d must be a positive multiple of 4", F);
    VK_REQUIRE(!attr_logits || (A >= 1 && ld_attr >= A), VK_EINVAL, "per_class_select: A=%d ld_attr=%d", A, ld_attr);
    hipStream_t s = (hipStream_t)stream;
    const int K = N * R;
    // scratch: the best-class words and the per-row attribute predictions (freed after the stream drains; stage-level entry point only)
    char *scratch = nullptr;
    const size_t per = align_up((size_t)K * 8, 256);
    VK_CHECK_HIP(hipMalloc((void **)&scratch, per * 3));
    float *attr_prob = (float *)(scratch + per);
    int32_t *attr_cls = (int32_t *)(scratch + 2 * per);
    int st = VK_OK;
    if (attr_logits) st = launch_softmax_argmax(attr_logits, ld_attr, K, A, A, attr_prob, attr_cls, nullptr, s);
    if (st == VK_OK) {
        PerClassArgs a;
        fill_per_class_args(a, obj_scores, ld_scores, box_deltas, ld_box, cls_agnostic, proposals, counts, features,
                            attr_logits ? attr_prob : nullptr, attr_logits ? attr_cls : nullptr, F, R, C, image_hw, scales_yx_dev,
                            weights4_host, sp, out, keep_ids_out, nonfinite_flag);
        a.best = (unsigned long long *)scratch;
        a.max_conf = max_conf_out;
        st = launch_per_class_select(a, N, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (st != VK_OK) return st;
    VK_CHECK_HIP(e);
    return VK_OK;
}

int vk_detections_lds_keys(void) { return VK_DETECTIONS_LDS_KEYS; }

int vk_detections_select(const float *obj_scores, int ld_scores, const float *attr_logits, int ld_attr, const float *box_deltas,
                         int ld_box, int cls_agnostic, const float *proposals, const int32_t *counts, const float *features, int F,
                         int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                         const float *weights4_host, const vk_select_params *sp, const vk_outputs *out, int64_t *keep_ids_out,
                         int32_t *n_survivors_out, int32_t *nonfinite_flag, void *stream) {
    VK_REQUIRE(obj_scores && box_deltas && proposals && counts && features && image_hw && weights4_host && sp && out && nonfinite_flag,
               VK_EINVAL, "detections_select: null argument");
    VK_REQUIRE(sp->mode == VK_SELECT_DETECTIONS, VK_EINVAL, "detections_select: mode=%d is not VK_SELECT_DETECTIONS", sp->mode);
    VK_TRY(check_detections_params(sp, "detections_select"));
    VK_REQUIRE(N >= 1 && N <= 65535 && R >= 1 && R <= 1024 && C >= 1 && C < (1 << 20), VK_EINVAL,
               "detections_select: N=%d R=%d C=%d (N at most 65535, R at most 1024, C below 2^20)", N, R, C);
    VK_REQUIRE(F >= 4 && F % 4 == 0, VK_EINVAL, "detections_select: F=%d must be a positive multiple of 4", F);
    VK_REQUIRE(!attr_logits || (A >= 1 && ld_attr >= A), VK_EINVAL, "detections_select: A=%d ld_attr=%d", A, ld_attr);
    VK_REQUIRE(ld_scores >= C && ld_box >= (cls_agnostic ? 4 : 4 * C), VK_EINVAL, "detections_select: row strides ld_scores=%d "
               "ld_box=%d are shorter than the rows", ld_scores, ld_box);
    hipStream_t s = (hipStream_t)stream;
    const int K = N * R;
    // scratch: the per-row attribute predictions and the candidate / survivor lists, from the device's pool in stream order
    const size_t per = align_up((size_t)K * 4, 256);
    char *scratch = nullptr;
    VK_CHECK_HIP(hipMallocAsync((void **)&scratch, 2 * per + det_workspace_bytes(N, R, C), s));
    float *attr_prob = (float *)scratch;
    int32_t *attr_cls = (int32_t *)(scratch + per);
    int st = VK_OK;
    if (attr_logits) st = launch_softmax_argmax(attr_logits, ld_attr, K, A, A, attr_prob, attr_cls, nullptr, s);
    if (st == VK_OK) {
        DetArgs d;
        memset(&d, 0, sizeof(d));
        fill_per_class_args(d.pc, obj_scores, ld_scores, box_deltas, ld_box, cls_agnostic, proposals, counts, features,
                            attr_logits ? attr_prob : nullptr, attr_logits ? attr_cls : nullptr, F, R, C, image_hw, scales_yx_dev,
                            weights4_host, sp, out, keep_ids_out, nonfinite_flag);
        det_carve(d, scratch + 2 * per, N, R, C);
        d.n_survivors = n_survivors_out;
        st = launch_detections_select(d, N, s);
    }
    hipError_t e = hipFreeAsync(scratch, s);
    if (st != VK_OK) return st;
    VK_CHECK_HIP(e);
    return VK_OK;
}

}  // extern "C"
