/*
 * vltk_hip.h -- C ABI of libvltk_hip.so: the MI355X (gfx950) implementation of
 * vltk's Faster R-CNN visual-feature extraction forward pass.
 *
 * This is the drop-in boundary.  The reference has no native layer (it is
 * pure Python over torch/torchvision), so every entry point below replaces a
 * Python-level interface of /root/reference/vltk/modeling/frcnn.py; the
 * file:line each one stands in for is given per function.  A maintainer binds
 * these with ctypes; vltk_amd/_lib.py is that binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - Every function returns an int status: VK_OK (0) or a VK_E* code;
 *     vk_last_error() returns a thread-local message for the last failure.
 *   - "dev" pointers are device (HBM) pointers owned by the caller; "host"
 *     pointers are ordinary host memory.  `stream` is a hipStream_t passed as
 *     void* (NULL = the default stream).
 *   - Activations are NHWC ("pixel-major": a feature map is a row-major
 *     [N*H*W, C] matrix), dtype per vk_dtype; boxes are (x1,y1,x2,y2) f32.
 */
#ifndef VLTK_HIP_H
#define VLTK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_OK 0
#define VK_EINVAL 1      /* bad argument / unsupported configuration  -> ValueError      */
#define VK_ENOTIMPL 2    /* reference raises NotImplementedError (frcnn.py:1930)         */
#define VK_ENONFINITE 3  /* non-finite box: reference's assert in _clip_box (frcnn.py:148) -> AssertionError */
#define VK_EWEIGHTS 4    /* missing / mis-shaped weight (strict load, frcnn.py:1881)     -> OSError */
#define VK_EHIP 5        /* HIP runtime failure                                          -> RuntimeError */
#define VK_ENOMEM 6

typedef enum { VK_F32 = 0, VK_F16 = 1, VK_I64 = 2, VK_I32 = 3, VK_BF16 = 4 } vk_dtype;
/* epilogue activation of vk_conv2d / vk_linear (the `relu` argument): */
typedef enum { VK_ACT_NONE = 0, VK_ACT_RELU = 1, VK_ACT_GELU = 2 /* erf form */, VK_ACT_TANH = 3 } vk_act;

#define VK_MAX_ANCHOR_DIM 8
#define VK_MAX_NMS_THRESH 8

/* The config keys the reference model reads (frcnn.py:200-223,
 * 1230-1237, 1312-1336, 1414-1417, 1537, 1583-1607). */
typedef struct vk_config {
    int32_t depth;                 /* RESNETS.DEPTH 50|101|152 */
    int32_t num_groups;            /* RESNETS.NUM_GROUPS (frcnn.py:217; > 1: ResNeXt, width_per_group a power of two) */
    int32_t width_per_group;       /* RESNETS.WIDTH_PER_GROUP */
    int32_t stem_out_channels;     /* RESNETS.STEM_OUT_CHANNELS */
    int32_t res2_out_channels;     /* RESNETS.RES2_OUT_CHANNELS */
    int32_t stride_in_1x1;         /* RESNETS.STRIDE_IN_1X1 */
    int32_t caffe_maxpool;         /* MODEL.MAX_POOL */
    int32_t num_sizes;             /* ANCHOR_GENERATOR.SIZES[0] */
    float   sizes[VK_MAX_ANCHOR_DIM];
    int32_t num_ratios;            /* ANCHOR_GENERATOR.ASPECT_RATIOS[0] */
    float   ratios[VK_MAX_ANCHOR_DIM];
    float   anchor_offset;         /* ANCHOR_GENERATOR.OFFSET */
    int32_t rpn_hidden_channels;   /* PROPOSAL_GENERATOR.HIDDEN_CHANNELS (-1 = same as res4) */
    float   rpn_min_size;          /* PROPOSAL_GENERATOR.MIN_SIZE */
    double  rpn_nms_thresh;        /* RPN.NMS_THRESH */
    int32_t pre_nms_topk;          /* RPN.PRE_NMS_TOPK_TEST  (<= 8192) */
    int32_t post_nms_topk;         /* RPN.POST_NMS_TOPK_TEST (<= 1024) */
    float   rpn_bbox_weights[4];   /* RPN.BBOX_REG_WEIGHTS */
    int32_t num_classes;           /* ROI_HEADS.NUM_CLASSES */
    int32_t num_attrs;             /* ROI_BOX_HEAD.NUM_ATTRS */
    int32_t use_attr;              /* ROI_BOX_HEAD.ATTR */
    int32_t pooler_resolution;     /* ROI_BOX_HEAD.POOLER_RESOLUTION */
    int32_t res5_halve;            /* ROI_BOX_HEAD.RES5HALVE (1: the plain stride-2 Res5 stage, 7x7 maps) */
    int32_t cls_agnostic_bbox_reg; /* ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG */
    float   roi_bbox_weights[4];   /* ROI_BOX_HEAD.BBOX_REG_WEIGHTS */
    int32_t precision;             /* VK_F16: fp16 storage / fp32 accumulate (fast);
                                      VK_F32: fp32 storage, exact-f32 MFMA (strict parity mode) */
} vk_config;

/* Per-call knobs = the mutable attributes of the reference's model.roi_outputs
 * (frcnn.py:1229-1240; set by callers, tests/frcnn_test.py:16-19). */
typedef struct vk_roi_params {
    int32_t num_nms_thresh;
    double  nms_thresh[VK_MAX_NMS_THRESH];
    int32_t min_detections;
    int32_t max_detections;
} vk_roi_params;

/* Selection mode of the detections (model.roi_outputs.selection) and its knobs.
 * VK_SELECT_CLASS_MAX: the reference's ROIOutputs.inference (class-max NMS over the threshold list); score_thresh is
 *   accepted and unused, as upstream (do_nms frcnn.py:116 never reads it).
 * VK_SELECT_PER_CLASS: NMS per class at roi.nms_thresh[0] (roi.num_nms_thresh must be 1), a box's confidence = its best
 *   class that survives NMS (0 and class 0 when it survives in none; ties to the smaller class), ranked by confidence
 *   descending (ties to the lower proposal row), the first min(max(#{(double)confidence >= score_thresh},
 *   min_detections), max_detections, proposals of the image) are the output.  0 <= score_thresh <= 1 and
 *   min_detections <= max_detections, else VK_EINVAL.  The contract in full: DESIGN.md section 15.
 * VK_SELECT_DETECTIONS: a detector's output (detectron2's fast_rcnn_inference_single_image).  Every (proposal, class) pair
 *   with (double)score > score_thresh (strict) is a candidate, NMS per class at roi.nms_thresh[0] (roi.num_nms_thresh must
 *   be 1) over the candidates, the survivors of all classes ranked by score descending, then lower proposal row, then
 *   lower class; the first min(#survivors, max_detections) are the output: a proposal may come out under several classes,
 *   and an image may yield nothing.  0 <= score_thresh <= 1, min_detections == 0 (the rule has no minimum count) and
 *   1 <= max_detections <= 1024 (it may exceed the proposals per image), else VK_EINVAL.  DESIGN.md section 18.
 *   VK_DETECTIONS_LDS_KEYS: an image with at most this many NMS survivors is ranked by a sort in LDS, one with more by a
 *   radix select over the survivors in global memory; the results do not depend on the path. */
#define VK_SELECT_CLASS_MAX 0
#define VK_SELECT_PER_CLASS 1
#define VK_SELECT_DETECTIONS 2
#define VK_DETECTIONS_LDS_KEYS 4096
typedef struct vk_select_params {
    int32_t       mode;
    double        score_thresh;
    vk_roi_params roi;
} vk_select_params;

/* Device output block of one forward (caller-allocated, fixed capacity D =
 * max_detections per image; rows >= preds_per_image[n] are zero).  Mirrors the
 * OrderedDict returned by FRCNN.inference (frcnn.py:1996-2004). */
typedef struct vk_outputs {
    int64_t *obj_ids;          /* [N, D]        */
    float   *obj_probs;        /* [N, D]        */
    int64_t *attr_ids;         /* [N, D]        */
    float   *attr_probs;       /* [N, D]        */
    float   *boxes;            /* [N, D, 4]     */
    int64_t *preds_per_image;  /* [N]           */
    float   *roi_features;     /* [N, D, 2048]  */
} vk_outputs;

/* ignorey: horizontal bands whose RPN proposals are removed or trimmed (find_top_rpn_proposals frcnn.py:328-366),
 * applied per image after the decode and before the clip.  `bands` holds [N][max_per_image][2] values (y0, y1) of
 * double (f64 = 1) or float (f64 = 0), ALREADY divided by scales_yx[n][1] (the reference's quirk: the x scale, on y);
 * image n uses its first counts[n] rows, in order.  0 <= counts[n] <= max_per_image <= VK_MAX_IGNOREY.  A NULL
 * vk_ignorey, or max_per_image == 0, means no bands: exactly the entry point without _ignorey.  For each band, with
 * g0, g1 the band and (y0, y1) a box's current rows, compared in the bands' dtype: g1 <= y1 && g0 >= y0 removes the
 * box; otherwise, unless y0 > g1 && y1 > g0, |g0 - y0| < |g1 - y1| sets y0 = trunc(g1) and |g1 - y1| < |g0 - y0|
 * sets y1 = trunc(g0).  A removed box keeps its candidate slot, flagged like a size-filtered one, and is not checked
 * for non-finite values. */
#define VK_MAX_IGNOREY 64
typedef struct vk_ignorey {
    const void    *bands;
    const int32_t *counts;
    int32_t        max_per_image;
    int32_t        f64;
} vk_ignorey;

typedef struct vk_handle vk_handle;

const char *vk_last_error(void);
int vk_version(void);

/* ---- model lifetime ------------------------------------------------------
 * vk_create        <- FRCNN.__init__            frcnn.py:1744-1755 (build_backbone :200-261,
 *                                               RPN :1580-1610, Res5ROIHeads :1312-1363)
 * vk_load_weights  <- load_state_dict, one call per state-dict tensor, reference key names
 *                                               frcnn.py:1862-1881
 * vk_finalize      <- model.eval() + BN folding / NHWC repack (frcnn.py:1920; Conv2d :794-822)
 * vk_destroy       <- Python GC
 * One process may hold handles on several devices (the device index of vk_create); the kernel launchers keep their state
 * (LDS limits, scratch pages, CU count) per device.
 */
int vk_create(const vk_config *cfg, int device, vk_handle **out);
int vk_load_weights(vk_handle *h, const char *name, const void *host_ptr,
                    const int64_t *shape, int ndim, vk_dtype dtype);
int vk_finalize(vk_handle *h);
int vk_destroy(vk_handle *h);

/* Tunables.  Results do not depend on any of them (bit for bit); a value out of range is VK_EINVAL.
 *   "head_chunk"               RoIs per Res5-head chunk, 0 = all RoIs in one pass (default 9600, VK_HEAD_CHUNK)
 *   "backbone_streams"         1..4: res3 / res4 as that many image groups on as many streams (default 2, VK_BACKBONE_STREAMS)
 *   "backbone_split_min_batch" ... from this batch size on (default 8)
 *   "head_streams"             1 or 2: each Res5 chunk as two half-chunks on two streams (default 1, VK_HEAD_STREAMS)
 *   "head_split_min_rois"      ... for chunks of at least this many RoIs (default 512)
 *   "forward_lanes"            1 or 2 (default 2, VK_FORWARD_LANES): with 2, forwards of one handle that are in flight
 *                              together (vk_forward_begin) alternate between two working sets and two internal streams and
 *                              run beside each other on the device; the second working set is allocated when two forwards
 *                              first overlap (if it does not fit, the handle stays with one).  1: one working set, every
 *                              forward on the caller's stream.  The per-launch and per-stage timers force 1 while they are on.
 *   "head_dedupe"              0 or 1 (default 1, VK_HEAD_DEDUPE): with 1, block 0 of the Res5 head pools each DISTINCT RoIPool
 *                              window of a chunk once and runs its conv1 once per distinct window (vk_roi_windows and the
 *                              entry points next to it); the dense [K,P,P,C] pooled tensor is then not written during the
 *                              forward (the stage "pooled" is built when it is asked for).  Taken per chunk in the f16 mode,
 *                              with stride-1 Res5 and "head_streams" = 1, where both 1x1 GEMMs of block 0 run as
 *                              VK_ROUTE_GEMM4; every other chunk takes the plain path.
 *   "head_dedupe_taps"         0 or 1 (default 1, VK_HEAD_DEDUPE_TAPS): with 1, a chunk on the "head_dedupe" path whose conv2 reads
 *                              through the index goes on over its distinct nine-window NEIGHBOURHOODS (vk_roi_neighbourhoods):
 *                              block 0's conv3 + shortcut GEMM and conv1 of block 1 run once per neighbourhood, conv2 and conv3
 *                              of block 1 read those rows through the index.  Taken where Res5 has three blocks or more and
 *                              block 1's layers run as VK_ROUTE_GEMM4 / the indexed VK_ROUTE_PANEL form / VK_ROUTE_WS at K = 512;
 *                              every other chunk runs what "head_dedupe" alone runs.
 * The environment variables are read by vk_create.  vk_option_check validates a value without a handle and
 * vk_option_default gives the value a new handle starts with (the variable, where it holds a valid value); both are host only.
 * vk_get_option reads an option back, and two read-only counters for tests and tools: "working_sets" (arenas the handle
 * holds: 0, 1 or 2), "lane_forwards" (forwards that ran on a stream of the handle's own since vk_create) and
 * "dedupe_chunks" (Res5 chunks that took the "head_dedupe" path since vk_create), "indexed_chunks" (those of them whose conv2 read
 * conv1's distinct rows through the index, without the row gather: vk_panel_phase_indexed), "tap_dedupe_chunks" (those of them
 * that took the "head_dedupe_taps" path), "out_indexed_chunks" (those of these whose conv2 of block 0 stored the distinct
 * neighbourhoods' rows itself, without the row gather behind it: vk_panel_out_indexed). */
int vk_set_option(vk_handle *h, const char *key, int value);
int vk_get_option(vk_handle *h, const char *key, int *value);
int vk_option_check(const char *key, int value);
int vk_option_default(const char *key, int *value);

/* The box pooler of the C4 head (ROI_BOX_HEAD.POOLER_TYPE / POOLER_SAMPLING_RATIO; spatial scale 1/16, resolution
 * POOLER_RESOLUTION).  VK_POOLER_ROIPOOL is the reference's (frcnn.py:1179) and what a new handle has; the two RoIAlign types
 * are detectron2's (torchvision roi_align semantics; PARITY UNPINNED for the rule, the reference holds no RoIAlign) and run
 * wherever the Res5 head runs: detection in every selection mode, ignorey, given boxes.  Not an option of the table above:
 * the pooler changes the results.  0 <= sampling_ratio <= 8 (0: adaptive, ceil(bin size)); it is kept and unused with
 * VK_POOLER_ROIPOOL.  With a RoIAlign pooler the "head_dedupe" path is never taken (distinct RoIPool windows mean nothing to
 * it) and the stage "head_windows" is not set.  The handle pools through vk_roi_align on one level (res4); the boxes that
 * reach it are finite and inside the image (the RPN's and vk_forward_boxes_begin's _clip_box), a non-finite box having
 * been flagged before.
 * vk_pooler_check validates a pair without a handle; vk_set_pooler is legal only before the handle's first forward
 * (VK_EINVAL after: the working set is planned for the pooler). */
#define VK_POOLER_ROIPOOL    0
#define VK_POOLER_ROIALIGN   1   /* aligned = 0 */
#define VK_POOLER_ROIALIGNV2 2   /* aligned = 1 */
int vk_pooler_check(int type, int sampling_ratio);
int vk_set_pooler(vk_handle *h, int type, int sampling_ratio);
int vk_get_pooler(vk_handle *h, int *type, int *sampling_ratio);

/* Number of weight tensors the model expects and their names (strict load). */
int vk_num_weights(vk_handle *h, int *count);
int vk_weight_name(vk_handle *h, int index, const char **name);

/* ---- the forward pass ----------------------------------------------------
 * vk_forward <- FRCNN.forward / inference   frcnn.py:1924-2004
 *   images_dev : [N,3,H,W] f32 NCHW, already resized / mean-subtracted / zero-padded
 *   image_hw   : host [N,2] int32 (h, w) of the un-padded content   (image_shapes)
 *   scales_yx  : host [N,2] f32 or NULL                              (frcnn.py:1280-1283)
 * Asynchronous on `stream` except for one small device->host read of the
 * non-finite flag at the end (the reference asserts on host, frcnn.py:148).
 */
int vk_forward(vk_handle *h, const float *images_dev, int N, int H, int W,
               const int32_t *image_hw, const float *scales_yx,
               const vk_roi_params *rp, const vk_outputs *out_dev, void *stream);

/* The same forward in two halves, so that a caller can enqueue the next batch before the previous one has finished
 * (the reference's loop is strictly serial, abc/extraction.py:189-213; on the GPU that leaves the device idle while the
 * host formats one batch and launches the next).  vk_forward_begin enqueues everything on `stream` and returns a
 * ticket; vk_forward_end(ticket) waits for that forward only, and raises the non-finite assertion (frcnn.py:148).
 * Tickets must be ended in order; at most 4 may be open.  `image_hw` / `scales_yx` are consumed before _begin returns.
 * With "forward_lanes" = 2 (the default) a forward that begins while another is open runs on a stream of the handle's
 * own, in the working set the open one does not use: it starts once everything enqueued on `stream` before _begin has
 * finished (inputs ready), and vk_forward_end makes `stream` wait for the ticket's completion before it returns, so
 * work enqueued on `stream` after _end sees the outputs.  Until _end of its ticket, `images_dev`, the given boxes and
 * the out_dev buffers belong to that forward: they must not be written, freed or reused (for another ticket or
 * anything else), not even by work enqueued on `stream` after _begin, which no longer orders behind the forward; and
 * `stream` must stay alive.  Pass the same stream to every _begin.  vk_forward == begin + end. */
int vk_forward_begin(vk_handle *h, const float *images_dev, int N, int H, int W,
                     const int32_t *image_hw, const float *scales_yx,
                     const vk_roi_params *rp, const vk_outputs *out_dev, void *stream, int64_t *ticket);
int vk_forward_end(vk_handle *h, int64_t ticket);
/* vk_forward_begin with ignorey bands (see vk_ignorey; NULL = vk_forward_begin).  bands and counts are HOST arrays,
 * copied into the ticket's slot before the call returns, like image_hw; every band must be finite with |value| < 2^31.
 * The reference applies bands only when scales_yx is given (frcnn.py:328): with scales_yx NULL the bands are ignored. */
int vk_forward_begin_ignorey(vk_handle *h, const float *images_dev, int N, int H, int W,
                             const int32_t *image_hw, const float *scales_yx,
                             const vk_roi_params *rp, const vk_outputs *out_dev, void *stream, int64_t *ticket,
                             const vk_ignorey *ignorey);
/* The detection forward with a selection mode (see vk_select_params); ignorey as above, NULL for none.  VK_SELECT_CLASS_MAX
 * is exactly the entry point above on sp->roi.  VK_SELECT_PER_CLASS computes, after the box head, the soft-max of every class
 * (stage "obj_scores" [K, ld] f32, K = N * POST_NMS_TOPK_TEST; the first C+1 columns of a row), bbox_pred over all 4C rows
 * through the linear path in the predictor's precision (stage "box_deltas" [K, ld] f32, class c at columns 4c..4c+3; the 4
 * columns of the one box with CLS_AGNOSTIC_BBOX_REG), then the selection (stages "max_conf" [N, R] f32, "attr_prob" [K] and "keep_ids");
 * "chosen_deltas" is not produced.  A non-finite box of ANY class raises the reference's assertion from vk_forward_end
 * (_clip_box runs on all R*C boxes, do_nms frcnn.py:121).  Its scores, deltas and confidences live in an arena of their own,
 * taken on the first per-class forward (K * (5C + 4) floats: 0.31 GB at 32 x 300 x 1600) and never by the other mode.
 * VK_SELECT_DETECTIONS computes the same "obj_scores" and "box_deltas", then the detector-style selection; its stages are
 * "obj_scores", "box_deltas", "attr_prob", "keep_ids" [N, max_detections] i64 (the proposal row of each output row) and
 * "n_survivors" [N] i32; max_detections may exceed POST_NMS_TOPK_TEST (at most 1024) and min_detections must be 0.  The
 * non-finite rule is the per-class mode's.  Its arena is a third allocation, taken on the first forward in this mode and by
 * no other: about K * (5C + 2) floats + N * R * C * 10 bytes (0.46 GB at 32 x 300 x 1600), DESIGN.md section 18. */
int vk_forward_begin_select(vk_handle *h, const float *images_dev, int N, int H, int W,
                            const int32_t *image_hw, const float *scales_yx,
                            const vk_select_params *sp, const vk_outputs *out_dev, void *stream, int64_t *ticket,
                            const vk_ignorey *ignorey);

/* Region features for caller-supplied boxes (the reference's `proposals=` slot, frcnn.py:1924-1964, which is broken
 * upstream: `proposal_boxes` is never bound when proposals are given).  Detection, but with the RPN replaced by the
 * caller's boxes, each kept in input order and none dropped:
 *   boxes_dev : [N,B,4] f32 (x0,y0,x1,y1), device; rows b >= counts[n] are ignored.  0 <= counts[n] <= B <= 1024.
 *   counts    : host [N] int32, copied into the ticket's pinned slot before this call returns (like image_hw).
 *   out_dev   : vk_outputs of capacity B per image.
 * Coordinates are in the frame of the returned boxes: network-input pixels without scales_yx; with scales_yx
 * original-image pixels, divided on the device (fp32 IEEE division) by scales_yx[n][1] (x) and scales_yx[n][0] (y) --
 * the inverse of frcnn.py:1280-1283.  Per box: _clip_box to image_hw[n] (frcnn.py:147-153; a non-finite box raises its
 * assertion from vk_forward_end, :148), RoIPool 14x14 at 1/16 on res4, the Res5 head and the spatial mean
 * (roi_features, :1391-1403), cls_score -> soft-max over C+1, obj_probs / obj_ids = max / arg-max over the first C
 * (do_nms :117-127), the attribute branch on that class (attr_probs / attr_ids as _predict_attrs :1257-1260).  boxes out =
 * the clipped box times the scales; no box regression, no NMS; preds_per_image[n] = counts[n].
 * The ticket belongs to vk_forward_begin's ring and is finished with vk_forward_end; detection and given-box forwards
 * may be in flight together, in order.  B == 0: every image is empty, preds_per_image is zeroed and nothing else runs.
 * Stages of the last forward: "res4", "proposal_boxes" [N,B,4] (clipped, network pixels), "proposal_counts",
 * "pooled", "feature_pooled", "obj_logits", "attr_logits"; the RPN's and the regression's are not produced. */
int vk_forward_boxes_begin(vk_handle *h, const float *images_dev, int N, int H, int W,
                           const int32_t *image_hw, const float *scales_yx,
                           const float *boxes_dev, int B, const int32_t *counts,
                           const vk_outputs *out_dev, void *stream, int64_t *ticket);

/* The two ends of vk_forward_boxes_begin as stage-level calls, for a binding that composes the forward itself (the FPN
 * detector, vltk_amd/frcnn_fpn.py).  Every array is a device array; nothing is copied to or from the host.
 * vk_given_boxes_ingest: boxes [N,B,4] f32 (rows b >= counts[n] ignored), counts [N] i32, image_hw [N,2] i32, scales_yx
 *   [N,2] f32 or NULL -> divide by the scales, flag a non-finite box (atomic OR of 1 into *nonfinite, which the caller
 *   zeroes), _clip_box to image_hw (frcnn.py:147-153) -> prop_boxes [N,B,4], rois [N*B,5] (batch, x0, y0, x1, y1; padding
 *   rows zero-size at the origin), and with levels != NULL each row's level [N*B] i32 by assign_boxes_to_levels
 *   (frcnn.py:444-460, bit-equal to vk_assign_levels on the same rois).  N >= 1, 1 <= B <= 1024.
 * vk_given_box_outputs: vk_outputs of capacity B per image from the per-row predictions [N*B] (obj_prob / obj_cls of the
 *   soft-max over C+1 and arg-max over C, attr_prob / attr_cls), prop_boxes times the scales, and feat [N*B, F] f32 rows;
 *   rows b >= counts[n] are zero, preds_per_image[n] = counts[n].  F a positive multiple of 4; feat and roi_features
 *   16-byte aligned. */
int vk_given_boxes_ingest(const float *boxes_dev, const int32_t *counts_dev, const int32_t *image_hw_dev,
                          const float *scales_yx_dev, int N, int B, float *prop_boxes, float *rois, int32_t *levels,
                          int min_level, int max_level, float canonical_box_size, int canonical_level, int32_t *nonfinite,
                          void *stream);
int vk_given_box_outputs(const float *obj_prob, const int32_t *obj_cls, const float *attr_prob, const int32_t *attr_cls,
                         const float *prop_boxes, const int32_t *counts_dev, const float *scales_yx_dev, const float *feat,
                         int F, int N, int B, const vk_outputs *out_dev, void *stream);

/* Grid features (this project's mode, no counterpart in the reference): the backbone, then the Res5
 * stage ONCE over the whole res4 map (roi_heads.res5 run convolutionally, frcnn.py:1344-1355) -> M [N,Hm,Wm,F] (Hm x Wm =
 * res4's Hf x Wf, halved by block 0's stride under RES5HALVE; S = 16, or 32 then), average-pooled to a Gh x Gw grid over
 * each image's content, and the box predictor on every cell's row.  No RPN head, no proposals, no RoIPool, no NMS.
 * Per image n with (h, w) = image_hw[n], in integers: fh = min(Hm, max(1, (h + S - 1) / S)), fw likewise; cell (i, j) is
 * row i * Gw + j and covers map rows floor(i * fh / Gh) .. ceil((i + 1) * fh / Gh) (exclusive) and columns likewise from
 * fw, Gw (adaptive_avg_pool2d's bins; with fh < Gh neighbouring cells share a pixel).
 *   roi_features[n, row, c] = (float)(sum of (double)M[n, y, x, c] / (double)count), the sum taken in y-outer, x-inner order;
 *   boxes[n, row]           = (xs * S, ys * S, min(xe * S, w), min(ye * S, h)), times the scales as frcnn.py:1280-1283;
 *   obj_ids / obj_probs / attr_ids / attr_probs: the predictor on the row exactly as vk_forward_boxes_begin produces them;
 *   preds_per_image[n] = Gh * Gw.  out_dev: vk_outputs of capacity Gh * Gw per image.  1 <= Gh, Gw and Gh * Gw <= 1024.
 * The ticket belongs to vk_forward_begin's ring and is finished with vk_forward_end; grid, detection and given-box
 * forwards may be in flight together, in order.  The working set's Res5 buffers are sized for the whole map; a plan that
 * could not hold it is refused with VK_EINVAL before anything is enqueued.
 * Stages of the last forward: "res4", "grid_res5_0" / "grid_res5_1" (the first two Res5 blocks' outputs, [N,Hm,Wm,F]),
 * "grid_map" [N,Hm,Wm,F] (the third's; all in the handle's dtype), "feature_pooled" [N*G,F], "proposal_boxes" [N,G,4]
 * (the cell boxes in network pixels, BEFORE the scales), "obj_logits", "attr_logits". */
int vk_forward_grid_begin(vk_handle *h, const float *images_dev, int N, int H, int W,
                          const int32_t *image_hw, const float *scales_yx, int Gh, int Gw,
                          const vk_outputs *out_dev, void *stream, int64_t *ticket);

/* The pooling stage of vk_forward_grid_begin on its own, independent of a handle.  Every array is a device array.
 * map [N,Hm,Wm,C] NHWC in dt (VK_F16 or VK_F32); image_hw_dev [N,2] i32; scales_yx_dev [N,2] f32 or NULL (boxes in
 * network pixels); S: input pixels per map pixel; feat_out [N*Gh*Gw, ldf] f32 (ldf >= C); boxes_out [N,Gh*Gw,4] f32.
 * One workgroup per (cell, image); a lane owns 8 consecutive channels (16-byte loads) when C is a multiple of 8 and the
 * map is 16-byte aligned, single channels otherwise; fp64 sums in a fixed order, no atomics: a host restatement of the
 * rule above is bit-equal.  image_hw values below 1 or beyond the map are clamped into it (fh, fw in 1..Hm, 1..Wm). */
int vk_grid_pool(const void *map, int N, int Hm, int Wm, int C, vk_dtype dt, const int32_t *image_hw_dev,
                 const float *scales_yx_dev, int S, int Gh, int Gw, float *feat_out, int ldf, float *boxes_out,
                 void *stream);

/* Intermediate tensors of the last forward, for stage-level parity tests.
 * name in {"res4","rpn_out","proposal_boxes","proposal_logits",
 * "proposal_counts","pooled","feature_pooled","obj_logits","attr_logits","chosen_deltas","keep_ids"},
 * after a grid forward (vk_forward_grid_begin) {"grid_res5_0","grid_res5_1","grid_map"},
 * and, after a per-class forward (vk_forward_begin_select), {"obj_scores","box_deltas","max_conf","attr_prob"}
 * ("attr_prob" [K] f32: each row's attribute probability, what attr_probs gathers);
 * "rpn_out" is the fused RPN head output [N,Hf,Wf,ld]: columns [0,A) objectness, [A,5A) deltas.
 * Returns a device pointer owned by the handle (valid until the next forward),
 * its dtype and its shape (up to 4 dims). */
int vk_get_stage(vk_handle *h, const char *name, const void **dev_ptr,
                 vk_dtype *dtype, int64_t *shape, int *ndim);

/* device->device copy on `stream` (lets a binding copy a stage tensor into memory it owns). */
int vk_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);

/* timing of the last forward's stages (HIP events on the launch stream), ms:
 * [0] backbone [1] rpn head [2] proposals [3] roi pool+res5 head [4] predictor+outputs [5] total.
 * Only recorded when enabled (costs event records, no syncs in the timed path). */
int vk_enable_stage_timing(vk_handle *h, int enable);
int vk_get_stage_timing(vk_handle *h, float *ms6);

/* Per-kernel timing of the forward's convolution launches (HIP events on the launch stream around
 * every launch; read after the forward's own end-of-call synchronisation, accumulated until reset).
 * bucket 0: conv_mfma256_kernel (256x256 LDS-ring tile)          1: conv_mfma_kernel f16->f16 (128x{64,128} tile)
 * bucket 2: conv_mfma_kernel f16->f32 out (RPN heads, predictor)  3: f32 strict-mode convs / stem
 * bucket 4: conv3x3_panel_kernel (3x3, LDS-resident input panel)  5: conv_duo_kernel (1x1, 128x256 tile, two per CU)
 * bucket 6: any conv kernel launched in the two-stream section of the backbone (res3 / res4 half-batches): these launches
 *           overlap each other in time, so their summed durations exceed the wall time they took -- kept apart so that the
 *           buckets above hold only launches that had the GPU to themselves
 * bucket 7: conv3x3_blk_kernel (3x3 over narrow channel blocks: ResNeXt grouped conv2, dense 64 -> 64)
 * bucket 8: conv_ws_kernel (1x1, K <= 512, weight-stationary: a workgroup keeps its 256 x K weights in registers)
 * bucket 9: conv_mfma256_kernel<0, true> (the ring kernel's two-input build: conv3 + projection shortcut as one GEMM; its own
 *           symbol in a rocprofv3 trace)
 * bucket 10: conv_gemm4_kernel (1x1 with K >= 1024, one or two inputs: 256x256 tile, four waves of 128x128)
 * bucket 11: bneck64_kernel (a whole res2 BottleneckBlock as one kernel: conv1 -> 3x3 -> conv3 + shortcut, 64 bottleneck channels)
 * launches[12], ms[12], flops[12] (algorithmic 2*M*Cout*K of the launches), bytes[12] (algorithmic HBM bytes:
 * input + output (+ residual) + weights, each once). */
#define VK_NUM_KERNEL_BUCKETS 12
int vk_enable_kernel_timing(vk_handle *h, int enable);
int vk_get_kernel_timing(vk_handle *h, int64_t *launches, double *ms, double *flops, double *bytes, int reset);

/* ---- stage-level entry points (tests, micro-benchmarks) -------------------
 * All pointers are device pointers unless marked host.                      */

/* Packed-weight helpers (host side).  K is ordered (kh, kw, cin) and padded to
 * whole 128-byte K-tiles; rows are padded to a multiple of 128 output channels. */
size_t vk_packed_weight_bytes(int cout, int cin, int kh, int kw, int groups, vk_dtype dt);
int vk_packed_cout(int cout);
/* Grouped convolutions (ResNeXt, BottleneckBlock conv2 `groups=num_groups` frcnn.py:942-952) run as dense GEMMs over an
 * input-channel SLICE per 64-output-channel tile: slice = min(max(cin/groups, 64), cin) channels, weights
 * zero outside a channel's own group.  Needs cin == cout and cin/groups a power of two.  groups == 1: dense. */
int vk_conv_slice_channels(int cin, int groups);
/* w_oihw [cout,cin/groups,kh,kw] f32; bn = {gamma,beta,mean,var} each [cout] or NULL;
 * bias [cout] or NULL; outputs: packed weights (dtype dt) and f32 bias [vk_packed_cout]. */
int vk_pack_conv_weight(const float *w_oihw_host, const float *bn_host, const float *bias_host,
                        int cout, int cin, int kh, int kw, int groups, vk_dtype dt,
                        void *w_packed_host, float *bias_packed_host);

/* conv + folded-BN bias (+ residual) (+ ReLU)  <- Conv2d.forward frcnn.py:794-822,
 * BottleneckBlock.forward :963-979.  x [N,H,W,cin] (dt), residual/y [N*Ho*Wo, ldy].  `relu` is a vk_act; a value outside
 * 0..3 is VK_EINVAL before any launch (vk_conv_route answers the same).
 * What a launch writes (vk_linear too): rows 0 .. N*Ho*Wo - 1, columns 0 .. round_up(cout, 8) - 1 of y.  The columns
 * cout .. round_up(cout, 8) - 1 are PADS: they are written, with unspecified contents.  Columns from round_up(cout, 8) up to
 * ldy, rows past the last, and memory in front of y are left alone; rows of the residual past the last are not read into
 * any output. */
int vk_conv2d(const void *x, int N, int H, int W, int cin,
              const void *w_packed, const float *bias_packed, const void *residual,
              void *y, int cout, int ldy, int kh, int kw, int stride, int pad, int dil, int groups,
              int relu, vk_dtype dt, vk_dtype out_dt, void *stream);

/* Which kernel a convolution launch runs on, asked of the dispatcher itself (host only, touches no device): the launch
 * entry points below switch on the same function, under the same A/B environment switches, re-read per call.
 * Geometry as vk_conv2d (N, H, W: the input; Ho / Wo follow); flags in place of pointers: cin2 > 0 is the dual-source form
 * (vk_conv1x1_dual: N = H = 1, W = M), has_residual a residual pointer, fused_mean vk_conv1x1_meanpool (N images of
 * H x W = 1 x HW).  vk_linear is N = H = 1, W = M, cin = K, cout = N, relu = act.  Returns a VK_ROUTE_* or, where the launch
 * would refuse the layer, the negative of its VK_E* code.  Not askable: vk_stem's convolution (always the generic kernel's stem
 * form, or stem_pool.hip as one kernel) and the sub-form a kernel picks for itself (the panel kernel's 8 or 9 row tiles, the
 * weight-stationary kernel's wave count, the fused block's rows / tile form). */
#define VK_ROUTE_GENERIC 0   /* conv_mfma_kernel: im2col, 128 x {64,128} tile; f32 / f16 / bf16, grouped, stem form */
#define VK_ROUTE_RING 1      /* conv_mfma256_kernel: 256 x 256 LDS-ring tile */
#define VK_ROUTE_DUO 2       /* conv_duo_kernel: 1x1, 128 x 256 tile, two workgroups per CU (f16 / bf16) */
#define VK_ROUTE_WS 3        /* conv_ws_kernel: 1x1, K <= 512, weight-stationary */
#define VK_ROUTE_GEMM4 4     /* conv_gemm4_kernel: 1x1, K >= 1024, four waves of 128 x 128 */
#define VK_ROUTE_PANEL 5     /* conv3x3_panel_kernel: 3x3, LDS-resident input panel */
#define VK_ROUTE_BLK 6       /* conv3x3_blk_kernel: 3x3 over narrow channel blocks */
int vk_conv_route(int N, int H, int W, int cin, int cin2, int has_residual, int fused_mean, int cout, int ldy, int kh, int kw,
                  int stride, int pad, int dil, int groups, int relu, vk_dtype dt, vk_dtype out_dt);
/* How a VK_ROUTE_PANEL launch of N images of H x W with this dilation splits (host only; VK_PANEL_PHASE is re-read per call):
 * the number of leading images that run in the kernel's phase-interleaved form (whole groups of 16; dilation 2, even H, even
 * W <= 14), 0 = none.  The other N - that many images run in the plain form, in a second launch when both counts are non-zero.
 * The two forms give the same bits. */
int vk_panel_phase_images(int N, int H, int W, int dil);
/* The tile of that phase part (host only; VK_PANEL_TALL is re-read per call): 512 = 512 rows x 128 output channels per workgroup,
 * 256 = 256 x 256 under VK_PANEL_TALL=0, 0 = the launch has no phase part (vk_panel_phase_images == 0, or cout is not a multiple
 * of 256 and the layer is not a panel launch at all).  A remainder of fewer than 16 images keeps the plain form's tile.  The two
 * shapes give the same bits. */
int vk_panel_phase_tile_rows(int N, int H, int W, int dil, int cout);
/* The A-fragment schedule of that tile (host only; VK_PANEL_REUSE is re-read per call): 1 = the 512-row tile with the three taps of
 * a tap row sharing one window of fragment registers (66 instead of 108 LDS fragment reads per wave and channel stage), 0 = every
 * tap reads its own fragments (VK_PANEL_REUSE=0), or the launch has no 512-row phase tile (vk_panel_phase_tile_rows != 512).  The
 * two schedules issue the same matrix instructions on the same operands in the same order: the same bits. */
int vk_panel_phase_reuse(int N, int H, int W, int dil, int cout);
/* Whether that launch can read its input through a row index (vk_conv2d_rows; host only; VK_PANEL_INDEXED is re-read per call):
 * 1 = the WHOLE launch runs the 512-row fragment-window tile (vk_panel_phase_images == N and vk_panel_phase_reuse == 1), the one
 * form that takes an index; 0 = it does not (N is not a multiple of 16, the shape has no phase form, one of VK_PANEL_PHASE / TALL /
 * REUSE is 0), or VK_PANEL_INDEXED=0 keeps the gather + dense launch everywhere.  A row's bits do not depend on where its input
 * row lives: the indexed launch and vk_gather_rows + vk_conv2d give the same bits. */
int vk_panel_phase_indexed(int N, int H, int W, int dil, int cout);
/* Whether that launch can STORE its rows through an index (vk_conv2d_rows_out; host only; VK_PANEL_OUT_INDEXED is re-read per call):
 * 1 = the whole launch runs the 512-row fragment-window tile, as above; 0 = it does not, or VK_PANEL_OUT_INDEXED=0 keeps the dense
 * output + vk_gather_rows_dev everywhere.  It does not read VK_PANEL_INDEXED: the two indices are independent. */
int vk_panel_out_indexed(int N, int H, int W, int dil, int cout);

/* conv3 + projection shortcut of a stride-1 BottleneckBlock as ONE f16 GEMM (`out = conv3(t) ; out += shortcut(x)`,
 * frcnn.py:970-977): y[M,cout] = relu?([x1 | x2] . W^T + bias (+ residual)), W rows = [conv3 row (cin1) | shortcut row
 * (cin2)] as packed by vk_pack_conv_weight and concatenated per output channel, bias = the two folded biases
 * summed.  cout % 256 == 0, cin1 and cin2 multiples of 64 (whole 128-byte K-tiles of the packer). */
int vk_conv1x1_dual(const void *x1, int cin1, const void *x2, int cin2, long M,
                    const void *w_packed, const float *bias_packed, const void *residual,
                    void *y, int cout, int relu, void *stream);

/* A whole stride-1 BottleneckBlock with 64 bottleneck channels and 256 outputs (res2) as ONE f16 kernel
 * (BottleneckBlock.forward frcnn.py:963-979): y = relu(conv3(relu(conv2(relu(conv1 x)))) + shortcut(x)); the two 64-channel
 * intermediates stay in LDS (rounded to f16 there, as the layer-by-layer path rounds them in HBM), x is read once.
 * proj == 0: identity shortcut, cin == 256, w3 = conv3's packed rows [256][64].  proj != 0: projection shortcut of block 0,
 * cin == 64, w3 = [conv3 row | shortcut row] per output channel and b3 = the two folded biases summed (vk_conv1x1_dual's
 * layout).  w1 [>=64][cin], w2 [>=64][9*64] as vk_pack_conv_weight writes them.  x [N,H,W,cin], y [N,H,W,256];
 * N*H*W*512 < 2^32 - 2^20. */
int vk_bottleneck64(const void *x, int N, int H, int W, int cin, int proj,
                    const void *w1_packed, const float *b1_packed, const void *w2_packed, const float *b2_packed,
                    const void *w3_packed, const float *b3_packed, void *y, void *stream);

/* Host-only dispatch rules of a BottleneckBlock, asked by the C4 model and by callers that compose the backbone themselves
 * (the FPN detector, vltk_amd/frcnn_fpn.py), so that both run the same kernels for the same block.
 * vk_fuse_shortcut: 1 when conv3 (input cin channels) and a projection shortcut (input cin_shortcut channels) run as one
 * dual-source GEMM (vk_conv1x1_dual): f16, stride-1 block, cout % 256 == 0, both inputs multiples of 32 channels; 0 with
 * VK_NO_FUSED_SHORTCUT set.
 * vk_bottleneck64_eligible: 1 when the block runs as vk_bottleneck64 on its input [N,H,W,cin]: cmid bottleneck channels,
 * stride = conv1's times conv2's, conv2's dilation and groups, proj = a projection shortcut and fused_shortcut = that
 * vk_fuse_shortcut said yes for it; 0 with VK_BNECK_FUSED=0. */
int vk_fuse_shortcut(int cin, int cin_shortcut, int cout, int stride, vk_dtype dt);
int vk_bottleneck64_eligible(int cin, int cmid, int cout, int stride, int dil, int groups, int proj, int fused_shortcut,
                             long N, int H, int W, vk_dtype dt);

/* Last Res5 conv3 with the RoI's spatial mean folded into its epilogue (`res5(x).mean(dim=[2,3])`, frcnn.py:1401):
 * out_mean[n][c] = mean over the HW rows of image n of relu?(x . W^T + bias + residual), summed EXACTLY (integer
 * accumulation of the f16-rounded values) and rounded once, so it does not depend on how rows fall into tiles;
 * a non-finite value gives NaN.  The [N*HW, cout] tensor itself is never written.  f16, 128 <= HW <= 255,
 * cout % 256 == 0. */
size_t vk_conv1x1_meanpool_workspace_bytes(int N, int HW, int cout);
int vk_conv1x1_meanpool(const void *x, int N, int HW, int cin, const void *w_packed, const float *bias_packed,
                        const void *residual, int cout, int relu, float *out_mean,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- N3: LXMERT-style cross-modality encoder ops (transformers LxmertModel, the consumer the reference feeds:
 * vltk/legacy/legacy_train.py:30-39; restated from transformers/models/lxmert/modeling_lxmert.py v5.15) ---- */

/* nn.Linear (+ residual) (+ activation): y[M, ldy] = act(x[M,K] . W^T + bias + residual).  W packed by
 * vk_pack_conv_weight(w [N,K,1,1], NULL, bias, ...); K a whole number of 128-byte K-tiles; dt f32 | f16 | bf16.  The sum and
 * the activation are fp32 and the result is rounded once to out_dt (dt or f32).  act is a vk_act: outside 0..3 VK_EINVAL.
 * Written columns and pads: as vk_conv2d. */
int vk_linear(const void *x, long M, int K, const void *w_packed, const float *bias_packed, const void *residual,
              void *y, int N, int ldy, int act, vk_dtype dt, vk_dtype out_dt, void *stream);
/* y = scale * LayerNorm(x) (+ y when accumulate): LxmertAttentionOutput / LxmertOutput :269-342 (eps 1e-12),
 * LxmertVisualFeatureEncoder `(LN(a) + LN(b)) / 2` :468-476 as two calls with scale 0.5. */
int vk_layernorm(const void *x, int ldx, const float *gamma, const float *beta, void *y, int ldy, int M, int C,
                 float eps, float scale, int accumulate, vk_dtype dt, void *stream);
/* LxmertEmbeddings.forward :191-214: LayerNorm(word[ids] + position[arange(L)] + token_type[tt]); tables in dt.
 * The ids index the tables unchecked: keeping them inside the tables (and L inside `position`) is the caller's responsibility. */
int vk_embed_layernorm(const int64_t *input_ids, const int64_t *token_type_ids, int B, int L, const void *word,
                       const void *position, const void *token_type, const float *gamma, const float *beta,
                       void *y, int C, float eps, vk_dtype dt, void *stream);
/* LxmertAttention.forward :238-266 after the three projections: out[b, i, h*d:(h+1)*d] =
 * softmax_j(q_i . k_j / sqrt(d) + mask[b, j]) . v_j; q [B*Lq, ldq], k / v [B*Lk, ld*], heads side by side in a row.
 * Any Lq, Lk >= 1.  The kernel follows vk_attention_route: the matrix-core kernel (16-bit, d 32 / 64, Lq <= 48, Lk <= 64, rows
 * 16-byte aligned), else the LDS kernel where one head's Q, K, V and scores fit 160 KiB, else an online-soft-max kernel: the
 * tiled matrix-core form (16-bit, d 32 / 64, aligned) or the strict fp32 streaming form (d <= 256, VK_EINVAL beyond). */
int vk_attention(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask,
                 void *out, int ldo, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream);
/* The same function on the online-soft-max kernels at every shape, small ones included: the tiled matrix-core form where it is
 * eligible, else the streaming form (d <= 256).  With VK_ATTENTION_TILED=0 in the environment (re-read per call) it is
 * vk_attention.  The two matrix-core forms round the probabilities to dt before the second product; the LDS and streaming
 * forms do not. */
int vk_attention_tiled(const void *q, int ldq, const void *k, int ldk, const void *v, int ldv, const float *mask,
                       void *out, int ldo, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, void *stream);
/* Which kernel an attention launch runs on (host only, touches no device; both entry points switch on it, under the same
 * environment switches, re-read per call).  aligned16: q, k and v are 16-byte aligned; tiled_entry: 1 asks for
 * vk_attention_tiled, 0 for vk_attention.  VK_ATTENTION_MFMA=0 takes both matrix-core forms out of the choice.  Returns a
 * VK_ATT_ROUTE_* or, where the launch would refuse the call, the negative of its VK_E* code. */
#define VK_ATT_ROUTE_MFMA 0     /* attention_mfma_kernel: whole score matrix in registers */
#define VK_ATT_ROUTE_LDS 1      /* attention_kernel: one head in LDS, fp32 FMAs */
#define VK_ATT_ROUTE_TILED 2    /* attention_tiled_kernel: 64-key tiles on the matrix cores, online soft-max */
#define VK_ATT_ROUTE_STREAM 3   /* attention_stream_kernel: 64-key fp32 tiles in LDS, online soft-max */
int vk_attention_route(int Lq, int Lk, int d, vk_dtype dt, int ldq, int ldk, int ldv, int aligned16, int tiled_entry);

/* VisualBertEmbeddings.forward (transformers modeling_visual_bert.py v5.15 :72-168) for the single-stream encoder: one launch
 * writes y [B * (Lt + V), C], text rows first in each batch entry, with no concatenation in between:
 *   text row   (b, t)       LayerNorm(word[ids[b,t]] + token_type[tt[b,t]] + position[t])
 *   visual row (b, Lt + j)  LayerNorm(proj[b*V + j] + visual_token_type[vtt[b,j]] + visual_position[0] + mean_a position[align[b,j,a]])
 * proj [B*V, ldp] is visual_projection's output (vk_linear).  image_text_alignment [B, V, A] int32 (A <= 16, -1 pads; the mean
 * is over the valid entries, summed in order of a, and a box with none adds zero) or NULL with A = 0.  Tables, proj and y in dt;
 * sums, statistics and the affine in fp32.  C <= 2048; Lt <= max_position.  The kernel clamps every table index into its table;
 * refusing bad ids is the caller's. */
int vk_visualbert_embed(const int64_t *input_ids, const int64_t *token_type_ids, const int64_t *visual_token_type_ids,
                        const int32_t *image_text_alignment, int A, int B, int Lt, int V, const void *word, int vocab,
                        const void *position, int max_position, const void *token_type, const void *visual_token_type,
                        int type_vocab, const void *visual_position, const void *proj, int ldp, const float *gamma,
                        const float *beta, void *y, int C, float eps, vk_dtype dt, void *stream);

/* The embedding stage of a Vision Transformer (transformers modeling_vit.py v5.15: ViTPatchEmbeddings.forward :62-69,
 * ViTEmbeddings.forward :129-161) as two launches around one vk_linear.
 * vk_vit_patchify: pixel_values [B, C, Hi, Wi] fp32 NCHW -> rows [B * gh * gw, ldk] in dt (gh = Hi / P, gw = Wi / P).  Row
 * b*gh*gw + i*gw + j holds patch (i, j) in the order (c, py, px), the flattening of Conv2d(C, H, P, stride = P).weight.view(H, -1),
 * so the projection is vk_linear against that matrix; the columns C*P*P .. ldk - 1 (the GEMM's K-tile padding) are written as zero.
 * VK_EINVAL: B < 1, P < 1, C outside 1..4, Hi or Wi no positive multiple of P, ldk < C*P*P, rows that are no whole 16-byte chunks
 * (ldk * sizeof(dt) % 16, or a base that is not 16-byte aligned), 2^31 rows or more. */
int vk_vit_patchify(const float *pixel_values, int B, int C, int Hi, int Wi, int P, void *rows, int ldk, vk_dtype dt, void *stream);
/* vk_vit_assemble: x [B * (N + 1), H]; row b*(N+1) = cls_token + position[0], row b*(N+1) + 1 + n = proj[b*N + n] + position[1 + n].
 * proj [B*N, ldp] is the patch projection's output (bias added; its columns past H are never read), cls_token [H] and position
 * [N + 1, H] in dt; the sum is formed in fp32 and rounded once.  VK_EINVAL: B or N < 1, H < 1, ldp < H, 2^31 rows or more. */
int vk_vit_assemble(const void *proj, int ldp, const void *cls_token, const void *position, int B, int N, void *x, int H,
                    vk_dtype dt, void *stream);

/* ---- N5: LayoutLM (transformers modeling_layoutlm.py v5.15), the consumer of the reference's OCR word boxes ---- */

/* LayoutLMEmbeddings.forward :66-119 as one launch: out [B * L, C], row (b, t) =
 *   LayerNorm(word[ids] + position[t] + x[x0] + y[y0] + x[x1] + y[y1] + h[y1 - y0] + w[x1 - x0] + token_type[tt])
 * with bbox [B, L, 4] int32 (x0, y0, x1, y1).  The sum is formed in fp32 in exactly that order, the statistics and the affine are
 * fp32, the result is rounded to dt once.  word [vocab, C], position [max_position, C], x / y / h / w [max_2d, C] and token_type
 * [type_vocab, C] in dt.  The kernel clamps every index into its table (the two extents at 0 as well); refusing bad ids and boxes
 * is the caller's.  VK_EINVAL before any launch: a null pointer, B or L < 1, L > max_position, 2^31 rows or more, C outside
 * 1..2048, an empty table, a dtype other than f32 / f16 / bf16. */
int vk_layoutlm_embed(const int64_t *input_ids, const int64_t *token_type_ids, const int32_t *bbox, int B, int L, const void *word,
                      int vocab, const void *position, int max_position, const void *x, const void *y, const void *h,
                      const void *w, int max_2d, const void *token_type, int type_vocab, const float *gamma, const float *beta,
                      void *out, int C, float eps, vk_dtype dt, void *stream);
/* The token-classification tail (what vltk/utils/adapters.py map_ocr_predictions does per example on the host; PARITY UNPINNED
 * for the rule).  logits [B * L, ld] in dt, of which the first C columns count; word_ids [B, L]: the word a token belongs to, -1
 * for a special or padding token (an id >= W is ignored too).  token_labels [B, L]: the arg-max over C, scanning upward with
 * v > best from -inf at index 0 (ties give the lowest index, a NaN never wins, a row of NaN / -inf gives 0).  word_labels [B, W]:
 * the most frequent token label among the tokens of that word, which need not be contiguous; ties give the smallest label
 * (torch.mode's rule on the CPU); a word with no token gets -1.  1 <= C <= 64, 1 <= L <= 4096, 1 <= W <= L, ld >= C. */
int vk_token_word_labels(const void *logits, int ld, const int32_t *word_ids, int B, int L, int C, int W, int32_t *token_labels,
                         int32_t *word_labels, vk_dtype dt, void *stream);
/* The extractive-QA tail (PARITY UNPINNED for the rule: the reference has no span decode).  Element (b, t) of the start logits is
 * start_logits[(b * L + t) * start_stride] (dt), likewise the end logits, so the two columns of a [B * L, ld] GEMM output are read
 * in place.  context_mask [B, L]: non-zero where an answer token may lie.  Candidates are the pairs s <= e with both tokens in the
 * context and e - s + 1 <= max_answer_tokens; a pair scores float(start[s]) + float(end[e]); the best wins under score > best
 * from -inf, ties go to the smaller s, then the smaller e.  start / end [B] int32 and score [B] f32; (-1, -1, -inf) when nothing
 * wins.  1 <= L <= 4096, max_answer_tokens >= 1, strides >= 1. */
int vk_span_select(const void *start_logits, int start_stride, const void *end_logits, int end_stride, const int32_t *context_mask,
                   int B, int L, int max_answer_tokens, int32_t *start, int32_t *end, float *score, vk_dtype dt, void *stream);

/* ---- N6: the losses of LXMERT's pre-training heads (transformers LxmertForPreTraining.forward :1059-1095; csrc/losses.hip) ----
 * fp32 arithmetic on values read from dt (f32, f16 or bf16); no atomics, so the same input gives the same bits on every run. */
/* row_loss[m] = logsumexp(logits[m, :C]) - logits[m, labels[m]], the row maximum subtracted before the exponential; 0 where
 * labels[m] == ignore_index (the row is then not read).  `CrossEntropyLoss(reduction="none")`.  A label that is neither
 * ignore_index nor in [0, C) gives NaN and reads nothing: keeping labels in range is the caller's responsibility.
 * ignore_index < 0, ld >= C.  The kernel follows vk_cross_entropy_form. */
int vk_cross_entropy(const void *logits, int ld, int M, int C, const int64_t *labels, int ignore_index, float *row_loss,
                     vk_dtype dt, void *stream);
/* Which kernel a cross-entropy launch runs on (host only).  aligned16: `logits` is 16-byte aligned.  VEC where the rows are
 * 16-byte addressable (aligned16 and ld a multiple of 16 / sizeof(dt) elements) and C >= 128; SCALAR elsewhere.  Returns a
 * VK_CE_FORM_* or -VK_EINVAL where the launch would refuse the call. */
#define VK_CE_FORM_VEC 0        /* ce_vec_kernel: a 256-thread workgroup per row, 16-byte chunks, online max and sum */
#define VK_CE_FORM_SCALAR 1     /* ce_scalar_kernel: a wave per row, one element per lane and step */
int vk_cross_entropy_form(int C, int ld, vk_dtype dt, int aligned16);
/* row_loss[m] = mean over C of SmoothL1(pred[m, c] - target[m, c]) with beta = 1: `SmoothL1Loss(reduction="none")(..).mean(1)`.
 * pred [M, ld] in dt, target [M, ldt] f32. */
int vk_smooth_l1_rows(const void *pred, int ld, const float *target, int ldt, int M, int C, float *row_loss, vk_dtype dt,
                      void *stream);
/* One number from M row losses: an fp64 sum in a fixed order, rounded to f32 once after the division.
 * labels given (weight null): out = sum of row_loss over the rows with labels[m] != ignore_index / their count: `CrossEntropyLoss()`'s
 * mean, NaN when no row counts (scale unused).  labels null: out = scale * sum_m row_loss[m] * weight[m] / M (weight null: all
 * ones): `(loss * mask_conf).mean() * visual_loss_normalizer`. */
int vk_loss_reduce(const float *row_loss, const float *weight, const int64_t *labels, int ignore_index, int M, float scale,
                   float *out, void *stream);
/* out = the fp32 sum of the present terms in transformers' order.  terms [6]: masked-LM, matched, obj, attr, feat, answer; bit i
 * of `present` says that term i takes part: total = 0 + mlm + matched + (0 + obj + attr + feat) + answer. */
int vk_loss_total(const float *terms, int present, float *out, void *stream);

/* ---- N7: training an answer head over a frozen encoder (vltk/legacy/legacy_train.py; csrc/train.hip) ----
 * fp32 in memory; no atomics and no split-K: one writer and one summation order per output, the same bits on every run. */
/* C[M, N] = op(A) . op(B) (+ bias[N]) (+ C when accumulate), row-major fp32 with leading dimensions of their own.  transA 0: A is
 * [M, K] (lda >= K), 1: A is [K, M] (lda >= M); transB 0: B is [K, N] (ldb >= N), 1: B is [N, K] (ldb >= K), the layout of
 * nn.Linear's weight.  Y = X . W^T + b is (0, 1), dX = dY . W is (0, 0), dW = dY^T . X is (1, 0).  Any M, N, K >= 1; edges are
 * masked.  Each output element is one fmaf chain in ascending k on the fp32-input matrix instruction, started from
 * (accumulate ? C : 0) + bias: data whose sums stay below 2^24 is exact.  bias may be NULL. */
int vk_gemm_f32(const float *A, long lda, int transA, const float *B, long ldb, int transB, const float *bias, float *C, long ldc,
                int M, int N, int K, int accumulate, void *stream);
/* What the launch refuses, without a device: a size below 1, a flag that is neither 0 nor 1, a leading dimension below the row
 * width.  VK_OK or VK_EINVAL. */
int vk_gemm_f32_check(int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB);
/* out[c] = sum_m x[m, c]: fp64 adds in a fixed order, rounded to f32 once.  M > 256 runs in two stages through `workspace`
 * (8-byte aligned, the bytes the size function names; 0 bytes and NULL where M <= 256). */
size_t vk_col_sums_workspace_bytes(int M, int N);
int vk_col_sums(const float *x, long ld, int M, int N, float *out, void *workspace, size_t workspace_bytes, void *stream);
/* dlogits[m, :C] = (softmax(logits[m, :C]) - onehot(labels[m])) * scale, the row maximum subtracted before the exponential: the
 * gradient of `CrossEntropyLoss()` with scale = 1 / (rows whose label is not ignore_index).  Rows with that label are written as
 * zeros; a label that is neither it nor in [0, C) gives a row of NaN and reads nothing.  ignore_index < 0; ld, ldd >= C. */
int vk_cross_entropy_grad(const float *logits, long ld, int M, int C, const int64_t *labels, int ignore_index, float scale,
                          float *dlogits, long ldd, void *stream);
/* y = act(x) and dx = dy * act'(x) over n elements; act VK_ACT_GELU (erf form) or VK_ACT_TANH, anything else VK_EINVAL.  The
 * backward takes the pre-activation x, which the caller keeps.  fp64 arithmetic, one rounding at the store. */
int vk_act_f32(const float *x, float *y, long n, int act, void *stream);
int vk_act_grad_f32(const float *x, const float *dy, float *dx, long n, int act, void *stream);
/* The backward of y = gamma * (x - mean) / sqrt(var + eps) + beta over rows of C: dx [M, lddx], dgamma [C], dbeta [C] from x, gamma
 * and dy.  Mean and variance are recomputed from x; fp64 arithmetic, fixed-order column sums, one rounding at each store.
 * workspace: 8-byte aligned, the bytes the size function names. */
size_t vk_layernorm_grad_workspace_bytes(int M, int C);
int vk_layernorm_grad(const float *x, long ldx, const float *gamma, const float *dy, long lddy, float *dx, long lddx, float *dgamma,
                      float *dbeta, int M, int C, double eps, void *workspace, size_t workspace_bytes, void *stream);
/* One record of vk_adamw_step's table (device memory): n elements of a parameter, its gradient and its two moments, each
 * starting at any 4-byte boundary; decay != 0: the tensor takes weight decay. */
typedef struct {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t n;
    int32_t decay;
    int32_t reserved;
} vk_adamw_tensor;
/* torch.optim.AdamW's step over `count` tensors in one launch (max_n: the largest n of the table):
 * m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; p = p (1 - lr weight_decay) where the record decays;
 * p = p - lr / bias_correction1 * m / (sqrt(v) / sqrt(bias_correction2) + eps).  The caller computes bias_correction_i =
 * 1 - beta_i^step in fp64.  fp64 arithmetic on the fp32 values; m, v and p are rounded once each, at the store. */
int vk_adamw_step(const vk_adamw_tensor *table, int count, int64_t max_n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double bias_correction1, double bias_correction2, void *stream);
/* y = a + b over n dense fp32 elements, one rounding each; y may be a or b.  The residual adds of a trained layer: a residual
 * passed to vk_gemm_f32 through `accumulate` instead takes K roundings at the residual's magnitude, one per step of the chain. */
int vk_add_f32(const float *a, const float *b, float *y, long n, void *stream);
/* The backward of a row gather: dst [M, C] (dense rows, ld_dst == C) is cleared, then row idx[i] receives src[i], i < n.  The
 * indices must be distinct (one per example; the caller checks); one outside [0, M) is skipped. */
int vk_scatter_rows_f32(const float *src, long ld_src, const int32_t *idx, int n, float *dst, long ld_dst, int M, int C, void *stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) over the gradients of vk_adamw_step's table, without a host round trip:
 * fp64 sums of squares per (tensor, block) into `workspace` (8-byte aligned, the bytes the size function names), one workgroup
 * adds them in a fixed order and writes norm_coef[0] = the total norm and norm_coef[1] = min(1, max_norm / (norm + 1e-6)) (f32,
 * device memory), then every gradient is multiplied by norm_coef[1] as read from the device.  A non-finite norm propagates
 * (torch's error_if_nonfinite=False); a coefficient of 1 leaves every gradient's bits unchanged. */
size_t vk_grad_clip_workspace_bytes(int count);
int vk_grad_clip(const vk_adamw_tensor *table, int count, int64_t max_n, double max_norm, float *norm_coef, void *workspace,
                 size_t workspace_bytes, void *stream);
/* The backward of vk_attention in fp32: O = softmax(Q K^T / sqrt(d) + mask) V per (batch, head), head h in columns h d .. h d + d
 * of rows [B * L, ld]; q, dout, o, dq have B * Lq rows, k, v, dk, dv B * Lk rows, each matrix its own leading dimension (a packed
 * QKV projection passes 3 * heads * d three times).  mask [B, Lk] is additive, may be NULL and receives no gradient.  From what
 * the forward kept (q, k, v, o) and dout it writes dq = scale dS K, dk = scale dS^T Q, dv = P^T dout, with scale = 1 / sqrt(d),
 * s = (q . k) scale + mask, P = expf(s - m) * (1 / l) recomputed from a row maximum m and row sum l, D = sum_c dout o per row and
 * dS = P (dP - D).  1 <= d <= 128, any Lq, Lk >= 1, any 4-byte alignment.  Three launches (row statistics into `workspace`, dq,
 * dk and dv), no atomics: the same input gives the same bits.  vk_attention_grad_check: what the launch refuses, host only (no
 * pointer is read through): a NULL pointer other than mask, a size below 1, d outside 1..128, a leading dimension below
 * heads * d, a workspace below the size function's bytes. */
size_t vk_attention_grad_workspace_bytes(int B, int heads, int Lq);
int vk_attention_grad_check(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const float *mask, const float *o,
                            long ldo, const float *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk, const float *dv,
                            long lddv, int B, int heads, int Lq, int Lk, int d, const void *workspace, size_t workspace_bytes);
int vk_attention_grad(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const float *mask, const float *o,
                      long ldo, const float *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, int B,
                      int heads, int Lq, int Lk, int d, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mixed-precision fine-tuning: 16-bit operands on the matrix cores, fp32 accumulation ---- */

/* y[i] = x[i] rounded to dt (VK_BF16 or VK_F16, nearest even) over n dense elements, as the conversion instruction does it: Inf
 * stays Inf, NaN stays NaN, values below the target's normal range become its subnormals. */
int vk_cast_16(const float *x, void *y, long n, vk_dtype dt, void *stream);
/* vk_gemm_f32's contract on 16-bit operands: C [M, N] = op(A) . op(B) (+ bias), the same three forms, A and B in dt (VK_BF16 or
 * VK_F16), fp32 accumulation on v_mfma_f32_16x16x32, the fp32 bias (NULL: none) added in fp32, C written as fp32 (out_dt = VK_F32)
 * or with one rounding as dt (out_dt = dt).  Any M, N, K >= 1; edges are masked and nothing outside the matrices is read, padding
 * included.  A, B and C are 16-byte aligned and the leading dimensions of 16-bit matrices are multiples of 8 elements.  There is
 * no accumulate flag (a residual is vk_add_f32's).  No split-K, no atomics: the same input gives the same bits; integer data
 * whose sums stay below 2^24 is exact.  vk_gemm_16_check: what the launch refuses, host only (no pointer is read through): what
 * vk_gemm_f32_check refuses, a NULL or misaligned A, B or C, a dt that is not 16-bit, an out_dt that is neither VK_F32 nor dt, a
 * leading dimension of a 16-bit matrix that is no multiple of 8. */
int vk_gemm_16_check(const void *A, long lda, int transA, const void *B, long ldb, int transB, const void *C, long ldc, int M, int N, int K,
                     vk_dtype dt, vk_dtype out_dt);
int vk_gemm_16(const void *A, long lda, int transA, const void *B, long ldb, int transB, const float *bias, void *C, long ldc, int M, int N,
               int K, vk_dtype dt, vk_dtype out_dt, void *stream);
/* The backward of the forward vk_attention_tiled runs in dt (VK_BF16 or VK_F16): vk_attention_grad's arguments and layout with
 * q, k, v, o and dout in dt and dq, dk, dv in fp32.  Every product runs on the matrix cores with fp32 accumulation:
 * s = (q . k) scale + mask and the online row maximum m and row sum l over 64-key tiles in fp32, P = exp(s - m) (1 / l) (rounded to
 * dt for dv = P^T dout), D = sum_c dout o, dP = dout V^T, dS = P (dP - D) in fp32 (rounded to dt for dq = scale dS K and
 * dk = scale dS^T Q).  d is 32 or 64, any Lq, Lk >= 1; every matrix is 16-byte aligned with a leading dimension that is a multiple
 * of 8.  Two launches (statistics into `workspace` and dq; dk and dv), no atomics: the same input gives the same bits.
 * vk_attention_grad_16_check: what the launch refuses, host only: a NULL pointer other than mask, a dt that is not 16-bit, a size
 * below 1, d other than 32 or 64, a leading dimension below heads * d or no multiple of 8, a pointer that is not 16-byte
 * aligned, a workspace below the size function's bytes. */
size_t vk_attention_grad_16_workspace_bytes(int B, int heads, int Lq);
int vk_attention_grad_16_check(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o,
                               long ldo, const void *dout, long lddo, const float *dq, long lddq, const float *dk, long lddk,
                               const float *dv, long lddv, int B, int heads, int Lq, int Lk, int d, vk_dtype dt, const void *workspace,
                               size_t workspace_bytes);
int vk_attention_grad_16(const void *q, long ldq, const void *k, long ldk, const void *v, long ldv, const float *mask, const void *o, long ldo,
                         const void *dout, long lddo, float *dq, long lddq, float *dk, long lddk, float *dv, long lddv, int B, int heads,
                         int Lq, int Lk, int d, vk_dtype dt, void *workspace, size_t workspace_bytes, void *stream);

/* ---- N4: FPN-side ops (what north_star names; the reference holds only fragments, see oracle/fpn_oracle.py) ---- */

/* RoIAlign over a feature pyramid (torchvision roi_align semantics, `aligned` as detectron2's ROIAlignV2; the level loop of
 * ROIPooler.forward frcnn.py:1214-1222): maps[l] NHWC [N,Hs[l],Ws[l],C], rois [K,5] (batch,x1,y1,x2,y2), roi_levels [K]
 * (NULL when levels == 1), out [K,P,P,C].  PARITY UNPINNED (no RoIAlign in the reference). */
int vk_roi_align(const void *const *maps, const int32_t *Hs, const int32_t *Ws, const float *scales, int levels,
                 int N, int C, const float *rois, const int32_t *roi_levels, int K, int P, int sampling_ratio,
                 int aligned, void *out, vk_dtype dt, void *stream);
/* Which kernel a RoIAlign launch runs on (host only, touches no device).  SCALAR where C is not a whole number of 16-byte
 * chunks or C * sizeof(dt) / 16 > 256; else SEP where P <= 16, unless VK_ROIALIGN_TABLES (re-read per call) is set to a
 * text whose atoi is 0; VEC elsewhere.  The vector forms read maps and write `out` in 16-byte chunks: both must be
 * 16-byte aligned, which the entry does not check.  Returns a VK_RA_FORM_* or -VK_EINVAL where the launch would refuse
 * the call (C < 1, P < 1, a dtype that is not f32 / f16 / bf16). */
#define VK_RA_FORM_SEP 0        /* roi_align_sep_kernel: per-axis weight tables in LDS, each footprint pixel read once */
#define VK_RA_FORM_VEC 1        /* roi_align_vec_kernel: the per-sample loop, 16-byte lanes */
#define VK_RA_FORM_SCALAR 2     /* roi_align_kernel: a workgroup per (RoI, bin), one channel per lane and step */
int vk_roi_align_form(int C, int P, vk_dtype dt);
/* assign_boxes_to_levels frcnn.py:444-460: floor(canonical_level + log2(sqrt(area)/canonical_box_size + 1e-8)),
 * clamped to [min_level, max_level], minus min_level.  boxes [K, ld] (x1,y1,x2,y2 first). */
int vk_assign_levels(const float *boxes, int ld, int K, int min_level, int max_level, float canonical_box_size,
                     int canonical_level, int32_t *levels_out, void *stream);
/* FPN top-down step: y = lateral + nearest-2x(top) (detectron2 FPN; absent from the reference: unpinned). NHWC. */
int vk_upsample2x_add(const void *lateral, const void *top, void *y, int N, int H, int W, int Ht, int Wt, int C,
                      vk_dtype dt, void *stream);
/* LastLevelMaxPool frcnn.py:835-836: max_pool2d(kernel 1, stride 2) = every second pixel.  y [N,(H-1)/2+1,(W-1)/2+1,C] */
int vk_subsample2(const void *x, void *y, int N, int H, int W, int C, vk_dtype dt, void *stream);
/* the ReLU between LastLevelP6P7's convolutions frcnn.py:852-853 (p6 itself stays un-rectified); as torch.relu, NaN stays
 * NaN and -0.0 stays -0.0 */
int vk_relu_copy(const void *x, void *y, long n, vk_dtype dt, void *stream);

/* find_top_rpn_proposals frcnn.py:264-390 over SEVERAL levels (the reference's RPN class itself cannot run them: its
 * AnchorGenerator stacks per-level anchors of unequal length; the function and the per-level pieces can, which is how the
 * golden vectors are made): per level top pre_nms_topk of [N,Hl,Wl,A] logits (row stride ld), decode with that level's cell
 * anchors / stride, clip, size filter; concat level-major; batched NMS (torchvision form: boxes shifted by
 * level * (max coordinate + 1)); first post_nms_topk.  levels * pre_nms_topk <= 8192.  Outputs as vk_rpn_proposals. */
size_t vk_rpn_multilevel_workspace_bytes(int N, int levels, int pre_topk, int post_topk);
/* The two RPN entries with ignorey bands (see vk_ignorey; NULL = the entry without _ignorey): bands and counts are
 * DEVICE arrays here, read by the decode kernel; counts[n] above max_per_image is taken as max_per_image.  The
 * multi-level form gives every level of image n the same bands. */
int vk_rpn_proposals_multilevel_ignorey(const float *const *logits, const int32_t *ld_logits, const float *const *deltas,
                                        const int32_t *ld_deltas, int levels, int N, const int32_t *Hs, const int32_t *Ws,
                                        int A, const float *const *cell_anchors, const int32_t *strides, float offset,
                                        const int32_t *image_hw, const float *bbox_weights4_host, float min_size,
                                        double nms_thresh, int pre_topk, int post_topk, float *out_boxes,
                                        float *out_logits, int32_t *out_counts, int32_t *nonfinite_flag, void *workspace,
                                        size_t workspace_bytes, void *stream, const vk_ignorey *ignorey);
int vk_rpn_proposals_ignorey(const float *logits, int ld_logits, const float *deltas, int ld_deltas,
                             int N, int Hf, int Wf, int A, const float *cell_anchors, int stride, float offset,
                             const int32_t *image_hw, const float *bbox_weights4_host, float min_size,
                             double nms_thresh, int pre_topk, int post_topk,
                             float *out_boxes, float *out_logits, int32_t *out_counts, int32_t *nonfinite_flag,
                             void *workspace, size_t workspace_bytes, void *stream, const vk_ignorey *ignorey);
int vk_rpn_proposals_multilevel(const float *const *logits, const int32_t *ld_logits, const float *const *deltas,
                                const int32_t *ld_deltas, int levels, int N, const int32_t *Hs, const int32_t *Ws, int A,
                                const float *const *cell_anchors, const int32_t *strides, float offset,
                                const int32_t *image_hw, const float *bbox_weights4_host, float min_size,
                                double nms_thresh, int pre_topk, int post_topk, float *out_boxes, float *out_logits,
                                int32_t *out_counts, int32_t *nonfinite_flag, void *workspace, size_t workspace_bytes,
                                void *stream);

/* NCHW f32 -> NHWC (dt) and back (layout plumbing for tests). */
int vk_nchw_to_nhwc(const float *x, int N, int C, int H, int W, void *y, vk_dtype dt, void *stream);
int vk_nhwc_to_nchw(const void *x, int N, int C, int H, int W, float *y, vk_dtype dt, void *stream);

/* stem: 7x7 s2 p3 conv + BN + ReLU + max-pool  <- BasicStem.forward frcnn.py:872-879.
 * x NCHW f32 [N,3,H,W]; w_packed from vk_pack_stem_weight; y NHWC [N,Hp,Wp,cout]. */
size_t vk_packed_stem_bytes(int cout, vk_dtype dt);
int vk_pack_stem_weight(const float *w_oihw_host, const float *bn_host, int cout, vk_dtype dt,
                        void *w_packed_host, float *bias_packed_host);
int vk_stem(const float *x, int N, int H, int W, const void *w_packed, const float *bias_packed,
            int cout, int caffe_maxpool, void *y, vk_dtype dt, void *workspace, size_t workspace_bytes,
            void *stream);
size_t vk_stem_workspace_bytes(int N, int H, int W, int cout, vk_dtype dt);
void vk_stem_out_hw(int H, int W, int caffe_maxpool, int *Ho, int *Wo);

/* Image pre-processing  <- ResizeShortestEdge + Preprocess, vltk/legacy/processing.py:29-150:
 * per image bilinear resize (align_corners=False) of a float HWC (BGR 0-255) device image to new_hw, (x-mean)/std,
 * pad with pad_value to [N,3,Hmax,Wmax] f32 NCHW.  raw_dev_ptrs_host: host array of N device pointers;
 * raw_hw_host / new_hw_host: host [N,2] (h, w); the resize size rule itself is host logic (vltk_amd/preprocess.py).
 * Every image (a non-null pointer, sizes >= 1, new_hw within Hmax x Wmax) is validated before the first launch: VK_EINVAL
 * leaves the output untouched, whatever the image's index. */
int vk_preprocess(const float *const *raw_dev_ptrs_host, const int32_t *raw_hw_host, const int32_t *new_hw_host,
                  int N, int Hmax, int Wmax, const float *mean3_host, const float *std3_host, float pad_value,
                  float *out_nchw_dev, void *stream);

/* max-pool 3x3 s2 (ceil_mode pad 0, or pad 1)  <- frcnn.py:875-878 */
int vk_maxpool3x3s2(const void *x, int N, int H, int W, int C, int caffe, void *y, vk_dtype dt, void *stream);

/* RPN proposals  <- RPNOutputs.predict_* frcnn.py:748-781, find_top_rpn_proposals :264-390,
 * AnchorGenerator :1463-1510, Box2BoxTransform.apply_deltas :548-584, batched_nms (torchvision).
 *   logits [N,Hf,Wf,A] f32, deltas [N,Hf,Wf,4A] f32 (row stride ld_* elements),
 *   cell_anchors [A,4] f32, image_hw dev [N,2] i32.
 *   out_boxes [N,post,4], out_logits [N,post], out_counts [N] i32, nonfinite_flag [1] i32. */
size_t vk_rpn_workspace_bytes(int N, int HWA, int pre_topk);
int vk_rpn_proposals(const float *logits, int ld_logits, const float *deltas, int ld_deltas,
                     int N, int Hf, int Wf, int A, const float *cell_anchors, int stride, float offset,
                     const int32_t *image_hw, const float *bbox_weights4_host, float min_size,
                     double nms_thresh, int pre_topk, int post_topk,
                     float *out_boxes, float *out_logits, int32_t *out_counts, int32_t *nonfinite_flag,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Greedy NMS (torchvision.ops.nms semantics; frcnn.py:132): boxes [n,4], scores [n];
 * keep_out [n] i64 in score order, count_out [1] i32. */
int vk_nms(const float *boxes, const float *scores, int n, double thresh,
           int64_t *keep_out, int32_t *count_out, void *workspace, size_t workspace_bytes, void *stream);
size_t vk_nms_workspace_bytes(int n);

/* RoIPool (torchvision.ops.RoIPool; frcnn.py:1179,1198): feat [N,H,W,C] NHWC, rois [K,5] f32
 * -> out [K,P,P,C] NHWC. */
int vk_roi_pool(const void *feat, int N, int H, int W, int C, const float *rois, int K,
                float spatial_scale, int P, void *out, vk_dtype dt, void *stream);

/* The distinct RoIPool windows of K RoIs (rois [K,5] f32 as for vk_roi_pool, on N maps of H x W cells).  Bin (ph, pw) of RoI k
 * is row (k * P + ph) * P + pw; its window is the clamped cell range [y0, y1) x [x0, x1) that vk_roi_pool takes the maximum
 * over (an empty range is a window too: a row of zeros).  idx [K*P*P] i32: the id of each row's window; win [K*P*P][5] i32,
 * of which the first *u_dev rows are written: (image, y0, y1, x0, x1) of each id; u_dev [1] i32: the number of ids.  An id is
 * the rank of (image, y0, y1, x0, x1), compared in that order, among the windows present.  Nothing is read back to the host.
 * The workspace (vk_roi_windows_workspace_bytes, 16-byte aligned; 0 = the maps are too large for the table) holds one bit per
 * possible window. */
size_t vk_roi_windows_workspace_bytes(int N, int H, int W);
int vk_roi_windows(const float *rois, int K, int N, int H, int W, int P, float spatial_scale, int32_t *idx, int32_t *win,
                   int32_t *u_dev, void *workspace, size_t workspace_bytes, void *stream);
/* out [*u_dev][C] (f16): row i is what vk_roi_pool writes for every bin whose window is win[i], bit for bit.  max_u: the rows
 * `out` can hold (ids from max_u on are not written). */
int vk_roi_pool_windows(const void *feat, int N, int H, int W, int C, const int32_t *win, const int32_t *u_dev, int max_u,
                        void *out, vk_dtype dt, void *stream);
/* dst[row] = src[idx[row]] for rows of row_bytes bytes (a multiple of 16) */
int vk_gather_rows(const void *src, const int32_t *idx, long rows, int row_bytes, void *dst, void *stream);
/* ... for row < min(*rows_dev, rows): the row count lives on the device and `rows` bounds it (idx entries beyond it are not read).
 * rows_dev may be null (vk_gather_rows). */
int vk_gather_rows_dev(const void *src, const int32_t *idx, long rows, const int32_t *rows_dev, int row_bytes, void *dst, void *stream);
/* The distinct NINE-WINDOW NEIGHBOURHOODS of K RoIs of P x P bins, from the window ids idx [K*P*P] of vk_roi_windows.  The
 * neighbourhood of bin (k, i, j) is the nine ids at (i + {-dil, 0, dil}, j + {-dil, 0, dil}) of RoI k, a position outside the
 * P x P map counting as a value of its own: what a stride-1 3x3 convolution of dilation `dil` over rows that depend on the window
 * alone reads at that bin.  nid [K*P*P] i32: the id of each row's neighbourhood; rep [K*P*P] i32, of which the first *v_dev
 * entries are written: the smallest row with that id; idx_rep likewise: idx[rep[id]]; v_dev [1] i32: the number of ids.  Two
 * rows share an id exactly when their nine window ids are equal (compared in full; the hash inside only orders the probes).
 * Ids number the neighbourhoods in the order of their smallest rows, so rep is ascending and nothing depends on the order in
 * which the device runs anything.  Nothing is read back to the host.  The workspace (vk_roi_neighbourhoods_workspace_bytes,
 * 16-byte aligned; 0 = too many rows) holds two slots per row and one bit per row. */
size_t vk_roi_neighbourhoods_workspace_bytes(long rows);
int vk_roi_neighbourhoods(const int32_t *idx, int K, int P, int dil, int32_t *nid, int32_t *rep, int32_t *idx_rep, int32_t *v_dev,
                          void *workspace, size_t workspace_bytes, void *stream);
/* Where each dense row goes among the distinct neighbourhoods' rows: out_row[m] = nid[m] where rep[nid[m]] == m, -1 elsewhere
 * (nid, rep of vk_roi_neighbourhoods; `rows` = K*P*P entries each).  Every id of [0, V) appears exactly once and the non-negative
 * entries ascend with m.  vk_conv2d_rows_out stores through it. */
int vk_roi_out_rows(const int32_t *nid, const int32_t *rep, long rows, int32_t *out_row, void *stream);
/* The VK_ROUTE_GEMM4 kernel on de-duplicated rows (f16): y[m] = relu?([x1[m] | x2[x2_idx[m]]] . W^T + bias) for m < M', where
 * M' = min(*m_dev, M) when m_dev is given (M then only bounds the launch) and M otherwise.  x2 / x2_idx may be null (one input,
 * x2 [M,cin2] read by m).  Weights and bias as for vk_conv1x1_dual.  VK_EINVAL where vk_conv_route would not give
 * VK_ROUTE_GEMM4 for the layer at M rows, or, with two inputs, cin1 is not a multiple of 128 from 256 on.  A row's bits do not depend on its
 * position, on M' or on which of these forms computes it. */
int vk_conv1x1_rows(const void *x1, int cin1, const void *x2, int cin2, long M, const int32_t *m_dev, const int32_t *x2_idx,
                    const void *w_packed, const float *bias_packed, void *y, int cout, int relu, void *stream);
/* The VK_ROUTE_PANEL kernel on de-duplicated input rows (f16, 3x3, stride 1, pad == dil): vk_conv2d of the tensor whose row m is
 * x[x_idx[m]], m < N*H*W, without that tensor being written.  x is [x_rows, cin]; x_idx holds N*H*W entries, every one in
 * [0, x_rows): the index is a contract, the kernel does not check it.  residual / y [N*H*W, cout] go by m.  VK_EINVAL, before any
 * launch, where vk_panel_phase_indexed answers 0 for the launch, where the layer is not a VK_ROUTE_PANEL launch, or where
 * x_rows * cin * 2 reaches 2^32.  Same bits as vk_gather_rows + vk_conv2d. */
int vk_conv2d_rows(const void *x, long x_rows, const int32_t *x_idx, int N, int H, int W, int cin, const void *w_packed,
                   const float *bias_packed, const void *residual, void *y, int cout, int dil, int relu, void *stream);
/* The same launch storing its rows through an index: row m of the result goes to y[y_idx[m]] and is not stored where y_idx[m] is
 * outside [0, y_rows) (-1 by convention).  y is [y_rows, cout]; y_idx holds N*H*W entries, and no two entries inside [0, y_rows)
 * may be equal (two rows would race for one place).  x_idx may be null: x is then the dense [N*H*W, cin] tensor and x_rows is
 * not read.  No residual.  VK_EINVAL, before any launch, where vk_panel_out_indexed answers 0 for the launch (with x_idx: or
 * vk_panel_phase_indexed), with a residual, or with y_rows <= 0.  The rows stored have the bits vk_conv2d gives them. */
int vk_conv2d_rows_out(const void *x, long x_rows, const int32_t *x_idx, int N, int H, int W, int cin, const void *w_packed,
                       const float *bias_packed, const void *residual, void *y, long y_rows, const int32_t *y_idx, int cout, int dil,
                       int relu, void *stream);
/* The VK_ROUTE_WS kernel with a de-duplicated residual (f16, 1x1, K = 512): y[m] = relu?(x[m] . W^T + bias + residual[res_idx[m]]),
 * m < M, without the dense residual being written.  res_idx holds M entries, every one a row of `residual`: the index is a
 * contract, the kernel does not check it.  res_idx may be null (residual [M, cout] read by m: the plain build, same entry).
 * The kernel is launched whatever M is (the dispatcher sends it layers from 1024 rows on).  VK_EINVAL, before any launch, where
 * the layer is not one of that kernel's K = 512 build with two waves per SIMD (cin 512, cout a multiple of 256 that divides
 * 8192, VK_CONV_WS / VK_WS_WAVES not set against it).  Same bits as vk_gather_rows of the residual + the plain build. */
int vk_conv1x1_res_rows(const void *x, int cin, long M, const void *w_packed, const float *bias_packed, const void *residual,
                        const int32_t *res_idx, void *y, int cout, int relu, void *stream);

/* mean over the P*P positions of each RoI  <- frcnn.py:1401: x [K,S,C] (dt) -> out [K,C] f32 */
int vk_mean_pool(const void *x, int K, int S, int C, float *out, vk_dtype dt, void *stream);

/* Box2BoxTransform.apply_deltas (frcnn.py:548-584): deltas [M,4k], boxes [M,4] -> out [M,4k] */
int vk_box_decode(const float *deltas, const float *boxes, int M, int k, const float *weights4_host,
                  float *out, void *stream);

/* Pieces of the box head for callers that compose one themselves (the FPN detector, vltk_amd/frcnn_fpn.py):
 * vk_make_rois       <- convert_boxes_to_pooler_format frcnn.py:426-441: boxes [N,R,4] -> rois [N*R,5] (batch,x1,y1,x2,y2)
 * vk_softmax_argmax  <- ROIOutputs._predict_objs / _predict_attrs :1252-1260: per row soft-max over the first n_softmax
 *                       logits, max / arg-max of the probabilities over the first n_argmax; raw_argmax_out (optional) =
 *                       arg-max of the raw logits over n_softmax (`scores.max(-1)` incl. background, :1732)
 * vk_concat_embed    <- `cat([roi_features, cls_embedding(max_class)], -1)` :1733-1734: out[k] = [ (dt)features[k][0:F] |
 *                       emb[cls[k]][0:E] ]; E == 0: a plain f32 -> dt conversion of the features
 * vk_chosen_deltas   <- bbox_pred :1730 for the arg-max class only: out[k][j] = bias[r] + <x[k], w_rows[r]>,
 *                       r = 4 * cls[k] + j (class-specific) or j (agnostic); w_rows [4C or 4, F] in dt, unpadded rows */
int vk_make_rois(const float *boxes, int N, int R, float *rois, void *stream);
int vk_softmax_argmax(const float *logits, int ld, int K, int n_softmax, int n_argmax, float *prob_out,
                      int32_t *cls_out, int32_t *raw_argmax_out, void *stream);
int vk_concat_embed(const float *features, int F, const void *emb, int E, const int32_t *cls, int K, void *out,
                    vk_dtype dt, void *stream);
int vk_chosen_deltas(const void *x, int ldx, const void *w_rows, const float *bias, const int32_t *cls,
                     int cls_agnostic, int F, int K, float *out, vk_dtype dt, void *stream);

/* ROIOutputs.inference (frcnn.py:1262-1294) + do_nms (:116-143), per image:
 *   obj_logits [K,C+1] f32 (row stride ld_obj), attr_logits [K,A+1] f32 (ld_attr),
 *   box_deltas: either full [K,4C] (ld_box=4C, chosen_only=0) or only the arg-max class's
 *   4 deltas [K,4] (chosen_only=1), proposals [N,R,4] + counts [N], features [K,F] f32. */
int vk_roi_outputs(const float *obj_logits, int ld_obj, const float *attr_logits, int ld_attr,
                   const float *box_deltas, int ld_box, int chosen_only,
                   const float *proposals, const int32_t *counts, const float *features, int F,
                   int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                   const float *weights4_host, const vk_roi_params *rp, const vk_outputs *out,
                   int64_t *keep_ids_out, int32_t *nonfinite_flag, void *stream);

/* Per-class selection (VK_SELECT_PER_CLASS, see vk_select_params) as a stage-level call, independent of a handle, in the
 * manner of vk_roi_outputs; every array is a device array except weights4_host and sp.
 *   obj_scores [K, ld_scores] f32: class probabilities (non-negative; vk_class_probs of the logits), the first C columns used;
 *   attr_logits [K, ld_attr] f32 or NULL (attr_probs / attr_ids are then zero); box_deltas [K, ld_box] f32: class c at
 *   columns 4c..4c+3, or with cls_agnostic the one box at columns 0..3; proposals [N, R, 4] + counts [N]; features [K, F]
 *   f32 (F a multiple of 4, 16-byte aligned like out->roi_features); out of capacity sp->roi.max_detections per image;
 *   keep_ids_out [N, max_detections] i64 and max_conf_out [N, R] f32 are optional; *nonfinite_flag is OR-ed with 1 when a
 *   decoded box of any (row < counts[n], class) is not finite (the caller zeroes it).  1 <= R <= 1024, max_detections <= R.
 * Synchronises `stream` before it returns (its scratch is freed).
 * vk_class_probs: out[k][c] = soft-max(logits[k][0:n])[c] for c < n (ROIOutputs._predict_objs frcnn.py:1252-1255), in the
 * arithmetic of vk_softmax_argmax.
 * vk_class_boxes: out [N*R, C, 4] f32 = every (row, class) box exactly as the per-class NMS holds it (decode of box_deltas on
 * the proposals, _clip_box to image_hw); rows >= counts[n] are zero; *nonfinite_flag (optional) is OR-ed with 1 as above.  The
 * forward never materialises these; this is for callers and tests that want the device's own bits.  Does not synchronise. */
int vk_class_boxes(const float *box_deltas, int ld_box, int cls_agnostic, const float *proposals, const int32_t *counts,
                   int N, int R, int C, const int32_t *image_hw, const float *weights4_host, float *out,
                   int32_t *nonfinite_flag, void *stream);
int vk_class_probs(const float *logits, int ld, int K, int n, float *out, int ld_out, void *stream);
int vk_per_class_select(const float *obj_scores, int ld_scores, const float *attr_logits, int ld_attr,
                        const float *box_deltas, int ld_box, int cls_agnostic,
                        const float *proposals, const int32_t *counts, const float *features, int F,
                        int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                        const float *weights4_host, const vk_select_params *sp, const vk_outputs *out,
                        int64_t *keep_ids_out, float *max_conf_out, int32_t *nonfinite_flag, void *stream);

/* Detector-style selection (VK_SELECT_DETECTIONS, see vk_select_params and DESIGN.md section 18) as a stage-level call,
 * independent of a handle.  The arguments are vk_per_class_select's without max_conf_out, with these differences:
 * sp->mode must be VK_SELECT_DETECTIONS, sp->roi.min_detections 0 and 1 <= sp->roi.max_detections <= 1024 (it may exceed
 * R); C < 2^20; keep_ids_out [N, max_detections] i64 (optional) is the proposal row of each output row, so rows that share
 * a proposal can be seen; n_survivors_out [N] i32 (optional) is the image's count of (row, class) pairs that survive the
 * per-class NMS, before the cut to max_detections.  out->preds_per_image[n] = min(n_survivors, max_detections), possibly 0;
 * rows beyond it are zero.  *nonfinite_flag is OR-ed with 1 when a decoded box of any (row < counts[n], class) is not finite,
 * candidate or not.  Does not synchronise: its scratch (N * R * C * 10 bytes and small change) is taken from and returned to
 * the device's memory pool in stream order.
 * vk_detections_lds_keys() returns VK_DETECTIONS_LDS_KEYS of the library as built. */
int vk_detections_select(const float *obj_scores, int ld_scores, const float *attr_logits, int ld_attr,
                         const float *box_deltas, int ld_box, int cls_agnostic,
                         const float *proposals, const int32_t *counts, const float *features, int F,
                         int N, int R, int C, int A, const int32_t *image_hw, const float *scales_yx_dev,
                         const float *weights4_host, const vk_select_params *sp, const vk_outputs *out,
                         int64_t *keep_ids_out, int32_t *n_survivors_out, int32_t *nonfinite_flag, void *stream);
int vk_detections_lds_keys(void);

#ifdef __cplusplus
}
#endif
#endif /* VLTK_HIP_H */
