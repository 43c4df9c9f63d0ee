"""The FPN detector end to end: ResNet bottom-up (res2..res5) -> FPN neck -> one RPN head over P2..P6 -> multi-level
proposals -> RoIAlign 7x7 by level -> 2-FC box head -> the reference's box predictor / ROIOutputs.

What BASELINE.json's configs and north_star literally name ("ResNet-101-FPN", "RoIAlign").  The reference itself has
no FPN model: only `LastLevelMaxPool` :825-836, `assign_boxes_to_levels` :444-460, the level loop of
`ROIPooler.forward` :1200-1224 and `find_top_rpn_proposals` :264-390 exist, plus the level-agnostic `BottleneckBlock`,
`RPNHead`, `FastRCNNOutputLayers` (sized from `input_size`, :1699-1719) and `ROIOutputs`.  Those pieces are used with the
reference's semantics; the composition is detectron2's standard ResNet-FPN Faster R-CNN and is a build extension --
PARITY UNPINNED vs the reference end to end (oracle: oracle/fpn_oracle.py FPNDetectorOracle).

`vltk_amd.FRCNN(cfg)` returns this class when `cfg.RPN.IN_FEATURES` names several levels (`vltk_amd.config.fpn_config`).
Same call surface and outputs as the C4 model (roi_features are `ROI_BOX_HEAD.FC_DIM` wide).  The composition is host
logic (Python, as in the reference); every arithmetic step is a C-ABI call into libvltk_hip.so -- no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .config import CONFIG_NAME, WEIGHTS_NAME, Config          # noqa: F401
from .fpn import FPNNeck, MultiLevelRoIAlign
from .frcnn import FRCNN, SELECTIONS, PendingForward
from .layers import Conv, Linear, f32, stream
from .parallel import OutputBlock, output_spec
from .weights import BLOCKS_PER_STAGE, fpn_layer_spec


class _Bottleneck:
    """BottleneckBlock frcnn.py:903-979.  The library decides, as for the C4 model, whether a stride-1 projection shortcut
    is part of conv3's GEMM (`out = conv3(t); out += shortcut(x)` as one dual-source GEMM, vk_conv1x1_dual: vk_fuse_shortcut)
    and whether the whole block runs as one kernel (csrc/bneck_fused.hip, vk_bottleneck64: vk_bottleneck64_eligible)."""

    def __init__(self, model, sd, p, stride, groups, stride_in_1x1, dil=1):
        def conv(q, **kw):
            bn = [sd[f"{q}.norm.{s}"] for s in ("weight", "bias", "running_mean", "running_var")]
            return Conv(sd[q + ".weight"], model.precision, model.device, bn, **kw)
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)             # frcnn.py:932
        self.m, self.stride = model, stride
        self.conv1 = conv(p + ".conv1", stride=s1)
        self.conv2 = conv(p + ".conv2", stride=s3, pad=dil, dil=dil, groups=groups)
        self.conv3 = conv(p + ".conv3")
        self.shortcut, self.fused = None, None
        if (p + ".shortcut.weight") in sd:
            c3, sc = self.conv3, conv(p + ".shortcut", stride=stride)
            self.shortcut = sc
            if L.load().vk_fuse_shortcut(c3.cin, sc.cin, c3.cout, stride, model.dt):
                rows = c3.b.shape[0]                # per output channel [conv3 row | shortcut row]; the folded biases summed
                self.fused = (torch.cat([c3.w.view(rows, -1), sc.w.view(rows, -1)], 1).reshape(-1), c3.b + sc.b)

    def __call__(self, x):
        m, c1, c2, c3 = self.m, self.conv1, self.conv2, self.conv3
        N, H, W, cin = x.shape
        proj = self.shortcut is not None
        if L.load().vk_bottleneck64_eligible(cin, c1.cout, c3.cout, self.stride, c2.dil, c2.groups, int(proj),
                                            int(self.fused is not None), N, H, W, m.dt):
            w3, b3 = self.fused if proj else (c3.w, c3.b)
            y = torch.empty((N, H, W, 256), dtype=m.tdt, device=m.device)
            L.call("vk_bottleneck64", x.data_ptr(), N, H, W, cin, int(proj), c1.w.data_ptr(), c1.b.data_ptr(),
                   c2.w.data_ptr(), c2.b.data_ptr(), w3.data_ptr(), b3.data_ptr(), y.data_ptr(), stream(m.device))
            return y
        t = c2(c1(x, relu=True), relu=True)
        if self.fused is not None:
            y = torch.empty((N, H, W, c3.cout), dtype=m.tdt, device=m.device)
            L.call("vk_conv1x1_dual", t.data_ptr(), t.shape[3], x.data_ptr(), cin, N * H * W, self.fused[0].data_ptr(),
                   self.fused[1].data_ptr(), None, y.data_ptr(), c3.cout, 1, stream(m.device))
            return y
        return c3(t, relu=True, residual=self.shortcut(x) if proj else x)


class FRCNNFPN(FRCNN):
    STAGES = ("res2", "res3", "res4", "res5")
    given_boxes = True                   # forward(proposals=...): region features for caller-supplied boxes
    grid_features = False                # forward(grid=...) is the C4 model's: a ValueError here

    def __init__(self, cfg, precision=None, device=None):
        self._init_host(cfg, precision, device)
        self._stages = {}
        self._timing = None
        self.visual_dim = int(cfg.ROI_BOX_HEAD.FC_DIM)
        levels = len(cfg.RPN.IN_FEATURES)
        if levels * int(cfg.RPN.PRE_NMS_TOPK_TEST) > 8192 or int(cfg.RPN.POST_NMS_TOPK_TEST) > 1024:
            raise ValueError("levels * PRE_NMS_TOPK_TEST must be <= 8192 and POST_NMS_TOPK_TEST <= 1024")
        if len(cfg.ROI_HEADS.IN_FEATURES) != 4 or levels not in (4, 5):
            raise ValueError("the FPN detector pools from p2..p5 and proposes from p2..p5(+p6)")

    def expected_keys(self):
        keys = []
        for prefix, shape, kind in fpn_layer_spec(self.config):
            keys.append(prefix + ".weight")
            if kind.startswith("conv_bn"):
                keys += [prefix + ".norm." + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
            elif kind != "embedding":
                keys.append(prefix + ".bias")
        keys += [f"proposal_generator.anchor_generator.cell_anchors.{i}" for i in range(len(self.config.ANCHOR_GENERATOR.SIZES))]
        return keys

    def load_state_dict(self, state_dict, strict=True):
        """Strict load (frcnn.py:1862-1881) in detectron2's FPN key layout (weights.fpn_layer_spec), gamma/beta renamed."""
        if self._finalized:
            raise RuntimeError("weights were already loaded into this model")
        sd = {}
        for k, v in state_dict.items():
            k = k.replace("norm.gamma", "norm.weight").replace("norm.beta", "norm.bias")
            sd[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        want = self.expected_keys()
        missing = [k for k in want if k not in sd and not k.endswith("num_batches_tracked")]
        extra = [k for k in sd if k not in set(want)]
        if missing:
            raise OSError(f"missing key(s) in state_dict: {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        if extra:
            raise OSError(f"unexpected key(s) in state_dict: {extra[:5]}{' ...' if len(extra) > 5 else ''}")
        cfg, r, prec, dev = self.config, self.config.RESNETS, self.precision, self.device
        # stem (BasicStem frcnn.py:857-888)
        p = "backbone.bottom_up.stem.conv1"
        w = f32(sd[p + ".weight"])
        self.stem_c = w.shape[0]
        lib = L.load()
        wp = np.zeros(lib.vk_packed_stem_bytes(self.stem_c, self.dt), np.uint8)
        bp = np.zeros(lib.vk_packed_cout(self.stem_c), np.float32)
        bn = np.ascontiguousarray(np.concatenate([f32(sd[f"{p}.norm.{s}"]) for s in ("weight", "bias", "running_mean", "running_var")]))
        L.call("vk_pack_stem_weight", w.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p), self.stem_c, self.dt,
               wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
        self.stem_w, self.stem_b = torch.from_numpy(wp).to(dev), torch.from_numpy(bp).to(dev)
        # bottom-up stages (build_backbone frcnn.py:200-261 with res5 as a backbone stage)
        self.stages = []
        for si, name in enumerate(self.STAGES):
            blocks = []
            for b in range(BLOCKS_PER_STAGE[r.DEPTH][si]):
                stride = (1 if si == 0 else 2) if b == 0 else 1
                blocks.append(_Bottleneck(self, sd, f"backbone.bottom_up.{name}.{b}", stride, r.NUM_GROUPS, bool(r.STRIDE_IN_1X1)))
            self.stages.append(blocks)
        # neck (P6 only for the 5-level RPN: forward_async) and the RoIAlign pooler over P2..P5
        self.neck = FPNNeck([(sd[f"backbone.fpn_lateral{l}.weight"], sd[f"backbone.fpn_lateral{l}.bias"]) for l in (2, 3, 4, 5)],
                            [(sd[f"backbone.fpn_output{l}.weight"], sd[f"backbone.fpn_output{l}.bias"]) for l in (2, 3, 4, 5)], prec, dev)
        P, fc = int(cfg.ROI_BOX_HEAD.POOLER_RESOLUTION), int(cfg.FPN.OUT_CHANNELS)
        self.pooler = MultiLevelRoIAlign(P, (1 / 4, 1 / 8, 1 / 16, 1 / 32), int(cfg.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO),
                                         precision=prec, device=dev)
        # RPN head (RPNHead frcnn.py:1513-1572): 3x3 + ReLU, then [objectness | deltas] as one 1x1 GEMM with f32 output
        q = "proposal_generator.rpn_head."
        self.rpn_conv = Conv(sd[q + "conv.weight"], prec, dev, bias=sd[q + "conv.bias"], pad=1)
        self.A = int(sd[q + "objectness_logits.weight"].shape[0])
        self.rpn_out = Conv(np.concatenate([f32(sd[q + "objectness_logits.weight"]), f32(sd[q + "anchor_deltas.weight"])], 0), prec, dev,
                            bias=np.concatenate([f32(sd[q + "objectness_logits.bias"]), f32(sd[q + "anchor_deltas.bias"])], 0))
        self.cells = [torch.from_numpy(f32(sd[f"proposal_generator.anchor_generator.cell_anchors.{i}"])).to(dev)
                      for i in range(len(cfg.RPN.IN_FEATURES))]
        # box head: fc1 expects detectron2's (c, y, x) flatten; the pooled tensor here is [K, y, x, c]
        self.fcs = []
        for i in range(int(cfg.ROI_BOX_HEAD.NUM_FC)):
            w = f32(sd[f"roi_heads.box_head.fc{i + 1}.weight"])
            if i == 0:
                w = np.ascontiguousarray(w.reshape(w.shape[0], fc, P * P).transpose(0, 2, 1).reshape(w.shape[0], -1))
            self.fcs.append(Linear(w, sd[f"roi_heads.box_head.fc{i + 1}.bias"], prec, dev))
        # predictor (FastRCNNOutputLayers frcnn.py:1676-1740): fp32 in both modes, as in the C4 model (csrc/model.hip pdt)
        bp_ = "roi_heads.box_predictor."
        self.cls_score = Linear(sd[bp_ + "cls_score.weight"], sd[bp_ + "cls_score.bias"], "fp32", dev)
        self.bbox_w = torch.from_numpy(f32(sd[bp_ + "bbox_pred.weight"])).to(dev).contiguous()
        self.bbox_b = torch.from_numpy(f32(sd[bp_ + "bbox_pred.bias"])).to(dev)
        self.use_attr = bool(cfg.ROI_BOX_HEAD.ATTR)
        if not self.use_attr:
            raise NotImplementedError("ROI_BOX_HEAD.ATTR=false: the reference's Res5ROIHeads unpacks three outputs (frcnn.py:1400)")
        self.emb = torch.from_numpy(f32(sd[bp_ + "cls_embedding.weight"])).to(dev).contiguous()
        self.fc_attr = Linear(sd[bp_ + "fc_attr.weight"], sd[bp_ + "fc_attr.bias"], "fp32", dev)
        self.attr_score = Linear(sd[bp_ + "attr_score.weight"], sd[bp_ + "attr_score.bias"], "fp32", dev)
        self._finalized = True
        return self

    # ---- options / timing (the C4 model keeps these in the library; here they are host-side) ----
    def set_option(self, key, value):
        pass

    def enable_stage_timing(self, on=True):
        self._timing = {} if on else None

    def stage_timing_ms(self):
        t = self._timing or {}
        ev = t.get("ev")
        if not ev:
            return {}
        torch.cuda.synchronize(self.device)
        names = ("backbone", "neck", "rpn_head", "proposals", "box_head", "predictor_outputs")
        out = {n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)}
        out["total"] = ev[0].elapsed_time(ev[-1])
        return out

    def enable_kernel_timing(self, on=True):
        pass

    def kernel_timing(self, reset=False):
        return {}

    def get_stage(self, name):
        return self._stages[name]

    def _mark(self, evs):
        if evs is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            evs.append(e)

    # ---- forward ----
    def forward_async(self, images, image_shapes, gt_boxes=None, proposals=None, scales_yx=None, ignorey=None, grid=None):
        """Detection, or with `proposals` region features for exactly those boxes (FRCNN.forward).  The forward
        runs to its end here; the returned handle's wait() / wait_raw() only format / hand out the outputs.
        roi_outputs.selection = "per_class" and "detections" are the C4 model's: detection with either
        raises ValueError here, and so does grid=."""
        if grid is not None:                                                         # before anything is enqueued
            self._check_grid_args(grid, proposals, ignorey)
        if proposals is None:                                                        # before anything is enqueued
            sel = getattr(self.roi_outputs, "selection", "class_max")
            if sel in SELECTIONS and sel != "class_max":         # whatever its knobs hold: the mode itself is not here
                raise ValueError(f'roi_outputs.selection="{sel}" is not available on the FPN detector (C4 model only)')
            self.roi_outputs.select_params()                     # an unknown selection raises
        images, hw, sc, given, ig = self._prepare(images, image_shapes, proposals, scales_yx, ignorey)
        if given is not None and int(self.config.ROI_BOX_HEAD.FC_DIM) % 4:
            raise ValueError(f"given boxes need ROI_BOX_HEAD.FC_DIM a multiple of 4, got {int(self.config.ROI_BOX_HEAD.FC_DIM)}")
        if (hw < 1).any():
            raise ValueError("image_shapes must be positive")
        if given is not None:
            return self._forward_boxes(images, hw, *given, sc)
        N = images.shape[0]
        cfg, dev, s = self.config, self.device, stream(self.device)
        evs = [] if self._timing is not None else None
        st = self._stages = {}
        self._mark(evs)
        feats = self._bottom_up(images, st)
        self._mark(evs)
        pyr = self.neck(feats, p6=len(cfg.RPN.IN_FEATURES) == 5)
        st.update((f"p{i + 2}", p_) for i, p_ in enumerate(pyr))
        self._mark(evs)
        # ---- RPN head over every level ----
        A, nl = self.A, len(pyr)
        heads = [self.rpn_out(self.rpn_conv(p_, relu=True), out_f32=True) for p_ in pyr]          # [N,h,w,ld] f32: [0,A) obj, [A,5A) deltas
        for i, h_ in enumerate(heads):
            st[f"rpn_out{i + 2}"] = h_
        self._mark(evs)
        # ---- proposals (find_top_rpn_proposals frcnn.py:264-390 over the levels) ----
        R, pre = int(cfg.RPN.POST_NMS_TOPK_TEST), int(cfg.RPN.PRE_NMS_TOPK_TEST)
        ld = heads[0].shape[3]
        P_ = lambda ptrs: (C.c_void_p * nl)(*ptrs)                                             # noqa: E731
        I_ = lambda vs: (C.c_int32 * nl)(*[int(v) for v in vs])                                # noqa: E731
        hw_dev = torch.from_numpy(hw).to(dev)
        pb = torch.zeros((N, R, 4), dtype=torch.float32, device=dev)
        pl = torch.zeros((N, R), dtype=torch.float32, device=dev)
        pc = torch.zeros(N, dtype=torch.int32, device=dev)
        flag = torch.zeros(2, dtype=torch.int32, device=dev)
        nbw = L.load().vk_rpn_multilevel_workspace_bytes(N, nl, pre, R)
        wsp = torch.empty(nbw, dtype=torch.uint8, device=dev)
        wts = (C.c_float * 4)(*[float(v) for v in cfg.RPN.BBOX_REG_WEIGHTS])
        rpn_args = (P_([h_.data_ptr() for h_ in heads]), I_([ld] * nl),
                    P_([h_.data_ptr() + 4 * A for h_ in heads]), I_([ld] * nl), nl, N, I_([h_.shape[1] for h_ in heads]),
                    I_([h_.shape[2] for h_ in heads]), A, P_([c_.data_ptr() for c_ in self.cells]), I_([4 * 2 ** i for i in range(nl)]),
                    float(cfg.ANCHOR_GENERATOR.OFFSET), hw_dev.data_ptr(), wts, float(cfg.PROPOSAL_GENERATOR.MIN_SIZE),
                    float(cfg.RPN.NMS_THRESH), pre, R, pb.data_ptr(), pl.data_ptr(), pc.data_ptr(), flag.data_ptr(), wsp.data_ptr(), nbw, s)
        if ig is None:
            L.call("vk_rpn_proposals_multilevel", *rpn_args)
        else:                                      # device copies of the bands; kept in the stage map until the next forward
            st["ignorey_bands"], st["ignorey_counts"] = torch.from_numpy(ig[0]).to(dev), torch.from_numpy(ig[1]).to(dev)
            igs = L.vk_ignorey(st["ignorey_bands"].data_ptr(), st["ignorey_counts"].data_ptr(), ig[0].shape[1], int(ig[2]))
            L.call("vk_rpn_proposals_multilevel_ignorey", *rpn_args, C.byref(igs))
        st["proposal_boxes"], st["proposal_logits"], st["proposal_counts"] = pb, pl, pc
        self._mark(evs)
        # ---- box head: RoI rows, then RoIAlign by level and the FCs ----
        K = N * R
        rois = torch.empty((K, 5), dtype=torch.float32, device=dev)
        L.call("vk_make_rois", pb.data_ptr(), N, R, rois.data_ptr(), s)
        feat = self._box_head(pyr, rois, None, st)                                             # [K, FC_DIM] f32 = roi_features
        self._mark(evs)
        # ---- predictor (FastRCNNOutputLayers.forward :1726-1740) ----
        F_, Cn, At = feat.shape[1], int(cfg.ROI_HEADS.NUM_CLASSES), int(cfg.ROI_BOX_HEAD.NUM_ATTRS)
        cls_logits, obj_prob, obj_cls, attr_logits = self._predictor(feat, K, st)
        chosen = torch.empty((K, 4), dtype=torch.float32, device=dev)
        L.call("vk_chosen_deltas", feat.data_ptr(), F_, self.bbox_w.data_ptr(), self.bbox_b.data_ptr(), obj_cls.data_ptr(),
               int(bool(cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG)), F_, K, chosen.data_ptr(), L.VK_F32, s)
        st["chosen_deltas"] = chosen
        # ---- outputs (ROIOutputs.inference :1262-1294) ----
        rp = self.roi_outputs.params()
        bufs = OutputBlock(output_spec(N, rp.max_detections, F_), device=dev)
        bufs.flat.zero_()
        out = L.vk_outputs(*[bufs[k].data_ptr() for k in bufs])
        sc_dev = None
        if sc is not None:
            sc_dev = torch.from_numpy(sc).to(dev)
        keep = torch.zeros((N, rp.max_detections), dtype=torch.int64, device=dev)
        wts2 = (C.c_float * 4)(*[float(v) for v in cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS])
        L.call("vk_roi_outputs", cls_logits.data_ptr(), cls_logits.shape[1], attr_logits.data_ptr(), attr_logits.shape[1],
               chosen.data_ptr(), 4, 1, pb.data_ptr(), pc.data_ptr(), feat.data_ptr(), F_, N, R, Cn, At, hw_dev.data_ptr(),
               sc_dev.data_ptr() if sc_dev is not None else None, wts2, C.byref(rp), C.byref(out), keep.data_ptr(),
               flag.data_ptr() + 4, s)
        st["keep_ids"] = keep
        self._mark(evs)
        if evs is not None:
            self._timing["ev"] = evs
        if int(flag.cpu().sum()) != 0:
            raise AssertionError("Box tensor contains infinite or NaN!")          # frcnn.py:148
        self._last_padded = bufs
        return PendingForward.finished(self, bufs, hw)

    def _forward_boxes(self, images, hw, boxes, counts, sc):
        """Region features for caller-supplied boxes (FRCNN.forward's `proposals`): bottom-up -> neck (no P6) ->
        vk_given_boxes_ingest (scale, finite check, _clip_box, RoI rows and levels in one launch) -> RoIAlign -> FCs ->
        cls_score / soft-max -> attribute branch -> vk_given_box_outputs.  No RPN head, proposals, box regression or NMS."""
        cfg, dev = self.config, self.device
        N = images.shape[0]
        B, F_ = boxes.shape[1], (self.fcs[-1].nout + 7) // 8 * 8              # F_: the feature row width, as detection's
        bufs = OutputBlock(output_spec(N, B, F_), device=dev)
        st = self._stages = {}
        if B == 0:                                  # every image is empty: nothing to compute, no stage events
            bufs["preds_per_image"].zero_()
            if self._timing is not None:
                self._timing.pop("ev", None)
            self._last_padded = bufs
            return PendingForward.finished(self, bufs, hw, given_width=0)
        s = stream(dev)
        evs = [] if self._timing is not None else None
        # counts | image_hw | scales_yx: one host-to-device copy
        meta = np.zeros(N * (3 if sc is None else 5), dtype=np.int32)
        meta[:N], meta[N:3 * N] = counts, hw.reshape(-1)
        if sc is not None:
            meta[3 * N:] = sc.reshape(-1).view(np.int32)
        meta_dev = torch.from_numpy(meta).to(dev)
        cnt_dev, hw_dev = meta_dev[:N], meta_dev[N:3 * N]
        sc_ptr = meta_dev[3 * N:].data_ptr() if sc is not None else None
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._mark(evs)
        feats = self._bottom_up(images, st)
        self._mark(evs)
        pyr = self.neck(feats, p6=False)
        st.update((f"p{i + 2}", p_) for i, p_ in enumerate(pyr))
        self._mark(evs)
        self._mark(evs)                             # no RPN head
        # ---- the caller's boxes in place of the proposals: scale, finite check, _clip_box (frcnn.py:147-153), RoI rows, levels ----
        K = N * B
        pb = torch.empty((N, B, 4), dtype=torch.float32, device=dev)
        rois = torch.empty((K, 5), dtype=torch.float32, device=dev)
        lv = torch.empty(K, dtype=torch.int32, device=dev)
        L.call("vk_given_boxes_ingest", boxes.data_ptr(), cnt_dev.data_ptr(), hw_dev.data_ptr(), sc_ptr, N, B, pb.data_ptr(),
               rois.data_ptr(), lv.data_ptr(), 2, 5, 224.0, 4, flag.data_ptr(), s)
        st["proposal_boxes"], st["proposal_counts"] = pb, cnt_dev
        self._mark(evs)
        feat = self._box_head(pyr, rois, lv, st)
        self._mark(evs)
        _, obj_prob, obj_cls, attr_logits = self._predictor(feat, K, st)
        At = int(cfg.ROI_BOX_HEAD.NUM_ATTRS)
        attr_prob = torch.empty(K, dtype=torch.float32, device=dev)
        attr_cls = torch.empty(K, dtype=torch.int32, device=dev)
        L.call("vk_softmax_argmax", attr_logits.data_ptr(), attr_logits.shape[1], K, At, At, attr_prob.data_ptr(),
               attr_cls.data_ptr(), None, s)                                                # _predict_attrs :1257-1260
        out = L.vk_outputs(*[bufs[k].data_ptr() for k in bufs])
        L.call("vk_given_box_outputs", obj_prob.data_ptr(), obj_cls.data_ptr(), attr_prob.data_ptr(), attr_cls.data_ptr(),
               pb.data_ptr(), cnt_dev.data_ptr(), sc_ptr, feat.data_ptr(), F_, N, B, C.byref(out), s)
        self._mark(evs)
        if evs is not None:
            self._timing["ev"] = evs
        if int(flag.cpu()) != 0:
            raise AssertionError("Box tensor contains infinite or NaN!")          # frcnn.py:148
        self._last_padded = bufs
        return PendingForward.finished(self, bufs, hw, given_width=B)

    # ---- the stages shared by detection and given boxes ----
    def _bottom_up(self, images, st):
        """stem + res2..res5 (build_backbone frcnn.py:200-261 with res5 as a backbone stage) -> [C2, C3, C4, C5] NHWC."""
        cfg, dev, s = self.config, self.device, stream(self.device)
        N, _, H, W = images.shape
        ho, wo = C.c_int(), C.c_int()
        L.load().vk_stem_out_hw(H, W, int(bool(cfg.MODEL.MAX_POOL)), C.byref(ho), C.byref(wo))
        x = torch.empty((N, ho.value, wo.value, self.stem_c), dtype=self.tdt, device=dev)
        nb = L.load().vk_stem_workspace_bytes(N, H, W, self.stem_c, self.dt)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        L.call("vk_stem", images.data_ptr(), N, H, W, self.stem_w.data_ptr(), self.stem_b.data_ptr(), self.stem_c,
               int(bool(cfg.MODEL.MAX_POOL)), x.data_ptr(), self.dt, ws.data_ptr(), nb, s)
        feats = []
        for name, blocks in zip(self.STAGES, self.stages):
            for blk in blocks:
                x = blk(x)
            feats.append(x)
            st[name] = x
        return feats

    def _box_head(self, pyr, rois, levels, st):
        """RoIAlign 7x7 over P2..P5 by level (fpn.MultiLevelRoIAlign: ROIPooler.forward's level loop :1200-1224, the levels
        assigned there by the rule of :444-460 unless given) -> fc1 -> fc2: [K, FC_DIM] f32."""
        pooled, st["levels"] = self.pooler(pyr[:4], rois, levels)
        st["pooled"] = pooled
        x = pooled.view(pooled.shape[0], -1)
        for i, fcl in enumerate(self.fcs):
            x = fcl(x, relu=True, out_f32=(i + 1 == len(self.fcs)))
        st["box_features"] = x
        return x

    def _predictor(self, feat, K, st):
        """cls_score -> soft-max over C+1 (obj_prob / obj_cls over the first C, the raw arg-max class) -> the attribute
        branch on the raw arg-max class (FastRCNNOutputLayers.forward :1726-1740).  -> (cls_logits, obj_prob, obj_cls,
        attr_logits)."""
        cfg, dev, s = self.config, self.device, stream(self.device)
        F_, Cn, E = feat.shape[1], int(cfg.ROI_HEADS.NUM_CLASSES), self.emb.shape[1]
        cls_logits = self.cls_score(feat, out_f32=True)
        obj_prob = torch.empty(K, dtype=torch.float32, device=dev)
        obj_cls = torch.empty(K, dtype=torch.int32, device=dev)
        max_class = torch.empty(K, dtype=torch.int32, device=dev)
        L.call("vk_softmax_argmax", cls_logits.data_ptr(), cls_logits.shape[1], K, Cn + 1, Cn, obj_prob.data_ptr(), obj_cls.data_ptr(),
               max_class.data_ptr(), s)
        cat = torch.empty((K, F_ + E), dtype=torch.float32, device=dev)
        L.call("vk_concat_embed", feat.data_ptr(), F_, self.emb.data_ptr(), E, max_class.data_ptr(), K, cat.data_ptr(), L.VK_F32, s)
        attr_logits = self.attr_score(self.fc_attr(cat, relu=True), out_f32=True)
        st["obj_logits"], st["attr_logits"] = cls_logits, attr_logits
        return cls_logits, obj_prob, obj_cls, attr_logits
