"""Host-side mirror of the reference's `FRCNN` module over the HIP C ABI.

Same call surface as `vltk.modeling.frcnn.FRCNN` (reference
vltk/modeling/frcnn.py:1743-2004): `FRCNN(cfg)`, `FRCNN.from_pretrained(path,
config=...)` (local paths only), `model(images, image_shapes, scales_yx=...,
**kwargs)` returning the 7-key OrderedDict, and the mutable
`model.roi_outputs.{nms_thresh, score_thresh, min_detections, max_detections}`
attributes callers set (tests/frcnn_test.py:16-19), plus `model.roi_outputs.selection`
("class_max", the reference's rule; "per_class": NMS per class with a live score_thresh; or
"detections": a detector's (box, class, score) triples, NMS per class over the pairs above score_thresh).

All arithmetic runs in libvltk_hip.so (hand-written gfx950 kernels); torch is
used only to own device memory and to hand out result tensors.  There is no
CPU path: constructing the model without the library or without a GPU raises.
"""
import ctypes as C
import os
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .config import CONFIG_NAME, WEIGHTS_NAME, Config
from .layers import DTYPES, TORCH_DTYPES, stream
from .parallel import OutputBlock, output_spec


SELECTIONS = ("class_max", "per_class", "detections")
MAX_DETECTIONS_DETECTIONS = 1024      # the library's bound on max_detections with selection = "detections"


class ROIOutputs:
    """The mutable knobs of the reference's ROIOutputs (frcnn.py:1229-1240), and `selection`, which is this project's.

    selection = "class_max" (the default): the reference's rule -- NMS over each box's arg-max class, over the list of
    nms_thresh, until the count lands in [min_detections, max_detections].  score_thresh is accepted and unused, as
    upstream (do_nms frcnn.py:116 never reads it).

    selection = "per_class" (C4 model): NMS per class at the one nms_thresh, a box's confidence is
    its best class that survives NMS, boxes are ranked by confidence and those at or above score_thresh are kept, the
    count bounded to [min_detections, max_detections] (and the image's proposals).  obj_ids / obj_probs / boxes are that
    class, its probability and its regressed box; attr_ids / attr_probs are the reference's per-proposal values.  A list
    of several nms_thresh, min_detections > max_detections or a score_thresh outside [0, 1] is a ValueError.

    selection = "detections" (C4 model): a detector's output, the rule of detectron2's
    fast_rcnn_inference_single_image.  Every (proposal, class) pair whose probability is strictly above score_thresh is a
    candidate, NMS runs per class at the one nms_thresh, and the best max_detections (box, class, score) triples of the
    image come out, ranked by score (then lower proposal, then lower class).  A proposal may come out under several
    classes (stage "keep_ids" is each output row's proposal) and an image may yield nothing; roi_features / attr_ids /
    attr_probs of a row are its proposal's.  min_detections must be 0 -- the rule has no minimum count, and the config's
    MIN_DETECTIONS, which it starts as, must be cleared on purpose; 1 <= max_detections <= 1024, which may exceed POST_NMS_TOPK_TEST; one
    nms_thresh and a score_thresh in [0, 1]; anything else is a ValueError."""

    def __init__(self, cfg):
        self.score_thresh = cfg.ROI_HEADS.SCORE_THRESH_TEST     # read by selection = "per_class" and "detections" only
        self.min_detections = cfg.MIN_DETECTIONS
        self.max_detections = cfg.MAX_DETECTIONS
        nms_thresh = cfg.ROI_HEADS.NMS_THRESH_TEST
        self.nms_thresh = list(nms_thresh) if isinstance(nms_thresh, (list, tuple)) else [nms_thresh]
        self.selection = "class_max"

    def params(self):
        """The knobs as the library's vk_roi_params; ValueError beyond VK_MAX_NMS_THRESH thresholds."""
        thr = list(self.nms_thresh)
        if len(thr) > L.VK_MAX_NMS_THRESH:
            raise ValueError(f"at most {L.VK_MAX_NMS_THRESH} NMS thresholds")
        rp = L.vk_roi_params()
        rp.num_nms_thresh = len(thr)
        for i, t in enumerate(thr):
            rp.nms_thresh[i] = float(t)
        rp.min_detections, rp.max_detections = int(self.min_detections), int(self.max_detections)
        return rp

    def select_params(self):
        """Validate `selection` and its knobs -> None for "class_max" (the forward then takes params()), the library's
        vk_select_params for "per_class" and "detections".  ValueError: an unknown selection; in either of those a list of
        more (or fewer) than one nms_thresh (never silently ignored) or a score_thresh outside [0, 1]; in "per_class"
        min_detections > max_detections; in "detections" a min_detections other than 0 or a max_detections outside 1..1024."""
        sel = getattr(self, "selection", "class_max")
        if sel not in SELECTIONS:
            raise ValueError(f"roi_outputs.selection={sel!r} must be one of {SELECTIONS}")
        if sel == "class_max":
            return None
        thr = list(self.nms_thresh)
        if len(thr) != 1:
            raise ValueError(f'selection="{sel}" takes one nms_thresh, got the list {thr}')
        lo, hi = int(self.min_detections), int(self.max_detections)
        if sel == "detections":
            if lo != 0:
                raise ValueError(f'selection="detections" reports nothing when nothing clears score_thresh, so it has no '
                                 f"minimum count to fill: min_detections={lo} must be 0 (it starts as the config's MIN_DETECTIONS; set it to 0)")
            if not 1 <= hi <= MAX_DETECTIONS_DETECTIONS:
                raise ValueError(f'selection="detections": max_detections={hi} must be in 1..{MAX_DETECTIONS_DETECTIONS}')
        elif lo > hi:
            raise ValueError(f"min_detections={lo} exceeds max_detections={hi}")
        score = float(self.score_thresh)
        if not 0.0 <= score <= 1.0:
            raise ValueError(f"score_thresh={score} must be in [0, 1]")
        sp = L.vk_select_params()
        sp.mode = L.VK_SELECT_DETECTIONS if sel == "detections" else L.VK_SELECT_PER_CLASS
        sp.score_thresh, sp.roi = score, self.params()
        return sp


def _c_config(cfg, dt):
    c = L.vk_config()
    r = cfg.RESNETS
    c.depth, c.num_groups, c.width_per_group = r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP
    c.stem_out_channels, c.res2_out_channels = r.STEM_OUT_CHANNELS, r.RES2_OUT_CHANNELS
    c.stride_in_1x1 = int(bool(r.STRIDE_IN_1X1))
    c.caffe_maxpool = int(bool(cfg.MODEL.MAX_POOL))
    sizes, ratios = cfg.ANCHOR_GENERATOR.SIZES, cfg.ANCHOR_GENERATOR.ASPECT_RATIOS
    if len(sizes) != 1 or len(ratios) != 1:
        raise ValueError("only the single-level (C4) anchor generator is supported")
    c.num_sizes, c.num_ratios = len(sizes[0]), len(ratios[0])
    for i, v in enumerate(sizes[0]):
        c.sizes[i] = v
    for i, v in enumerate(ratios[0]):
        c.ratios[i] = v
    c.anchor_offset = cfg.ANCHOR_GENERATOR.OFFSET
    c.rpn_hidden_channels = cfg.PROPOSAL_GENERATOR.HIDDEN_CHANNELS
    c.rpn_min_size = cfg.PROPOSAL_GENERATOR.MIN_SIZE
    c.rpn_nms_thresh = cfg.RPN.NMS_THRESH
    c.pre_nms_topk, c.post_nms_topk = cfg.RPN.PRE_NMS_TOPK_TEST, cfg.RPN.POST_NMS_TOPK_TEST
    for i, v in enumerate(cfg.RPN.BBOX_REG_WEIGHTS):
        c.rpn_bbox_weights[i] = v
    c.num_classes, c.num_attrs = cfg.ROI_HEADS.NUM_CLASSES, cfg.ROI_BOX_HEAD.NUM_ATTRS
    c.use_attr = int(bool(cfg.ROI_BOX_HEAD.ATTR))
    c.pooler_resolution = cfg.ROI_BOX_HEAD.POOLER_RESOLUTION
    c.res5_halve = int(bool(cfg.ROI_BOX_HEAD.RES5HALVE))
    c.cls_agnostic_bbox_reg = int(bool(cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG))
    for i, v in enumerate(cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS):
        c.roi_bbox_weights[i] = v
    c.precision = dt
    return c


POOLER_TYPES = {"ROIPool": L.VK_POOLER_ROIPOOL, "ROIAlign": L.VK_POOLER_ROIALIGN, "ROIAlignV2": L.VK_POOLER_ROIALIGNV2}


def pooler_from_config(cfg):
    """The C4 head's box pooler -> (VK_POOLER_*, sampling ratio).  ROI_BOX_HEAD.POOLER_TYPE: absent or "ROIPool" (the
    reference's RoIPool, frcnn.py:1179), "ROIAlign" (RoIAlign, aligned = False) or "ROIAlignV2" (aligned = True, detectron2's
    C4 default); anything else is a ValueError.  ROI_BOX_HEAD.POOLER_SAMPLING_RATIO (default 0 = adaptive) is read by the
    two RoIAlign types only and must be an integer in 0..8.  Host only: the library validates the pair (vk_pooler_check).
    RoIAlign is torchvision's / detectron2's rule: parity unpinned for the rule."""
    head = cfg.ROI_BOX_HEAD
    kind = getattr(head, "POOLER_TYPE", "ROIPool")
    if not isinstance(kind, str) or kind not in POOLER_TYPES:
        raise ValueError(f"ROI_BOX_HEAD.POOLER_TYPE={kind!r} must be one of {tuple(POOLER_TYPES)}")
    if POOLER_TYPES[kind] == L.VK_POOLER_ROIPOOL:
        return L.VK_POOLER_ROIPOOL, 0
    ratio = getattr(head, "POOLER_SAMPLING_RATIO", 0)
    if isinstance(ratio, (bool, np.bool_)) or not isinstance(ratio, (int, np.integer)):
        raise ValueError(f"ROI_BOX_HEAD.POOLER_SAMPLING_RATIO={ratio!r} must be an integer in 0..8")
    L.call("vk_pooler_check", POOLER_TYPES[kind], int(ratio))
    return POOLER_TYPES[kind], int(ratio)


MAX_GIVEN_BOXES = 1024          # boxes per image of vk_forward_boxes_begin


def _validate_proposals(proposals, N):
    """-> (one [N, K, 4] tensor or a list of N [K_i, 4] tensors, counts int32 [N]); ValueError on a bad shape."""
    if isinstance(proposals, (torch.Tensor, np.ndarray)):
        t = torch.as_tensor(proposals)
        if t.dim() != 3 or t.shape[2] != 4:
            raise ValueError(f"proposals as one array must be [N, K, 4], got shape {tuple(t.shape)}")
        if t.shape[0] != N:
            raise ValueError(f"proposals: {t.shape[0]} images of boxes for {N} images")
        if t.shape[1] > MAX_GIVEN_BOXES:
            raise ValueError(f"proposals: {t.shape[1]} boxes per image, at most {MAX_GIVEN_BOXES}")
        return t, np.full(N, t.shape[1], dtype=np.int32)
    items = list(proposals)
    if len(items) != N:
        raise ValueError(f"proposals: {len(items)} images of boxes for {N} images")
    ts = []
    for i, b in enumerate(items):
        t = b if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float32))
        if t.numel() == 0 and t.dim() == 1:          # [] for an image without boxes
            t = t.reshape(0, 4)
        if t.dim() != 2 or t.shape[1] != 4:
            raise ValueError(f"proposals[{i}] must be [K, 4], got {tuple(t.shape)}")
        if t.shape[0] > MAX_GIVEN_BOXES:
            raise ValueError(f"proposals[{i}]: {t.shape[0]} boxes, at most {MAX_GIVEN_BOXES}")
        ts.append(t)
    return ts, np.asarray([t.shape[0] for t in ts], dtype=np.int32).reshape(N)


def pack_proposals(proposals, N, device=None):
    """Validate caller-supplied boxes and pack them for vk_forward_boxes_begin.

    proposals: a sequence of N arrays / tensors of shape [K_i, 4] (x0, y0, x1, y1; K_i may be 0), or one [N, K, 4]
    array / tensor.  Returns (boxes, counts): boxes a contiguous float32 [N, B, 4] tensor on `device` (B = max K_i; rows
    >= K_i are zero), counts a host int32 numpy array [N].  Raises ValueError on a wrong N, a wrong shape or K_i > 1024.
    Non-finite values pass: the device flags them and the forward raises the reference's assertion (frcnn.py:148)."""
    ts, counts = _validate_proposals(proposals, N)
    if isinstance(ts, torch.Tensor):
        return ts.to(device=device, dtype=torch.float32).contiguous(), counts
    B = int(counts.max(initial=0))
    if all(t.device.type == "cpu" for t in ts):       # one host-to-device copy
        host = np.zeros((N, B, 4), dtype=np.float32)
        for i, t in enumerate(ts):
            host[i, :t.shape[0]] = t.detach().to(torch.float32).numpy()
        return torch.from_numpy(host).to(device), counts
    out = torch.zeros((N, B, 4), dtype=torch.float32, device=device)
    for i, t in enumerate(ts):
        out[i, :t.shape[0]] = t.detach().to(device=out.device, dtype=torch.float32)
    return out, counts


MAX_IGNOREY = L.VK_MAX_IGNOREY  # bands per image of ignorey=


def _validate_ignorey(ignorey, N):
    """-> (a list of N [J_i, 2] CPU tensors, f64): ValueError on a bad shape, more than 64 bands for one image or a dtype
    that is not a real number.  f64: ignorey (one of its arrays) is float64 -- torch's promoted dtype of the reference's
    `ignorey * 1 / scales_yx[n, 1]` with float32 scales; anything else computes in float32."""
    if isinstance(ignorey, (torch.Tensor, np.ndarray)):
        t = torch.as_tensor(ignorey)
        if t.dim() != 3 or t.shape[2] != 2:                # assert ignorey.ndim == 3 (frcnn.py:329)
            raise ValueError(f"ignorey as one array must be [N, J, 2], got shape {tuple(t.shape)}")
        if t.shape[0] != N:
            raise ValueError(f"ignorey: {t.shape[0]} images of bands for {N} images")
        items = list(t.detach().cpu())
    else:
        items = list(ignorey)
        if len(items) != N:
            raise ValueError(f"ignorey: {len(items)} images of bands for {N} images")
    ts = []
    for i, b in enumerate(items):
        t = torch.as_tensor(b).detach().cpu()
        if t.numel() == 0 and t.dim() == 1:          # [] for an image without bands
            t = t.reshape(0, 2)
        if t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"ignorey[{i}] must be [J, 2] (y0, y1 rows), got {tuple(t.shape)}")
        if t.shape[0] > MAX_IGNOREY:
            raise ValueError(f"ignorey[{i}]: {t.shape[0]} bands, at most {MAX_IGNOREY}")
        if t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"ignorey[{i}]: dtype {t.dtype} is not a real number")
        ts.append(t)
    return ts, any(t.dtype == torch.float64 for t in ts)


def pack_ignorey(ignorey, scales_yx, N):
    """Validate ignorey= and scale it for vk_forward_begin_ignorey / vk_rpn_proposals*_ignorey.

    ignorey: one [N, J, 2] array / tensor (the reference's form) or a sequence of N [J_i, 2] ones (J_i may be 0), rows
    (y0, y1) in the frame scales_yx maps to (original-image pixels).  scales_yx: host float32 [N, 2] or None.  Returns
    None when there is nothing to apply -- no band at all, or no scales_yx, which the reference ignores ignorey without
    (frcnn.py:328; a UserWarning here) -- else (bands, counts, f64): bands a C-contiguous [N, max J_i, 2] float32 /
    float64 numpy array holding ignorey[n] * 1 / scales_yx[n, 1] computed by torch on the CPU exactly as frcnn.py:331 does
    (the x scale on y values: the reference's quirk, kept), rows >= J_i zero; counts int32 [N].  ValueError on a bad
    shape, J_i > 64, or a scaled band that is not finite or not below 2^31 in magnitude (the reference's int() raises)."""
    ts, f64 = _validate_ignorey(ignorey, N)
    if scales_yx is None:
        warnings.warn("ignorey is ignored without scales_yx, as in the reference (frcnn.py:328)", UserWarning, stacklevel=3)
        return None
    counts = np.asarray([t.shape[0] for t in ts], dtype=np.int32).reshape(N)
    J = int(counts.max(initial=0))
    if J == 0:
        return None
    dt = torch.float64 if f64 else torch.float32
    sc = torch.from_numpy(np.ascontiguousarray(np.asarray(scales_yx, dtype=np.float32).reshape(N, 2)))
    bands = np.zeros((N, J, 2), dtype=np.float64 if f64 else np.float32)
    for n, t in enumerate(ts):
        if t.shape[0] == 0:
            continue
        g = (t.to(dt) * 1 / sc[n, 1]).numpy()                 # frcnn.py:331
        if not (np.isfinite(g).all() and (np.abs(g) < 2.0 ** 31).all()):
            raise ValueError(f"ignorey[{n}]: bands / scales_yx[{n}][1] must be finite and below 2^31 in magnitude, got {g.tolist()}")
        bands[n, :t.shape[0]] = g
    return bands, counts, f64


def check_given_width(width, max_detections):
    """Given boxes are never truncated: an explicit max_detections below the widest image's box count is an error."""
    if max_detections is not None and int(max_detections) < width:
        raise ValueError(f"max_detections={int(max_detections)} is smaller than the {width} boxes given for one image; "
                         "given boxes are never truncated")


MAX_GRID_CELLS = 1024  # cells per image of grid=


def check_grid(grid):
    """grid= -> (Gh, Gw) as ints: two integers >= 1 with Gh * Gw <= 1024; anything else is a ValueError."""
    try:
        gh, gw = grid
    except (TypeError, ValueError):
        raise ValueError(f"grid must be (Gh, Gw), got {grid!r}") from None
    for v in (gh, gw):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"grid must be two integers, got {grid!r}")
    gh, gw = int(gh), int(gw)
    if gh < 1 or gw < 1 or gh * gw > MAX_GRID_CELLS:
        raise ValueError(f"grid=({gh}, {gw}) must have Gh, Gw >= 1 and at most {MAX_GRID_CELLS} cells")
    return gh, gw


class _Ticket:
    """State of one forward in flight; the model keeps these in issue order (`FRCNN._open`)."""

    __slots__ = ("ticket", "block", "images", "done", "error")

    def __init__(self, ticket, block, images):
        self.ticket, self.block = ticket, block
        self.images = images           # keeps the input (and given boxes) alive until the kernels have read it
        self.done, self.error = False, None


class PendingForward:
    """A forward in flight (FRCNN.forward_async).  Handles are waited for in issue order; a handle that is DROPPED
    (garbage-collected) without a wait closes its own ticket and every older one that is still open, in order, so an
    out-of-order drop cannot leave tickets open (the results of those older forwards stay available to their handles)."""

    def __init__(self, model, state, hw, given_width=None):
        self.model, self._state, self.hw = model, state, hw
        self.given_width = given_width      # given boxes: the output width (max boxes per image); None for detection

    @classmethod
    def finished(cls, model, block, hw, given_width=None):
        """A handle over a forward that has already run to its end (the FPN detector's forward is synchronous)."""
        st = _Ticket(-1, block, None)
        st.done = True
        return cls(model, st, hw, given_width)

    @property
    def ticket(self):
        return self._state.ticket

    @property
    def block(self):
        return self._state.block

    def wait_raw(self):
        """Finish the forward; returns the fixed-capacity OutputBlock ([N, D, ...] device tensors)."""
        st = self._state
        if not st.done:
            self.model._end(st)         # ValueError if an older forward is still open (it stays open)
        if st.error is not None:
            raise st.error              # the forward finished and failed (non-finite boxes, frcnn.py:148)
        self.model._last_padded = st.block
        return st.block

    def wait(self, **kwargs):
        if self.given_width is not None:
            check_given_width(self.given_width, kwargs.get("max_detections"))
        return FRCNN._format(self.wait_raw(), self.hw, **kwargs)

    def __del__(self):
        try:
            if not self._state.done and self.model._h:
                self.model._close_through(self._state)
        except Exception:
            pass


class FRCNN:
    given_boxes = True                   # forward(proposals=...): region features for caller-supplied boxes
    grid_features = True                 # forward(grid=(Gh, Gw)): Res5 over the whole map, pooled to a grid of cells

    def __new__(cls, cfg=None, *a, **k):
        # several RPN input levels = the FPN detector (frcnn_fpn.py, a build extension); one = the reference's C4 model
        if cls is FRCNN and cfg is not None and len(cfg.RPN.IN_FEATURES) > 1:
            from .frcnn_fpn import FRCNNFPN
            return object.__new__(FRCNNFPN)
        return object.__new__(cls)

    def __init__(self, cfg, precision=None, device=None):
        self._init_host(cfg, precision, device)
        self.pooler = pooler_from_config(cfg)          # before the handle exists: a bad POOLER_TYPE raises here
        self._h = C.c_void_p()
        L.call("vk_create", C.byref(_c_config(cfg, self.dt)), self.device.index, C.byref(self._h))
        L.call("vk_set_pooler", self._h, *self.pooler)

    def _init_host(self, cfg, precision, device):
        """What the C4 model and the FPN detector (frcnn_fpn.py) set up alike: the GPU and library checks, the device, the
        precision, ROIOutputs and the forward bookkeeping."""
        if not torch.cuda.is_available():
            raise RuntimeError("vltk_amd.FRCNN needs an AMD GPU (HIP device); there is no CPU fallback")
        L.load()
        self.config = cfg
        self.min_detections = cfg.min_detections
        self.max_detections = cfg.max_detections
        dev = torch.device(device if device is not None else cfg.MODEL.DEVICE)
        if dev.type != "cuda" or dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.precision = precision or os.environ.get("VLTK_AMD_PRECISION", "fp16")
        if self.precision not in ("fp16", "fp32"):
            raise KeyError(self.precision)
        self.dt, self.tdt = DTYPES[self.precision]
        self.roi_outputs = ROIOutputs(cfg)
        self.training = False
        self._open = []                # _Ticket of every forward in flight, oldest first
        self._finalized = False

    # ---- nn.Module-like surface -----------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                L.load().vk_destroy(h)
            except Exception:
                pass
            self._h = None

    def expected_keys(self):
        n = C.c_int()
        L.call("vk_num_weights", self._h, C.byref(n))
        out = []
        for i in range(n.value):
            s = C.c_char_p()
            L.call("vk_weight_name", self._h, i, C.byref(s))
            out.append(s.value.decode())
        return out

    def load_state_dict(self, state_dict, strict=True):
        """Strict load in the reference's key layout (frcnn.py:1862-1881), then fold BN / repack on the device."""
        if self._finalized:
            raise RuntimeError("weights were already loaded into this model")
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if a.dtype == np.int64:
                dt = L.VK_I64
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                dt = L.VK_F32
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            L.call("vk_load_weights", self._h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, dt)
        L.call("vk_finalize", self._h)
        self._finalized = True
        return self

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        """Local branch of the reference loader (frcnn.py:1757-1922): a directory holding
        `pytorch_model.bin` (+ `config.yaml`) or a direct file path.  Fetch-by-name needs the network."""
        config = kwargs.pop("config", None)
        state_dict = kwargs.pop("state_dict", None)
        precision = kwargs.pop("precision", None)
        if not isinstance(config, Config):
            config = Config.from_pretrained(config if config is not None else pretrained_model_name_or_path)
        if state_dict is None:
            path = pretrained_model_name_or_path
            if os.path.isdir(path):
                path = os.path.join(path, WEIGHTS_NAME)
                if not os.path.isfile(path):
                    raise EnvironmentError(
                        "Error no file named {} found in directory {} ".format(WEIGHTS_NAME, pretrained_model_name_or_path))
            elif not os.path.isfile(path):
                raise EnvironmentError(f"Can't load weights for '{pretrained_model_name_or_path}'.")
            try:
                state_dict = torch.load(path, map_location="cpu", weights_only=True)
            except Exception:
                raise OSError("Unable to load weights from pytorch checkpoint file. ")
        model = cls(config, precision=precision)
        model.load_state_dict(state_dict)
        return model.eval()

    def set_option(self, key, value):
        L.call("vk_set_option", self._h, key.encode(), int(value))

    def get_option(self, key):
        """An option's current value; also the read-only "working_sets" and "lane_forwards" (vk_get_option)."""
        v = C.c_int()
        L.call("vk_get_option", self._h, key.encode(), C.byref(v))
        return v.value

    def enable_stage_timing(self, on=True):
        L.call("vk_enable_stage_timing", self._h, int(on))

    def stage_timing_ms(self):
        ms = (C.c_float * 6)()
        L.call("vk_get_stage_timing", self._h, ms)
        return dict(zip(("backbone", "rpn_head", "proposals", "roi_heads", "predictor_outputs", "total"), list(ms)))

    def enable_kernel_timing(self, on=True):
        L.call("vk_enable_kernel_timing", self._h, int(on))

    def kernel_timing(self, reset=False):
        """Per-bucket (launches, ms, algorithmic flops) of the conv launches since the last reset."""
        n = (C.c_int64 * 12)()
        ms = (C.c_double * 12)()
        fl = (C.c_double * 12)()
        by = (C.c_double * 12)()
        L.call("vk_get_kernel_timing", self._h, n, ms, fl, by, int(reset))
        names = ("conv_mfma256", "conv_mfma_f16", "conv_mfma_f16_f32out", "other", "conv3x3_panel", "conv_duo", "two_stream_backbone", "conv3x3_blk", "conv_ws",
                 "conv_mfma256_dual", "conv_gemm4", "bneck64")
        return {k: {"launches": int(n[i]), "ms": float(ms[i]), "flops": float(fl[i]), "bytes": float(by[i])}
                for i, k in enumerate(names)}

    def get_stage(self, name):
        """Intermediate tensor of the last forward as a torch tensor (a copy)."""
        ptr, dt, nd = C.c_void_p(), C.c_int(), C.c_int()
        shape = (C.c_int64 * 4)()
        L.call("vk_get_stage", self._h, name.encode(), C.byref(ptr), C.byref(dt), shape, C.byref(nd))
        shp = [int(shape[i]) for i in range(nd.value)]
        out = torch.empty(shp, dtype=TORCH_DTYPES[dt.value], device=self.device)
        nbytes = out.numel() * out.element_size()
        L.call("vk_memcpy_d2d", out.data_ptr(), ptr.value, nbytes, stream(self.device))
        torch.cuda.synchronize(self.device)
        return out

    # ---- forward ----------------------------------------------------------
    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def forward(self, images, image_shapes, gt_boxes=None, proposals=None, scales_yx=None, ignorey=None, grid=None, **kwargs):
        """kwargs (v1.0.0 semantics): max_detections, return_tensors {"np","pt",None},
        padding {None,"max_detections","max_batch"}, pad_value, location {"cuda","cpu"}.

        proposals (C4 and FPN models): region features for caller-supplied boxes instead of detection.  A sequence of N
        [K_i, 4] arrays / tensors (x0, y0, x1, y1; 0 <= K_i <= 1024) or one [N, K, 4] tensor, in the frame of the
        returned `boxes`: network-input pixels, or original-image pixels when `scales_yx` is given (x is divided by
        scales_yx[n][1], y by scales_yx[n][0] on the device).  Every box is kept, in input order: clipped to
        image_shapes[n] (_clip_box frcnn.py:147-153; a non-finite box raises its AssertionError), RoI-pooled, run through
        the Res5 head (the FPN model: RoIAlign by level and the FC head) (roi_features) and the box predictor (obj_probs / obj_ids: max / arg-max of the soft-max over the
        first C classes; attr_probs / attr_ids on that class); `boxes` = the clipped box times the scales, with no box
        regression and no NMS; preds_per_image[n] = K_i.  roi_outputs.{nms_thresh, min_detections, max_detections}
        are not used; the output width is max K_i, and an explicit max_detections below it raises ValueError.

        ignorey (detection only; with `proposals` a ValueError): horizontal bands whose RPN proposals are removed or
        trimmed (find_top_rpn_proposals frcnn.py:328-366) -- one [N, J, 2] array / tensor or N [J_i, 2] ones, rows (y0, y1)
        divided by scales_yx[n][1]; at most 64 per image.  Applied only with scales_yx, as in the reference (a UserWarning
        without).  See pack_ignorey and DESIGN §13.

        grid=(Gh, Gw) (C4 model only; with `proposals` or `ignorey` a ValueError): grid features instead of detection --
        the Res5 stage runs once over the whole res4 map and the result is average-pooled over each image's content to
        Gh x Gw cells (adaptive_avg_pool2d's bins), row i * Gw + j for cell (i, j).  Every image gets exactly Gh * Gw
        rows (preds_per_image), the same 2048-wide roi_features, the box predictor's obj / attr outputs on each row as
        the given-box forward produces them, and `boxes` = the cell's extent in network pixels (times scales_yx).  No
        RPN, no NMS; roi_outputs is not used; 1 <= Gh, Gw, Gh * Gw <= 1024, and an explicit max_detections below
        Gh * Gw raises ValueError.  The rule is this project's: parity unpinned for the rule.

        Which detections come out is roi_outputs.selection's: "class_max" (the reference's rule, the default) or
        "per_class" (NMS per class, a live score_thresh; see ROIOutputs and DESIGN §15), or "detections" (a detector's
        output: every (proposal, class) pair above score_thresh, NMS per class, the best max_detections triples; possibly
        none).  The given-box and grid forwards ignore roi_outputs; ignorey composes with every selection,
        because it acts on the proposals."""
        if proposals is not None and self.given_boxes:         # before anything is enqueued
            counts = _validate_proposals(proposals, len(images))[1]
            check_given_width(int(counts.max(initial=0)), kwargs.get("max_detections"))
        if grid is not None:                                   # before anything is enqueued
            self._check_grid_args(grid, proposals, ignorey)
            gh, gw = check_grid(grid)
            check_given_width(gh * gw, kwargs.get("max_detections"))
        return self.forward_async(images, image_shapes, gt_boxes, proposals, scales_yx, ignorey, grid).wait(**kwargs)

    def _check_grid_args(self, grid, proposals, ignorey):
        if not self.grid_features:
            raise ValueError("grid= is the C4 model's: the FPN detector has no Res5 stage to run over a map")
        if proposals is not None:
            raise ValueError("grid= pools fixed cells: it cannot be combined with proposals=")
        if ignorey is not None:
            raise ValueError("ignorey removes / trims RPN proposals: there are none with grid=")

    def _prepare(self, images, image_shapes, proposals, scales_yx, ignorey):
        """The argument checks and host-side parsing both detectors' forward_async start with; nothing is enqueued.
        -> (images [N,3,H,W] f32 on the device, image_shapes int32 [N,2], scales_yx f32 [N,2] or None, pack_proposals'
        (boxes, counts) or None, pack_ignorey's result or None)."""
        if self.training:
            raise NotImplementedError()            # frcnn.py:1930-1931
        if ignorey is not None and proposals is not None:
            raise ValueError("ignorey removes / trims RPN proposals: there are none with proposals=")
        if not self._finalized:
            raise RuntimeError("no weights loaded: call load_state_dict / from_pretrained first")
        images = torch.as_tensor(images)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [N,3,H,W], got {tuple(images.shape)}")
        N = images.shape[0]
        sc = None
        if scales_yx is not None:
            sc = np.ascontiguousarray(np.asarray(torch.as_tensor(scales_yx).cpu(), dtype=np.float32).reshape(N, 2))
        ig = pack_ignorey(ignorey, sc, N) if ignorey is not None else None
        given = pack_proposals(proposals, N, self.device) if proposals is not None else None
        images = images.to(device=self.device, dtype=torch.float32).contiguous()
        hw = np.ascontiguousarray(np.asarray(torch.as_tensor(image_shapes).cpu()).reshape(N, 2), dtype=np.int32)
        return images, hw, sc, given, ig

    def forward_async(self, images, image_shapes, gt_boxes=None, proposals=None, scales_yx=None, ignorey=None, grid=None):
        """Enqueue a forward and return at once (vk_forward_begin, vk_forward_begin_select with
        roi_outputs.selection = "per_class" or "detections", vk_forward_boxes_begin with `proposals`, or vk_forward_grid_begin with `grid`,
        see forward()); `.wait(**kwargs)`
        on the returned handle finishes it (vk_forward_end) and formats the outputs like forward().  Up to four may be in
        flight, detection and given-box forwards mixed; they must be waited for in order, on the same stream.  The caller
        must not modify `images` (or the proposals) before wait() returns.  Forwards in flight together run beside each
        other on the device (option "forward_lanes", 2 by default: two working sets and two streams of the model's own;
        `set_option("forward_lanes", 1)` keeps them one after the other on the current stream); the results are the same
        bits, and wait() orders the current stream behind the forward."""
        if grid is not None:
            self._check_grid_args(grid, proposals, ignorey)
            grid = check_grid(grid)
        images, hw, sc, given, ig = self._prepare(images, image_shapes, proposals, scales_yx, ignorey)
        N, _, H, W = images.shape
        F = self.config.RESNETS.RES2_OUT_CHANNELS * 8
        dev, s = self.device, stream(self.device)
        scp = sc.ctypes.data_as(C.c_void_p) if sc is not None else None
        ticket = C.c_int64(-1)
        if grid is not None:
            gh, gw = grid
            bufs = OutputBlock(output_spec(N, gh * gw, F), device=dev)
            out = L.vk_outputs(*[bufs[k].data_ptr() for k in bufs])
            L.call("vk_forward_grid_begin", self._h, images.data_ptr(), N, H, W, hw.ctypes.data_as(C.c_void_p), scp, gh, gw,
                   C.byref(out), s, C.byref(ticket))
            st = _Ticket(ticket.value, bufs, images)
            self._open.append(st)
            return PendingForward(self, st, hw, given_width=gh * gw)
        if given is not None:
            boxes, counts = given
            B = boxes.shape[1]
            bufs = OutputBlock(output_spec(N, B, F), device=dev)
            out = L.vk_outputs(*[bufs[k].data_ptr() for k in bufs])
            L.call("vk_forward_boxes_begin", self._h, images.data_ptr(), N, H, W, hw.ctypes.data_as(C.c_void_p), scp,
                   boxes.data_ptr() if B else None, B, counts.ctypes.data_as(C.c_void_p), C.byref(out), s, C.byref(ticket))
            st = _Ticket(ticket.value, bufs, (images, boxes))
            self._open.append(st)
            return PendingForward(self, st, hw, given_width=B)
        sp = self.roi_outputs.select_params()        # None: selection = "class_max", the entry points below
        rp = self.roi_outputs.params()
        # one flat block, the seven arrays are views (so the multi-GPU exchange is a single all-gather: parallel.py)
        bufs = OutputBlock(output_spec(N, rp.max_detections, F), device=dev)
        out = L.vk_outputs(*[bufs[k].data_ptr() for k in bufs])
        if sp is not None:                           # "per_class" / "detections": NMS per class; ignorey acts before it
            igs = None
            if ig is not None:
                bands, bcounts, f64 = ig
                igs = C.byref(L.vk_ignorey(bands.ctypes.data, bcounts.ctypes.data, bands.shape[1], int(f64)))
            L.call("vk_forward_begin_select", self._h, images.data_ptr(), N, H, W, hw.ctypes.data_as(C.c_void_p), scp,
                   C.byref(sp), C.byref(out), s, C.byref(ticket), igs)
        elif ig is None:
            L.call("vk_forward_begin", self._h, images.data_ptr(), N, H, W, hw.ctypes.data_as(C.c_void_p), scp, C.byref(rp),
                   C.byref(out), s, C.byref(ticket))
        else:                                      # the host bands are copied into the ticket's slot before the call returns
            bands, bcounts, f64 = ig
            igs = L.vk_ignorey(bands.ctypes.data, bcounts.ctypes.data, bands.shape[1], int(f64))
            L.call("vk_forward_begin_ignorey", self._h, images.data_ptr(), N, H, W, hw.ctypes.data_as(C.c_void_p), scp,
                   C.byref(rp), C.byref(out), s, C.byref(ticket), C.byref(igs))
        st = _Ticket(ticket.value, bufs, images)
        self._open.append(st)
        return PendingForward(self, st, hw)

    def _end(self, st):
        """vk_forward_end for one ticket.  Out of order -> ValueError from the library, nothing changes."""
        try:
            L.call("vk_forward_end", self._h, C.c_int64(st.ticket))
        except ValueError:
            raise
        except Exception as e:          # the forward itself ended; its assertion failed
            st.error = e
        st.done, st.images = True, None
        if st in self._open:
            self._open.remove(st)

    def _close_through(self, st):
        """End every open forward up to and including `st`, oldest first."""
        while self._open:
            head = self._open[0]
            self._end(head)
            if head is st:
                break

    inference = forward

    def forward_padded(self):
        """Fixed-capacity [N, D, ...] device tensors of the last forward (rows >= preds_per_image are zero)."""
        return self._last_padded

    @staticmethod
    def _format(bufs, hw, padding=None, max_detections=None, return_tensors=None, pad_value=0, location=None, **_):
        assert return_tensors in {"pt", "np", None}
        assert padding in {"max_detections", "max_batch", None}
        ppi = bufs["preds_per_image"].cpu()
        counts = ppi.tolist()
        N = len(counts)
        keys = ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "roi_features")
        if padding is None and return_tensors is None:
            # live-tree behaviour (frcnn.py:1996-2004): lists of per-image tensors
            out = OrderedDict((k, [bufs[k][i, :counts[i]] for i in range(N)]) for k in keys[:5])
            out["preds_per_image"] = ppi
            out["roi_features"] = [bufs["roi_features"][i, :counts[i]] for i in range(N)]
            return OrderedDict((k, out[k]) for k in
                               ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "preds_per_image", "roi_features"))
        D = bufs["obj_ids"].shape[1]
        if padding == "max_detections":
            width = int(max_detections) if max_detections is not None else D
        elif padding == "max_batch":
            width = max(counts) if counts else 0
        else:
            width = None

        def fix(t):
            if width is None:
                if len(set(counts)) > 1:
                    raise ValueError("return_tensors without padding needs equal detections per image")
                t = t[:, :counts[0]] if counts else t
            elif width <= t.shape[1]:
                t = t[:, :width].clone()
            else:
                pad = torch.zeros((t.shape[0], width - t.shape[1]) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
                t = torch.cat([t, pad], dim=1)
            if pad_value != 0 and width is not None:
                for i, c in enumerate(counts):
                    t[i, c:] = pad_value
            if location == "cpu" or return_tensors == "np":
                t = t.cpu()
            return t.numpy() if return_tensors == "np" else t

        out = OrderedDict((k, fix(bufs[k])) for k in keys)
        sizes = torch.as_tensor(hw.astype(np.int64))
        out["preds_per_image"] = ppi.numpy() if return_tensors == "np" else ppi
        out["sizes"] = sizes.numpy() if return_tensors == "np" else sizes
        nb = out["boxes"].copy() if return_tensors == "np" else out["boxes"].clone()
        hwf = hw.astype(np.float32)
        if return_tensors == "np":
            nb[:, :, 0::2] /= hwf[:, 1].reshape(-1, 1, 1)
            nb[:, :, 1::2] /= hwf[:, 0].reshape(-1, 1, 1)
        else:
            s = torch.as_tensor(hwf, device=nb.device)
            nb[:, :, 0::2] /= s[:, 1].view(-1, 1, 1)
            nb[:, :, 1::2] /= s[:, 0].view(-1, 1, 1)
        out["normalized_boxes"] = nb
        return OrderedDict((k, out[k]) for k in ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "sizes",
                                                 "preds_per_image", "roi_features", "normalized_boxes"))
