"""CPU restatement of the default selection rule, roi_outputs.selection = "class_max" (DESIGN.md section 16), for the tests.

Every piece of arithmetic is the oracle's restatement of the reference's own (oracle/frcnn_oracle.py: apply_deltas, clip_box,
nms, argsort_desc inside nms); only three things are written here: the choice of the arg-max class's box (do_nms
frcnn.py:128-129), the loop over the threshold list (ROIOutputs.inference :1274-1278) and the scaling (:1280-1283).
test_class_max_host.py holds this file to the reference's own vectors (tests/golden/kat_ops.npz) and to
FRCNNOracle.roi_outputs; test_gpu_class_max.py holds vk_roi_outputs to this file, bit for bit.

It takes (prob, cls) per row -- the class soft-max's maximum and its column -- as inputs, so that a GPU test can hand it the
device's own soft-max bits; the crafted inputs of both test files are made here too."""
import numpy as np
import torch

from oracle.frcnn_oracle import FRCNNOracle, nms

from test_gpu_per_class import IMG_HW, WEIGHTS, craft as clustered      # the clustered proposals of the per-class tests

C = 7          # classes of the crafted data (background is column C)
A = 5          # attributes (column A is the attributes' background)
SEED = {300: 102}      # craft's seed per R (default: R itself); at 102 both images of R = 300 lie inside the bounds of TABLE_300


def chosen_boxes(cls, boxes_or_deltas, proposals, image_hw, weights):
    """The arg-max class's decoded, clipped box per row -> [R, 4].
    proposals [R, 4] given: boxes_or_deltas are deltas, [R, 4C] (class c at columns 4c..4c+3) or [R, 4] (the chosen class's, or
    class-agnostic); only the chosen 4 are decoded, as on the device: the reference decodes all C and picks (:128-129), which is
    the same arithmetic per box, and its finite-ness assert is evaluated on the boxes that are used.
    proposals None: boxes_or_deltas are the decoded and clipped boxes themselves, [R, C, 4] or [R, 4] (a stage chain hands
    over the device's own: its expf and the host's exp may differ in the last bit)."""
    cls = torch.as_tensor(cls, dtype=torch.int64)
    x = torch.as_tensor(boxes_or_deltas, dtype=torch.float32)
    R = cls.shape[0]
    if R == 0:
        return torch.zeros((0, 4))
    if proposals is None:
        B = x.reshape(R, -1, 4)
        B = (B[torch.arange(R), cls] if B.shape[1] > 1 else B[:, 0]).clone()
        assert bool(torch.isfinite(B).all()), "Box tensor contains infinite or NaN!"
        return B
    d = x.reshape(R, -1, 4)
    d = (d[torch.arange(R), cls] if d.shape[1] > 1 else d[:, 0]).contiguous()
    B = FRCNNOracle.apply_deltas(d, torch.as_tensor(proposals, dtype=torch.float32).reshape(R, 4), weights).reshape(R, 4)
    FRCNNOracle.clip_box(B, image_hw)
    return B


def select_image(prob, cls, boxes_or_deltas, proposals, image_hw, weights, nms_thresh_list, min_detections, max_detections,
                 scale_yx=None, trace=None):
    """The rule for one image.  prob [R] f32 and cls [R]: per row the maximum class probability and its class.
    boxes_or_deltas / proposals: see chosen_boxes.  trace, a list, receives per threshold tried (threshold, kept before the
    cap, stop).  -> ids [n] i64 (rows, in rank order), classes [n] i64, probs [n] f32, boxes [n, 4] f32."""
    prob = torch.as_tensor(prob, dtype=torch.float32).contiguous()
    cls = torch.as_tensor(cls, dtype=torch.int64)
    B = chosen_boxes(cls, boxes_or_deltas, proposals, image_hw, weights)
    mind, maxd = int(min_detections), int(max_detections)
    keep = torch.zeros(0, dtype=torch.int64)
    for t in nms_thresh_list:
        full = nms(B, prob, float(t))
        keep = full[:maxd]
        stop = mind <= len(keep) <= maxd
        if trace is not None:
            trace.append((float(t), len(full), stop))
        if stop:
            break
    boxes = B[keep].clone()
    if scale_yx is not None:
        boxes[:, 0::2] *= scale_yx[1]
        boxes[:, 1::2] *= scale_yx[0]
    return keep, cls[keep], prob[keep], boxes


# ---- the crafted inputs -----------------------------------------------------------------------------------------------
# rows of an image that carry an edge case (R >= MIN_R_SPECIAL)
DUP = ((0, 1), (4, 5))       # rows 1 and 5 copy rows 0 and 4: box, deltas, logits
EQUAL = (2, 3)               # equal logits on two far-apart boxes
OUTSIDE = (6, 7)             # two identical proposals wholly outside the image: both clip to zero area, IoU 0/0
LINE = 8                     # clips to a vertical line on the right edge
MIN_R_SPECIAL = 10


def craft(N, R, seed, counts=None, F=16, dups=True):
    """Clustered proposals with class-specific shifts and zero size deltas (exp(0) = 1: host and device decode to the same
    bits), class and attribute logits in multiples of 1/8 (exact ties are common; two distinct logits differ in probability by
    a factor >= e^0.125), and the edge-case rows above.  Rows >= counts[n] hold NaN logits and inf deltas."""
    d = clustered(N, R, C, seed, counts=counts, F=F)
    g = torch.Generator().manual_seed(seed + 1000)
    K = N * R
    logits = torch.round(torch.randn((K, C + 1), generator=g) * 3.0 * 8) / 8
    attr = torch.round(torch.randn((K, A + 1), generator=g) * 2.0 * 8) / 8
    props, deltas = d["props"], d["deltas"]
    if R >= MIN_R_SPECIAL:
        for n in range(N):
            o = n * R
            if dups:
                for src, dst in DUP:
                    props[n, dst], deltas[o + dst], logits[o + dst], attr[o + dst] = props[n, src], deltas[o + src], logits[o + src], attr[o + src]
            props[n, EQUAL[0]] = torch.tensor([5.0, 300.0, 45.0, 340.0])
            props[n, EQUAL[1]] = torch.tensor([500.0, 5.0, 560.0, 45.0])
            logits[o + EQUAL[1]] = logits[o + EQUAL[0]]
            for r in OUTSIDE:
                props[n, r] = torch.tensor([IMG_HW[1] + 100.0, IMG_HW[0] + 50.0, IMG_HW[1] + 160.0, IMG_HW[0] + 100.0])
            props[n, LINE] = torch.tensor([IMG_HW[1] + 20.0, 100.0, IMG_HW[1] + 80.0, 160.0])
            for r in EQUAL + OUTSIDE + (LINE,):
                deltas[o + r] = 0
    for n in range(N):
        c = int(d["counts"][n])
        logits[n * R + c:(n + 1) * R] = float("nan")
        attr[n * R + c:(n + 1) * R] = float("nan")
        deltas[n * R + c:(n + 1) * R] = float("inf")
    d.update(logits=logits.contiguous(), attr=attr.contiguous())
    del d["scores"]
    return d


def host_prob_cls(logits):
    """_predict_objs (frcnn.py:1252-1255) + do_nms' max over the classes, as FRCNNOracle.roi_outputs computes them."""
    p = torch.nn.functional.softmax(torch.as_tensor(logits, dtype=torch.float32), dim=-1)
    return p[:, :-1].max(1)


def kept_counts(d, n, prob, cls, thresholds):
    """Boxes the class-max NMS of image n keeps at each threshold, uncapped."""
    c, R = int(d["counts"][n]), d["R"]
    rows = slice(n * R, n * R + c)
    B = chosen_boxes(cls[rows], d["deltas"][rows], d["props"][n, :c], d["hw"][n], WEIGHTS)
    return [len(nms(B, torch.as_tensor(prob[rows], dtype=torch.float32).contiguous(), t)) for t in thresholds]


REGIMES = ("first", "retry", "cap", "none", "full")
# the issue's table: bounds for the crafted data at R = 300, where the NMS keeps about 17 / 80 / 276 / 300 boxes
# at 0.05 / 0.3 / 0.7 / 0.9
TABLE_300 = {"first": ((0.05, 0.3, 0.9), 10, 20), "retry": ((0.05, 0.3, 0.9), 50, 100), "cap": ((0.05, 0.3, 0.9), 36, 36),
             "none": ((0.05, 0.3, 0.7), 290, 300), "full": ((0.97,), 300, 300)}


def regime(name, R, n05, n03, n07):
    """(thresholds, min_detections, max_detections) of a regime.  R = 300 takes the table; every other R derives the bounds
    the same way from the counts the restatement keeps at 0.05 / 0.3 / 0.7 (n05, n03, n07: one entry per image), so that
    every image is in the regime; assert_regime then checks that each is."""
    if R == 300:
        return TABLE_300[name]
    if name == "first":
        return (0.05, 0.3, 0.9), max(1, min(n05) // 2), min(R, max(n05) + 3)
    if name == "retry":
        return (0.05, 0.3, 0.9), max(n05) + 1, min(R, max(n03) + 20)
    if name == "cap":
        m = (max(n05) + min(n03)) // 2
        return (0.05, 0.3, 0.9), m, m
    if name == "none":
        return (0.05, 0.3, 0.7), max(n07) + 1, R
    return (0.97,), R, R


def assert_regime(name, trace, n_out, mind, maxd, R):
    """The regime is reached, from the restatement's trace of one image alone."""
    stops = [s for _, _, s in trace]
    if name == "first":
        assert stops == [True] and trace[0][1] <= maxd, trace
    elif name == "retry":
        assert stops == [False, True] and trace[0][1] < mind and trace[1][1] <= maxd, trace
    elif name == "cap":          # lands because of keep[:maxd]: the sweep stops at the maxd-th box
        assert stops[-1] and trace[-1][1] > maxd and n_out == maxd, trace
    elif name == "none":         # the last threshold's result stands
        assert not any(stops) and len(trace) == 3 and n_out == trace[-1][1] < mind, trace
    else:
        assert stops == [True] and n_out == R, trace


def i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)
