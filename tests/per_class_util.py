"""CPU restatement of roi_outputs.selection = "per_class" (DESIGN.md section 15), for the tests.

Every piece of arithmetic is the oracle's restatement of the reference's own (oracle/frcnn_oracle.py: apply_deltas, clip_box,
nms, argsort_desc); only the loop over classes, the max over surviving classes and the count rule are written here.
tools/gen_golden_per_class.py holds the same rule over the reference's own methods and wrote tests/golden/e2e_per_class.npz,
which test_per_class_host.py holds this file to."""
import numpy as np
import torch

from oracle.frcnn_oracle import FRCNNOracle, argsort_desc, nms


def class_boxes(deltas, proposals, image_hw, weights, num_classes):
    """_predict_boxes (frcnn.py:1242-1250) + _clip_box on all R*C boxes (do_nms :121) for one image -> [R, C, 4].
    deltas [R, 4C], or [R, 4] (CLS_AGNOSTIC_BBOX_REG: the one box is every class's).  AssertionError on a non-finite box."""
    deltas = torch.as_tensor(deltas, dtype=torch.float32)
    proposals = torch.as_tensor(proposals, dtype=torch.float32)
    R, k = deltas.shape[0], deltas.shape[1] // 4
    props = proposals.unsqueeze(-2).expand(R, k, 4).reshape(-1, 4)
    boxes = FRCNNOracle.apply_deltas(deltas.reshape(R * k, 4), props, weights).reshape(-1, 4)
    FRCNNOracle.clip_box(boxes, image_hw)
    boxes = boxes.view(R, k, 4)
    return boxes.expand(R, num_classes, 4) if k == 1 and num_classes != 1 else boxes


def select_image(scores, deltas, proposals, image_hw, weights, nms_thresh, score_thresh, min_detections, max_detections,
                 scale_yx=None, boxes=None):
    """The contract for one image.  scores [R, >= C] probabilities (the first C columns are the classes; C = deltas' classes,
    or the scores' columns minus the background when the deltas are class-agnostic), deltas [R, 4C] or [R, 4].
    boxes [R, C, 4], when given, are step 2's decoded and clipped boxes themselves and stand in for class_boxes(deltas, ...)
    (a stage chain hands over the device's own boxes: its expf and the host's exp may differ in the last bit).
    -> dict(ids [n_out] i64, classes [n_out] i64, probs [n_out] f32, boxes [n_out, 4] f32, max_conf [R] f32, cls [R] i64)."""
    scores = torch.as_tensor(scores, dtype=torch.float32)
    deltas = torch.as_tensor(deltas, dtype=torch.float32)
    R = scores.shape[0]
    C = deltas.shape[1] // 4 if deltas.shape[1] > 4 else scores.shape[1] - 1
    S = scores[:, :C]
    if boxes is not None:
        B = torch.as_tensor(boxes, dtype=torch.float32).reshape(R, C, 4)
        assert bool(torch.isfinite(B).all()), "Box tensor contains infinite or NaN!"
    else:
        B = class_boxes(deltas, proposals, image_hw, weights, C) if R else torch.zeros((0, C, 4))
    max_conf = torch.zeros(R, dtype=torch.float32)
    cls = torch.zeros(R, dtype=torch.int64)
    seen = torch.zeros(R, dtype=torch.bool)
    for c in range(C if R else 0):
        keep = nms(B[:, c].contiguous(), S[:, c].contiguous(), nms_thresh)
        conf = S[keep, c]
        better = ~seen[keep] | (conf > max_conf[keep])          # classes ascend: a tie stays with the smaller class
        rows = keep[better]
        max_conf[rows], cls[rows], seen[rows] = conf[better], c, True
    order = argsort_desc(max_conf) if R else torch.zeros(0, dtype=torch.int64)      # descending, ties to the lower row
    n_ge = int((max_conf.double() >= float(score_thresh)).sum())
    n_out = min(max(n_ge, int(min_detections)), int(max_detections), R)
    ids = order[:n_out]
    boxes = B[ids, cls[ids]].clone() if n_out else torch.zeros((0, 4))
    if scale_yx is not None:                                    # frcnn.py:1280-1283
        boxes[:, 0::2] *= scale_yx[1]
        boxes[:, 1::2] *= scale_yx[0]
    return dict(ids=ids, classes=cls[ids], probs=max_conf[ids], boxes=boxes, max_conf=max_conf, cls=cls)


def select(scores, deltas, proposals, image_shapes, weights, nms_thresh, score_thresh, min_detections, max_detections,
           scales_yx=None):
    """Per image over lists / row splits: scores and deltas are [sum R_n, ...], proposals a list of [R_n, 4]."""
    res, off = [], 0
    for n, p in enumerate(proposals):
        r = len(p)
        res.append(select_image(scores[off:off + r], deltas[off:off + r], p, image_shapes[n], weights, nms_thresh, score_thresh,
                                min_detections, max_detections, None if scales_yx is None else scales_yx[n]))
        off += r
    return res


def attrs_per_row(attr_logits):
    """_predict_attrs (frcnn.py:1257-1260): per proposal row, (prob, id) of the soft-max over the first A columns."""
    p = torch.as_tensor(attr_logits, dtype=torch.float32)[..., :-1].softmax(-1)
    return p.max(-1)


def i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)
