"""CPU restatement of roi_outputs.selection = "detections" (DESIGN.md section 18), for the tests.

The rule is detectron2's fast_rcnn_inference_single_image; every piece of arithmetic is the oracle's restatement of the
reference's own (oracle/frcnn_oracle.py: apply_deltas, clip_box, nms through per_class_util.class_boxes).  Step 3 is written
in the plain form -- NMS over ALL rows of a class, then the threshold -- while the device sweeps the candidates alone, so
the tests that hold the device to this file prove the two equal."""
import numpy as np
import torch

from oracle.frcnn_oracle import nms

from per_class_util import class_boxes


def select_image(scores, deltas, proposals, image_hw, weights, nms_thresh, score_thresh, max_detections, scale_yx=None, boxes=None):
    """The contract for one image.  scores [R, >= C] probabilities (the first C columns are the classes; C = the deltas'
    classes, or the scores' columns minus the background when the deltas are class-agnostic), deltas [R, 4C] or [R, 4].
    boxes [R, C, 4], when given, are step 1's decoded and clipped boxes themselves (a stage chain hands over the device's own).
    -> dict(ids [n_out] i64 proposal rows, classes [n_out] i64, probs [n_out] f32, boxes [n_out, 4] f32, n_survivors int)."""
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
    rows, classes = [], []
    for c in range(C if R else 0):
        keep = nms(B[:, c].contiguous(), S[:, c].contiguous(), nms_thresh)      # over all R rows of the class
        keep = keep[S[keep, c].double() > float(score_thresh)]                   # strict; NaN and zero are never candidates
        rows.append(keep.numpy())
        classes.append(np.full(len(keep), c, np.int64))
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    c = np.concatenate(classes) if classes else np.zeros(0, np.int64)
    s = S.numpy()[r, c] if len(r) else np.zeros(0, np.float32)
    order = np.lexsort((c, r, -s.astype(np.float64)))                            # score descending, then lower row, then lower class
    order = order[:min(len(order), int(max_detections))]
    r, c, s = r[order], c[order], s[order]
    out = B[torch.from_numpy(r), torch.from_numpy(c)].clone() if len(r) else torch.zeros((0, 4))
    if scale_yx is not None:                                                     # frcnn.py:1280-1283
        out[:, 0::2] *= scale_yx[1]
        out[:, 1::2] *= scale_yx[0]
    return dict(ids=torch.from_numpy(r), classes=torch.from_numpy(c), probs=torch.from_numpy(s.astype(np.float32)), boxes=out,
                n_survivors=sum(len(x) for x in rows))
