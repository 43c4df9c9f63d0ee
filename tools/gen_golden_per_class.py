#!/usr/bin/env python3
"""tests/golden/e2e_per_class.npz: the per-class selection (roi_outputs.selection = "per_class") built
from the REFERENCE's own pieces.  Runs only where the reference exists (tools/gen_golden.py's load_reference).

The reference's FRCNN.forward runs with hooks for the proposals, obj_logits, attr_logits, box_deltas and feature_pooled; then
its ROIOutputs._predict_boxes / _predict_objs / _predict_attrs, its _clip_box and its nms (the torchvision stub: oracle/tv_ops.c,
parity unpinned like every use of that op).  Only the loop over classes, the max over the classes a box survives in and the
count rule are this project's: the rule itself has no reference to be pinned to, and DESIGN.md says so.

The ranking by confidence does not depend on score_thresh, so one ranked list per image (the first max_detections rows) and the
count per threshold describe every case.  The scores and deltas are stored for the classes that decide the result only (every
box's confidence class, plus each box's three best classes) with a row checksum of the full deltas, as e2e_r101_small.npz
does: per-class NMS runs class by class, so the rule over those columns reproduces ids, classes and confidences exactly
(tests/test_per_class_host.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_per_class.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden import OUT, load_reference, np_, tie_free, to_torch_sd    # noqa: E402
from vltk_amd.config import Config, vg_c4_config_dict       # noqa: E402
from vltk_amd.weights import make_state_dict, synthetic_images   # noqa: E402

N, H, W = 2, 256, 352
SHAPES = ((256, 352), (240, 320))
POST_TOPK, SEED, IMAGES_SEED, DEPTH = 40, 1234, 16, 101      # weights of seed 1234; see MIN_MARGIN for the images' seed
NMS_T, MIN_DET, MAX_DET = 0.3, 6, 16
SCORE_THRESH = (0.9, 0.6, 0.4, 0.2)
EXPECT_COUNTS = {0.9: [7, 6], 0.6: [14, 11], 0.4: [16, 16], 0.2: [16, 16]}      # minimum / inside / maximum all occur
SCALES = ((1.25, 1.5), (2.0, 1.75))
PERTURB, TRIALS = 1e-5, 6
# The GPU's strict mode is held to these vectors at 1e-3 of the largest value (probabilities: about 1e-3 absolute), and must
# give identical ids and counts: every gap of the ranking down to the first row left out, and every threshold's distance to
# the nearest confidence, has to be wider than that.  With the images of seed 1234 image 1's ranks 8 and 9 are 2e-5 apart;
# of the image seeds 1..20 seed 16 has the widest smallest margin (2.0e-3) and still shows all three count regimes.
MIN_MARGIN = 1e-3


def rule(ref, ro, obj_logits, box_deltas, proposals, sizes):
    """Per image: (max_conf [R], cls [R], order [R], boxes [R, C, 4], second-best surviving score [R])."""
    ppi = [len(p) for p in proposals]
    boxes_all = ro._predict_boxes(proposals, box_deltas, ppi)
    probs_all = ro._predict_objs(obj_logits, ppi)
    res = []
    for boxes, probs, size in zip(boxes_all, probs_all, sizes):
        R, C = boxes.shape[0], boxes.shape[1] // 4
        b = boxes.reshape(-1, 4).clone()
        ref._clip_box(b, size)
        b = b.view(R, C, 4)
        S = probs[:, :C]
        conf, second = torch.zeros(R), torch.zeros(R)
        cls, seen = torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.bool)
        for c in range(C):
            keep = ref.nms(b[:, c].contiguous(), S[:, c].contiguous(), NMS_T)
            s = S[keep, c]
            better = ~seen[keep] | (s > conf[keep])
            second[keep] = torch.where(better, conf[keep], torch.maximum(second[keep], s))
            rows = keep[better]
            conf[rows], cls[rows], seen[rows] = s[better], c, True
        order = torch.from_numpy(np.argsort(-conf.numpy(), kind="stable"))
        res.append((conf, cls, order, b, second))
    return res


def count(conf, thresh):
    return min(max(int((conf.double() >= thresh).sum()), MIN_DET), MAX_DET, len(conf))


def main():
    ref = load_reference()
    cfg = Config(vg_c4_config_dict(depth=DEPTH, post_nms_topk=POST_TOPK))
    sd = make_state_dict(cfg, seed=SEED)
    net = ref.FRCNN(cfg).eval()
    net.load_state_dict(to_torch_sd(sd), strict=True)
    images = torch.from_numpy(synthetic_images(N, H, W, seed=IMAGES_SEED))
    for i, (hh, ww) in enumerate(SHAPES):
        images[i, :, hh:, :] = 0
        images[i, :, :, ww:] = 0
    st = {}
    hooks = [net.proposal_generator.rpn_head.register_forward_hook(lambda m, i, o: st.update(obj=o[0][0])),
             net.proposal_generator.register_forward_hook(lambda m, i, o: st.update(pboxes=o[0])),
             net.roi_heads.register_forward_hook(
                 lambda m, i, o: st.update(obj_logits=o[0], attr_logits=o[1], box_deltas=o[2], feat=o[3]))]
    with torch.no_grad():
        net(images, torch.tensor(SHAPES))
    for hk in hooks:
        hk.remove()
    tie_free(np_(st["obj"]), "per_class rpn logits")
    ro, props = net.roi_outputs, [p.clone() for p in st["pboxes"]]
    ppi = [len(p) for p in props]
    C = cfg.ROI_HEADS.NUM_CLASSES
    with torch.no_grad():
        base = rule(ref, ro, st["obj_logits"], st["box_deltas"], props, SHAPES)
        attr_p, attr_i = ro._predict_attrs(st["attr_logits"], ppi)
        probs = ro._predict_objs(st["obj_logits"], ppi)
    feats = st["feat"].split(ppi, 0)

    counts = {t: [count(r[0], t) for r in base] for t in SCORE_THRESH}
    print("counts", counts)
    assert counts == EXPECT_COUNTS, counts

    # the selection must not hang on the last bits of the logits / deltas: ids and classes survive 1e-5 perturbations
    g = torch.Generator().manual_seed(99)
    for trial in range(TRIALS):
        dl = (torch.rand(st["obj_logits"].shape, generator=g) * 2 - 1) * PERTURB
        dd = (torch.rand(st["box_deltas"].shape, generator=g) * 2 - 1) * PERTURB
        with torch.no_grad():
            pert = rule(ref, ro, st["obj_logits"] + dl, st["box_deltas"] + dd, props, SHAPES)
        for i, (a, b) in enumerate(zip(base, pert)):
            for t in SCORE_THRESH:
                k = count(a[0], t)
                assert count(b[0], t) == k, (trial, i, t)
                assert torch.equal(a[2][:k], b[2][:k]) and torch.equal(a[1][a[2][:k]], b[1][b[2][:k]]), (trial, i, t)
    print(f"{TRIALS} perturbations of {PERTURB:g}: no selected id or class changed")

    out = {"images_seed": np.asarray(IMAGES_SEED), "weights_seed": np.asarray(SEED), "shapes": np.asarray(SHAPES),
           "nhw": np.asarray([N, H, W]), "post_topk": np.asarray(POST_TOPK), "depth": np.asarray(DEPTH),
           "nms_thresh": np.asarray(NMS_T), "min_detections": np.asarray(MIN_DET), "max_detections": np.asarray(MAX_DET),
           "score_thresh": np.asarray(SCORE_THRESH), "counts": np.asarray([counts[t] for t in SCORE_THRESH]),
           "scales_yx": np.asarray(SCALES, dtype=np.float32), "perturbation": np.asarray([PERTURB, TRIALS])}
    off = 0
    for i, (conf, cls, order, b, second) in enumerate(base):
        top = order[:MAX_DET]
        R = len(conf)
        cols = torch.unique(torch.cat([cls, probs[i][:, :C].topk(3, dim=1).indices.reshape(-1)]))      # sorted
        out[f"proposal_boxes_{i}"] = np_(props[i])
        out[f"class_cols_{i}"] = np_(cols)
        out[f"scores_cols_{i}"] = np_(probs[i][:, cols])
        bd = st["box_deltas"][off:off + R]
        out[f"deltas_cols_{i}"] = np_(bd.view(R, C, 4)[:, cols].reshape(R, -1))
        out[f"deltas_rowsum_{i}"] = np_(bd.double().sum(1).float())
        out[f"max_conf_{i}"], out[f"cls_{i}"] = np_(conf), np_(cls)
        out[f"keep_ids_{i}"], out[f"obj_ids_{i}"], out[f"obj_probs_{i}"] = np_(top), np_(cls[top]), np_(conf[top])
        bx = b[top, cls[top]]
        out[f"boxes_{i}"] = np_(bx)
        sb = bx.clone()
        sb[:, 0::2] *= SCALES[i][1]            # frcnn.py:1280-1283
        sb[:, 1::2] *= SCALES[i][0]
        out[f"boxes_scaled_{i}"] = np_(sb)
        out[f"attr_ids_{i}"], out[f"attr_probs_{i}"] = np_(attr_i[i][top]), np_(attr_p[i][top])
        out[f"roi_features_{i}"] = np_(feats[i][top])
        # margins: the runner-up class a box survives in; the gaps of the ranking around every count; the thresholds
        out[f"cls_margin_{i}"] = np_((conf - second)[top])
        ranked = conf[order]
        out[f"rank_gap_{i}"] = np_(ranked[:MAX_DET] - ranked[1:MAX_DET + 1])
        out[f"thresh_margin_{i}"] = np.asarray([float((conf.double() - t).abs().min()) for t in SCORE_THRESH])
        assert float(out[f"rank_gap_{i}"].min()) >= MIN_MARGIN and float(out[f"thresh_margin_{i}"].min()) >= MIN_MARGIN, \
            (i, out[f"rank_gap_{i}"], out[f"thresh_margin_{i}"])
        print(f"image {i}: R {R} stored classes {len(cols)} min cls margin {float(out[f'cls_margin_{i}'].min()):.2e} "
              f"min rank gap {float(out[f'rank_gap_{i}'].min()):.2e} min thresh margin {out[f'thresh_margin_{i}'].min():.2e}")
        off += R
    path = os.path.join(OUT, "e2e_per_class.npz")
    np.savez_compressed(path, **out)
    print("e2e_per_class.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
