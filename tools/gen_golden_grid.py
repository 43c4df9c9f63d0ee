#!/usr/bin/env python3
"""tests/golden/e2e_grid.npz: grid features (FRCNN.forward(grid=...)) built from the REFERENCE's own
modules.  Runs only where the reference exists (tools/gen_golden.py's load_reference).

The arithmetic is the reference's: net.backbone, net.roi_heads.res5 on the whole res4 map, F.adaptive_avg_pool2d on each
image's [:fh, :fw] crop of that map, net.roi_heads.box_predictor on the pooled rows and roi_outputs._predict_objs /
_predict_attrs on its logits.  Only the choice of the crop (the content extent) and the cell boxes are this project's: the
rule has no reference to be pinned to, and DESIGN.md says so.

The GPU's strict mode is held to these vectors at 1e-3 and must give identical ids, so every row's gap from the best to the
second class probability, attribute probability and raw class logit (which picks the attribute embedding) must be >= 1e-3:
asserted here.  Images of seed 1234 pass with grids (2, 3) and (4, 5); seed 16 does not (attribute gap 3.7e-5 at (4, 5)), and a
7 x 7 grid does not on seed 1234 (class gap 4.4e-4).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_grid.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden import OUT, load_reference, np_, to_torch_sd    # noqa: E402
from vltk_amd.config import Config, vg_c4_config_dict       # noqa: E402
from vltk_amd.weights import make_state_dict, synthetic_images   # noqa: E402

N, H, W = 2, 256, 352
SHAPES = ((256, 352), (240, 320))
SEED, IMAGES_SEED, DEPTH = 1234, 1234, 101
GRIDS = ((2, 3), (4, 5))
SCALES = ((1.25, 1.5), (2.0, 1.75))
STRIDE = 16
MIN_MARGIN = 1e-3


def gap(t):
    v = t.topk(2, dim=-1).values
    return v[:, 0] - v[:, 1]


def main():
    ref = load_reference()
    cfg = Config(vg_c4_config_dict(depth=DEPTH))
    sd = make_state_dict(cfg, seed=SEED)
    net = ref.FRCNN(cfg).eval()
    net.load_state_dict(to_torch_sd(sd), strict=True)
    images = torch.from_numpy(synthetic_images(N, H, W, seed=IMAGES_SEED))
    for i, (hh, ww) in enumerate(SHAPES):
        images[i, :, hh:, :] = 0
        images[i, :, :, ww:] = 0
    C = cfg.ROI_HEADS.NUM_CLASSES
    with torch.no_grad():
        m = net.roi_heads.res5(net.backbone(images)["res4"])
    print("map", tuple(m.shape))
    Hm, Wm = m.shape[2:]
    out = {"images_seed": np.asarray(IMAGES_SEED), "weights_seed": np.asarray(SEED), "shapes": np.asarray(SHAPES),
           "nhw": np.asarray([N, H, W]), "depth": np.asarray(DEPTH), "grids": np.asarray(GRIDS), "stride": np.asarray(STRIDE),
           "map_hw": np.asarray([Hm, Wm]), "scales_yx": np.asarray(SCALES, dtype=np.float32), "min_margin": np.asarray(MIN_MARGIN)}
    for gh, gw in GRIDS:
        G = gh * gw
        feats, boxes = [], []
        for n, (h, w) in enumerate(SHAPES):
            fh, fw = min(Hm, max(1, -(-h // STRIDE))), min(Wm, max(1, -(-w // STRIDE)))
            with torch.no_grad():
                p = F.adaptive_avg_pool2d(m[n:n + 1, :, :fh, :fw], (gh, gw))            # [1, 2048, gh, gw]
            feats.append(p[0].permute(1, 2, 0).reshape(G, -1))
            b = torch.zeros(G, 4)
            for i in range(gh):
                for j in range(gw):
                    ys, ye = (i * fh) // gh, -(-(i + 1) * fh // gh)
                    xs, xe = (j * fw) // gw, -(-(j + 1) * fw // gw)
                    b[i * gw + j] = torch.tensor([xs * STRIDE, ys * STRIDE, min(xe * STRIDE, w), min(ye * STRIDE, h)], dtype=torch.float32)
            boxes.append(b)
        feat = torch.cat(feats, 0)
        ppi = [G] * N
        with torch.no_grad():
            obj_logits, attr_logits, _ = net.roi_heads.box_predictor(feat)
            probs = torch.cat(net.roi_outputs._predict_objs(obj_logits, ppi), 0)[:, :C]
            attr_p, attr_i = net.roi_outputs._predict_attrs(attr_logits, ppi)
        attr_all = attr_logits[..., :-1].softmax(-1)
        tag = f"{gh}x{gw}"
        margins = {"cls_margin": gap(probs), "attr_margin": gap(attr_all), "logit_margin": gap(obj_logits)}
        for k, v in margins.items():
            out[f"{k}_{tag}"] = np_(v)
            assert float(v.min()) >= MIN_MARGIN, (tag, k, float(v.min()))
        out[f"roi_features_{tag}"] = np_(feat.view(N, G, -1))
        out[f"obj_ids_{tag}"] = np_(probs.argmax(-1).view(N, G))
        out[f"obj_probs_{tag}"] = np_(probs.max(-1).values.view(N, G))
        out[f"attr_ids_{tag}"] = np_(torch.cat(attr_i, 0).view(N, G))
        out[f"attr_probs_{tag}"] = np_(torch.cat(attr_p, 0).view(N, G))
        bx = torch.stack(boxes)
        out[f"boxes_{tag}"] = np_(bx)
        sb = bx.clone()
        for n in range(N):
            sb[n, :, 0::2] *= SCALES[n][1]            # frcnn.py:1280-1283
            sb[n, :, 1::2] *= SCALES[n][0]
        out[f"boxes_scaled_{tag}"] = np_(sb)
        print(f"grid {tag}: class gap {float(margins['cls_margin'].min()):.2e} attribute gap "
              f"{float(margins['attr_margin'].min()):.2e} logit gap {float(margins['logit_margin'].min()):.2e}")
    path = os.path.join(OUT, "e2e_grid.npz")
    np.savez_compressed(path, **out)
    print("e2e_grid.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
