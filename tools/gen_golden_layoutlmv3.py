#!/usr/bin/env python3
"""Golden vectors for LayoutLMv3's relative-position bias from `transformers.models.layoutlmv3.modeling_layoutlmv3.LayoutLMv3Encoder`
itself (runs in the build container only; the tests never import transformers for them) -> tests/golden/layoutlmv3_relpos.npz:

  bucket/<bins>_<max_distance>   transformers' bucket of every delta in [-max_distance - 2, max_distance + 2], for the 1-D setting
                                 (32, 128) and the 2-D setting (64, 256)
  w1, wx, wy, position_ids, bbox, bias
                                 a seeded 4-head encoder's three bias matrices, seeded inputs (positions up to 400 apart; boxes with
                                 the page corners among them) and the [B, heads, L, L] tensor `_cal_1d_pos_emb + _cal_2d_pos_emb`
                                 that every layer of transformers adds to its scores before the division by sqrt(d)
"""
import os

import numpy as np
import torch
from transformers import LayoutLMv3Config
from transformers.models.layoutlmv3.modeling_layoutlmv3 import LayoutLMv3Encoder

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SEED = 2026
SETTINGS = ((32, 128), (64, 256))


def main():
    cfg = LayoutLMv3Config(hidden_size=32, num_attention_heads=4, num_hidden_layers=1, intermediate_size=32, vocab_size=50)
    assert (cfg.rel_pos_bins, cfg.max_rel_pos, cfg.rel_2d_pos_bins, cfg.max_rel_2d_pos) == (32, 128, 64, 256)
    enc = LayoutLMv3Encoder(cfg).eval()
    out = {}
    for bins, maxd in SETTINGS:
        delta = torch.arange(-maxd - 2, maxd + 3)
        out[f"bucket/{bins}_{maxd}"] = enc.relative_position_bucket(delta, num_buckets=bins, max_distance=maxd).numpy().astype(np.int32)
    g = np.random.Generator(np.random.PCG64(SEED))
    w1 = g.standard_normal((4, 32)).astype(np.float32)
    wx = g.standard_normal((4, 64)).astype(np.float32)
    wy = g.standard_normal((4, 64)).astype(np.float32)
    B, Lx = 2, 24
    pos = g.integers(2, 402, (B, Lx))
    pos[0, :6] = np.arange(2, 8)
    xs = np.sort(g.integers(0, 1001, (B, Lx, 2)), -1)
    ys = np.sort(g.integers(0, 1001, (B, Lx, 2)), -1)
    bbox = np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)
    bbox[0, 0] = (0, 0, 1000, 1000)
    bbox[0, 1] = (1000, 0, 1000, 0)
    bbox[1, 0] = (1, 1, 999, 999)
    bbox[1, 1:4, 0] = bbox[1, 0, 0] + np.array([1, 7, 200])        # small, exact-range and log-range x differences
    with torch.no_grad():
        enc.rel_pos_bias.weight.copy_(torch.from_numpy(w1))
        enc.rel_pos_x_bias.weight.copy_(torch.from_numpy(wx))
        enc.rel_pos_y_bias.weight.copy_(torch.from_numpy(wy))
        bias = enc._cal_1d_pos_emb(torch.from_numpy(pos)) + enc._cal_2d_pos_emb(torch.from_numpy(bbox))
    out.update(w1=w1, wx=wx, wy=wy, position_ids=pos.astype(np.int64), bbox=bbox.astype(np.int64), bias=bias.numpy())
    path = os.path.join(ROOT, "tests", "golden", "layoutlmv3_relpos.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
