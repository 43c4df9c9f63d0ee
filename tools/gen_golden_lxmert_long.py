#!/usr/bin/env python3
"""Golden vectors for the encoder at lengths beyond the small attention kernels, from
`transformers.LxmertModel` itself (runs in the build container only).

The layout and the draw order are tools/gen_golden_lxmert.py's, so tests/lxmert_util.golden_inputs rebuilds the weights and the
visual features from the seed.  40 text and 140 visual tokens at head dim 64: every attention of the encoder (40 x 40, 140 x 140,
40 x 140, 140 x 40) is past the 48-query / 64-key kernel, and 140 x 140 is past what one head's LDS image holds in fp32.  Both
masks are ragged.  Only the three outputs are stored (the per-stage hidden states would double the file).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.lxmert import lxmert_config, lxmert_param_spec, make_lxmert_state_dict  # noqa: E402

LONG = dict(vocab_size=500, hidden_size=128, num_attention_heads=2, intermediate_size=256, l_layers=1, x_layers=2, r_layers=1,
            max_position_embeddings=64, type_vocab_size=2, visual_feat_dim=256, visual_pos_dim=4)


def main():
    from transformers import LxmertConfig, LxmertModel
    cfg = lxmert_config(**LONG)
    hf = LxmertModel(LxmertConfig(**cfg)).eval()
    ref_keys = [(k, tuple(v.shape)) for k, v in hf.state_dict().items()]
    assert ref_keys == [(k, tuple(s)) for k, s in lxmert_param_spec(cfg)], "param spec differs from transformers' state_dict"
    seed = 2025
    sd = make_lxmert_state_dict(cfg, seed)
    hf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g = np.random.Generator(np.random.PCG64(seed))
    B, Lq, V = 2, 40, 140
    ids = g.integers(1, cfg["vocab_size"], (B, Lq))
    tts = g.integers(0, 2, (B, Lq))
    amask = np.ones((B, Lq), np.float32)
    amask[0, 33:] = 0
    amask[1, 17:] = 0
    vmask = np.ones((B, V), np.float32)
    vmask[0, 131:] = 0
    vmask[1, 70:] = 0
    feats = np.maximum(g.standard_normal((B, V, cfg["visual_feat_dim"])), 0).astype(np.float32) * 2.0     # ReLU'd RoI features
    x1y1 = g.uniform(0, 0.6, (B, V, 2))
    pos = np.concatenate([x1y1, x1y1 + g.uniform(0.05, 0.4, (B, V, 2))], -1).astype(np.float32)        # normalised boxes
    out = {"seed": np.asarray(seed), "input_ids": ids, "token_type_ids": tts, "attention_mask": amask, "visual_attention_mask": vmask,
           "visual_feats_seed": np.asarray(seed), "visual_pos": pos}
    out.update({f"cfg/{k}": np.asarray(v) for k, v in cfg.items()})
    with torch.no_grad():
        for tag, kw in (("masked", dict(attention_mask=torch.from_numpy(amask), visual_attention_mask=torch.from_numpy(vmask),
                                        token_type_ids=torch.from_numpy(tts))),
                        ("plain", dict())):
            o = hf(input_ids=torch.from_numpy(ids), visual_feats=torch.from_numpy(feats), visual_pos=torch.from_numpy(pos), **kw)
            out[f"{tag}/language_output"] = o.language_output.numpy()
            out[f"{tag}/vision_output"] = o.vision_output.numpy()
            out[f"{tag}/pooled_output"] = o.pooled_output.numpy()
            print(tag, "lang |max| %.3f visn |max| %.3f pooled |max| %.3f" % (np.abs(out[f"{tag}/language_output"]).max(),
                                                                             np.abs(out[f"{tag}/vision_output"]).max(),
                                                                             np.abs(out[f"{tag}/pooled_output"]).max()))
    path = os.path.join(ROOT, "tests", "golden", "lxmert_long.npz")
    np.savez_compressed(path, **out)
    print("lxmert_long.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
