#!/usr/bin/env python3
"""Golden vectors for the patch-token image encoder from `transformers.ViTModel` / `ViTForImageClassification` themselves (runs
in the build container only; the tests never import transformers for them).

No checkpoint can be fetched offline, so the models are built from small configs with build-owned seeded weights
(vltk_amd.vit.make_vit_state_dict / make_vit_classifier_state_dict, regenerated from the seed by the tests, never stored) and run
on the CPU in fp32 on seeded images.  Inputs and outputs go to tests/golden/vit_small.npz.  Hidden size and head count are
visualbert_small.npz's, so the attention kernels the cases reach are the ones that fixture reaches.

  square  32 x 32 / 8              17 tokens: the small matrix-core attention kernel
  tall    48 x 24, interpolated    19 tokens, gh != gw
  long    64 x 64, interpolated    65 tokens: past 48 queries, the tiled kernel
  p14     28 x 42 / 14 (a model of its own): patch rows that are not 16-byte aligned, C * P * P = 588 (no K-tile multiple)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.vit import (make_vit_classifier_state_dict, make_vit_state_dict, vit_classifier_param_spec, vit_config,  # noqa: E402
                          vit_param_spec)

SEED = 2026
NUM_LABELS = 10
B = 2
CASES = {"square": ("main", (32, 32), False), "tall": ("main", (48, 24), True), "long": ("main", (64, 64), True),
         "p14": ("p14", (28, 42), False)}


def models():
    vb = np.load(os.path.join(ROOT, "tests", "golden", "visualbert_small.npz"))
    common = dict(hidden_size=int(vb["cfg/hidden_size"]), num_attention_heads=int(vb["cfg/num_attention_heads"]),
                  intermediate_size=int(vb["cfg/intermediate_size"]), num_hidden_layers=2)
    return {"main": dict(common, image_size=(32, 32), patch_size=8), "p14": dict(common, image_size=(28, 42), patch_size=14)}


def draw_pixels(case, hw, seed=SEED):
    """Normalised pixel values, N(0, 1), one generator per case."""
    g = np.random.Generator(np.random.PCG64([seed, sorted(CASES).index(case)]))
    return g.standard_normal((B, 3) + tuple(hw)).astype(np.float32)


def main():
    from transformers import ViTConfig, ViTForImageClassification, ViTModel
    small = models()
    for kw in list(small.values()) + [{}]:                # the small and the default geometry: names, shapes and order
        c = vit_config(**kw)
        with torch.device("meta"):
            ref, ref_c = ViTModel(ViTConfig(**c)), ViTForImageClassification(ViTConfig(num_labels=NUM_LABELS, **c))
        assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(s)) for k, s in vit_param_spec(c)], \
            "param spec differs from transformers' state_dict"
        assert [(k, tuple(v.shape)) for k, v in ref_c.state_dict().items()] == \
            [(k, tuple(s)) for k, s in vit_classifier_param_spec(c, NUM_LABELS)], "classifier param spec differs"
    out = {"seed": np.asarray(SEED), "num_labels": np.asarray(NUM_LABELS)}
    hf, hf_c = {}, {}
    for name, kw in small.items():
        cfg = vit_config(**kw)
        out.update({f"cfg/{name}/{k}": np.asarray(v) for k, v in kw.items()})
        hf[name] = ViTModel(ViTConfig(**cfg)).eval()
        hf[name].load_state_dict({k: torch.from_numpy(v) for k, v in make_vit_state_dict(cfg, SEED).items()}, strict=True)
        hf_c[name] = ViTForImageClassification(ViTConfig(num_labels=NUM_LABELS, **cfg)).eval()
        hf_c[name].load_state_dict({k: torch.from_numpy(v) for k, v in make_vit_classifier_state_dict(cfg, NUM_LABELS, SEED).items()},
                                   strict=True)
    with torch.no_grad():
        for case, (name, hw, interp) in CASES.items():
            pix = draw_pixels(case, hw)
            out[f"{case}/pixel_values"] = pix
            out[f"{case}/model"] = np.asarray(name)
            out[f"{case}/interpolate_pos_encoding"] = np.asarray(interp)
            o = hf[name](torch.from_numpy(pix), interpolate_pos_encoding=interp, output_hidden_states=True)
            out[f"{case}/embedding_output"] = o.hidden_states[0].numpy()
            out[f"{case}/last_hidden_state"] = o.last_hidden_state.numpy()
            keys = ["embedding_output", "last_hidden_state"]
            if name == "main":
                out[f"{case}/pooler_output"] = o.pooler_output.numpy()
                out[f"{case}/logits"] = hf_c[name](torch.from_numpy(pix), interpolate_pos_encoding=interp).logits.numpy()
                keys += ["pooler_output", "logits"]
            print(case, out[f"{case}/last_hidden_state"].shape, " ".join("%s |max| %.3f" % (k, np.abs(out[f"{case}/{k}"]).max()) for k in keys))
    path = os.path.join(ROOT, "tests", "golden", "vit_small.npz")
    np.savez_compressed(path, **out)
    print("vit_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
