#!/usr/bin/env python3
"""Golden vectors for the document encoder from `transformers.LayoutLMModel`, `LayoutLMForTokenClassification`,
`LayoutLMForQuestionAnswering` and `LayoutLMForSequenceClassification` themselves (runs in the build container only; the tests
never import transformers for them).

No checkpoint can be fetched offline, so the models are built from a small config with build-owned seeded weights
(vltk_amd.layoutlm.make_layoutlm_state_dict / make_layoutlm_head_state_dict, regenerated from the seed by the tests, never
stored) and run on the CPU in fp32 on seeded inputs.  Inputs, outputs and the `state_dict()` names and shapes of the four classes
(small and default config) go to tests/golden/layoutlm_small.npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.layoutlm import (layoutlm_config, layoutlm_head_param_spec, layoutlm_param_spec,  # noqa: E402
                               make_layoutlm_head_state_dict, make_layoutlm_state_dict)

SMALL = dict(vocab_size=500, hidden_size=128, num_attention_heads=4, intermediate_size=256, num_hidden_layers=2,
             max_position_embeddings=96, max_2d_position_embeddings=1024, type_vocab_size=2)
HEADS = {"token": ("classifier", 7), "qa": ("qa_outputs", 2), "seq": ("classifier", 5)}
SEED = 2026
GEOMETRY = {"short": (3, 40), "long": (2, 80)}             # B, L: the small matrix-core attention kernel and the tiled one
CASES = [(geo, case) for geo in GEOMETRY for case in ("plain", "masked", "nobox")]


def draw_inputs(cfg, geo, seed=SEED):
    """Every input of one geometry.  The boxes cover the edges of the tables: the full page (a coordinate of 0 and one of 1000),
    a zero-width box, a zero-height box, a point."""
    B, Lt = GEOMETRY[geo]
    g = np.random.Generator(np.random.PCG64([seed, Lt]))
    ids = g.integers(1, cfg["vocab_size"], (B, Lt))
    tts = g.integers(0, 2, (B, Lt))
    xs = np.sort(g.integers(0, 1001, (B, Lt, 2)), -1)
    ys = np.sort(g.integers(0, 1001, (B, Lt, 2)), -1)
    bbox = np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)
    bbox[0, 0] = (0, 0, 1000, 1000)
    bbox[0, 1] = (417, 20, 417, 61)                       # zero width
    bbox[0, 2] = (3, 999, 640, 999)                       # zero height
    bbox[1, 0] = (1000, 0, 1000, 0)                       # a point in a corner
    bbox[1, Lt - 1] = (0, 0, 0, 0)                        # what padding carries
    amask = np.ones((B, Lt), np.float32)                  # ragged; every row keeps >= 2 tokens
    amask[1, Lt - 7:] = 0
    if B > 2:
        amask[2, 2:] = 0
    return dict(input_ids=ids, token_type_ids=tts, bbox=bbox, attention_mask=amask)


def case_inputs(inp, case):
    """The keyword arguments of one stored case (`<geometry>/<case>`)."""
    kw = dict(input_ids=inp["input_ids"])
    if case != "nobox":
        kw.update(bbox=inp["bbox"])
    if case == "masked":
        kw.update(attention_mask=inp["attention_mask"], token_type_ids=inp["token_type_ids"])
    return kw


def spec_of(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def main():
    import transformers as tr
    classes = {"token": tr.LayoutLMForTokenClassification, "qa": tr.LayoutLMForQuestionAnswering,
               "seq": tr.LayoutLMForSequenceClassification}
    out = {"seed": np.asarray(SEED)}
    out.update({f"cfg/{k}": np.asarray(v) for k, v in SMALL.items()})
    out.update({f"{h}/num_labels": np.asarray(n) for h, (_, n) in HEADS.items()})
    for tag, full in (("small", SMALL), ("default", {})):  # names, shapes and order of transformers' state_dict()
        c = layoutlm_config(**full)
        with torch.device("meta"):
            specs = {"model": spec_of(tr.LayoutLMModel(tr.LayoutLMConfig(**c)))}
            for h, (_, n) in HEADS.items():
                specs[h] = spec_of(classes[h](tr.LayoutLMConfig(num_labels=n, **c)))
        assert specs["model"] == [(k, tuple(s)) for k, s in layoutlm_param_spec(c)], "param spec differs from transformers' state_dict"
        for h, (lin, n) in HEADS.items():
            assert specs[h] == [(k, tuple(s)) for k, s in layoutlm_head_param_spec(c, lin, n)], f"{h} param spec differs"
        for k, spec in specs.items():
            out[f"spec/{tag}/{k}/names"] = np.asarray([name for name, _ in spec])
            out[f"spec/{tag}/{k}/shapes"] = np.asarray([tuple(s) + (0,) * (2 - len(s)) for _, s in spec], np.int64)

    cfg = layoutlm_config(**SMALL)
    hf = tr.LayoutLMModel(tr.LayoutLMConfig(**cfg)).eval()
    hf.load_state_dict({k: torch.from_numpy(v) for k, v in make_layoutlm_state_dict(cfg, SEED).items()}, strict=True)
    heads = {}
    for h, (lin, n) in HEADS.items():
        heads[h] = classes[h](tr.LayoutLMConfig(num_labels=n, **cfg)).eval()
        heads[h].load_state_dict({k: torch.from_numpy(v) for k, v in make_layoutlm_head_state_dict(cfg, lin, n, SEED).items()}, strict=True)
    grabbed = []
    hf.embeddings.register_forward_hook(lambda mod, args, output: grabbed.append(output.detach().numpy().copy()))

    inputs = {geo: draw_inputs(cfg, geo) for geo in GEOMETRY}
    for geo, inp in inputs.items():
        out.update({f"{geo}/{k}": v for k, v in inp.items()})
    with torch.no_grad():
        for geo, case in CASES:
            kw = {k: torch.from_numpy(v) for k, v in case_inputs(inputs[geo], case).items()}
            tag = f"{geo}/{case}"
            del grabbed[:]
            o = hf(**kw)
            assert len(grabbed) == 1
            out[f"{tag}/embedding_output"] = grabbed[0]
            out[f"{tag}/last_hidden_state"] = o.last_hidden_state.numpy()
            out[f"{tag}/pooler_output"] = o.pooler_output.numpy()
            out[f"{tag}/token_logits"] = heads["token"](**kw).logits.numpy()
            qa = heads["qa"](**kw)
            out[f"{tag}/start_logits"], out[f"{tag}/end_logits"] = qa.start_logits.numpy(), qa.end_logits.numpy()
            out[f"{tag}/seq_logits"] = heads["seq"](**kw).logits.numpy()
            print(tag, "emb |max| %.3f seq |max| %.3f pooled |max| %.3f" % tuple(
                np.abs(out[f"{tag}/{k}"]).max() for k in ("embedding_output", "last_hidden_state", "pooler_output")),
                "labels", out[f"{tag}/token_logits"].argmax(-1)[0, :8], "seq", out[f"{tag}/seq_logits"].argmax(-1))
    path = os.path.join(ROOT, "tests", "golden", "layoutlm_small.npz")
    np.savez_compressed(path, **out)
    print("layoutlm_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
