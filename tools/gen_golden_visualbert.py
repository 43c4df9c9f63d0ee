#!/usr/bin/env python3
"""Golden vectors for the single-stream encoder from `transformers.VisualBertModel` / `VisualBertForQuestionAnswering`
themselves (runs in the build container only; the tests never import transformers for them).

No checkpoint can be fetched offline, so the models are built from a small config with build-owned seeded weights
(vltk_amd.visualbert.make_visualbert_state_dict / make_visualbert_qa_state_dict, regenerated from the seed by the tests, never
stored) and run on the CPU in fp32 on seeded inputs.  Inputs and outputs only go to tests/golden/visualbert_small.npz; the
visual features are regenerated from the seed as well (tests/visualbert_util.py draws in this file's order).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.visualbert import (make_visualbert_qa_state_dict, make_visualbert_state_dict, visualbert_config,  # noqa: E402
                                 visualbert_param_spec, visualbert_qa_param_spec)

SMALL = dict(vocab_size=500, hidden_size=128, num_attention_heads=4, intermediate_size=256, num_hidden_layers=2,
             max_position_embeddings=64, type_vocab_size=2, visual_embedding_dim=2048)
NUM_LABELS = 40
SEED = 2025
GEOMETRY = {"short": (3, 11, 36), "long": (2, 20, 36)}      # B, Lt, V: 47 tokens (one-pass attention) and 56 (tiled)
ALIGN_A = 3


def draw_inputs(cfg, geo, seed=SEED):
    """Every input of one geometry, in a fixed order of draws (the tests redraw `visual_embeds` with this function's twin)."""
    B, Lt, V = GEOMETRY[geo]
    g = np.random.Generator(np.random.PCG64([seed, Lt]))
    ids = g.integers(1, cfg["vocab_size"], (B, Lt))
    tts = g.integers(0, 2, (B, Lt))
    feats = np.maximum(g.standard_normal((B, V, cfg["visual_embedding_dim"])), 0).astype(np.float32) * 2.0     # ReLU'd RoI features
    vtts = g.integers(0, 2, (B, V))
    align = g.integers(0, Lt, (B, V, ALIGN_A))
    align[g.uniform(size=align.shape) < 0.4] = -1
    align[0, 5] = -1                                      # a box aligned to no word
    align[1, 7] = (-1, Lt - 1, -1)                        # one valid entry, not the first
    amask = np.ones((B, Lt), np.float32)                  # ragged text; every row keeps >= 2 tokens (the QA head gathers sum - 2)
    amask[1, Lt - 4:] = 0
    if B > 2:
        amask[2, 4:] = 0
    vmask = np.ones((B, V), np.float32)
    vmask[0, 30:] = 0                                     # a masked tail of boxes
    return dict(input_ids=ids, token_type_ids=tts, visual_embeds=feats, visual_token_type_ids=vtts, image_text_alignment=align,
                attention_mask=amask, visual_attention_mask=vmask)


def case_inputs(inp, case):
    """The keyword arguments of one stored case (`<geometry>/<case>`)."""
    kw = dict(input_ids=inp["input_ids"], visual_embeds=inp["visual_embeds"])
    if case in ("masked", "aligned"):
        kw.update(attention_mask=inp["attention_mask"], visual_attention_mask=inp["visual_attention_mask"],
                  token_type_ids=inp["token_type_ids"])
    if case == "aligned":
        kw.update(image_text_alignment=inp["image_text_alignment"], visual_token_type_ids=inp["visual_token_type_ids"])
    return kw


CASES = [("short", "masked"), ("short", "plain"), ("long", "masked"), ("long", "aligned")]


def main():
    from transformers import VisualBertConfig, VisualBertForQuestionAnswering, VisualBertModel
    cfg = visualbert_config(**SMALL)
    hf_keys = {k: v for k, v in cfg.items()}
    for full in (SMALL, {}):                               # the small and the default geometry: names, shapes and order
        c = visualbert_config(**full)
        with torch.device("meta"):
            ref = VisualBertModel(VisualBertConfig(**c))
            ref_qa = VisualBertForQuestionAnswering(VisualBertConfig(num_labels=NUM_LABELS, **c))
        assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(s)) for k, s in visualbert_param_spec(c)], \
            "param spec differs from transformers' state_dict"
        assert [(k, tuple(v.shape)) for k, v in ref_qa.state_dict().items()] == \
            [(k, tuple(s)) for k, s in visualbert_qa_param_spec(c, NUM_LABELS)], "QA param spec differs from transformers' state_dict"
    hf = VisualBertModel(VisualBertConfig(**hf_keys)).eval()
    hf.load_state_dict({k: torch.from_numpy(v) for k, v in make_visualbert_state_dict(cfg, SEED).items()}, strict=True)
    qa = VisualBertForQuestionAnswering(VisualBertConfig(num_labels=NUM_LABELS, **hf_keys)).eval()
    qa.load_state_dict({k: torch.from_numpy(v) for k, v in make_visualbert_qa_state_dict(cfg, NUM_LABELS, SEED).items()}, strict=True)

    out = {"seed": np.asarray(SEED), "qa/num_labels": np.asarray(NUM_LABELS)}
    out.update({f"cfg/{k}": np.asarray(v) for k, v in SMALL.items()})
    inputs = {geo: draw_inputs(cfg, geo) for geo in GEOMETRY}
    for geo, inp in inputs.items():
        out.update({f"{geo}/{k}": v for k, v in inp.items() if k != "visual_embeds"})
    with torch.no_grad():
        for geo, case in CASES:
            kw = {k: torch.from_numpy(v) for k, v in case_inputs(inputs[geo], case).items()}
            o = hf(output_hidden_states=True, **kw)
            tag = f"{geo}/{case}"
            out[f"{tag}/last_hidden_state"] = o.last_hidden_state.numpy()
            out[f"{tag}/pooler_output"] = o.pooler_output.numpy()
            out[f"{tag}/embedding_output"] = o.hidden_states[0].numpy()
            print(tag, "seq |max| %.3f pooled |max| %.3f emb |max| %.3f" % tuple(np.abs(out[f"{tag}/{k}"]).max() for k in
                                                                                ("last_hidden_state", "pooler_output", "embedding_output")))
        for geo in GEOMETRY:                              # the QA head on the masked inputs; transformers' gather needs an integer text mask
            kw = {k: torch.from_numpy(v) for k, v in case_inputs(inputs[geo], "masked").items()}
            kw["attention_mask"] = kw["attention_mask"].to(torch.int64)
            assert int(kw["attention_mask"].sum(1).min()) >= 2
            out[f"qa/{geo}/logits"] = qa(**kw).logits.numpy()
            print(f"qa/{geo} logits |max| %.3f argmax %s" % (np.abs(out[f"qa/{geo}/logits"]).max(), out[f"qa/{geo}/logits"].argmax(-1)))
    path = os.path.join(ROOT, "tests", "golden", "visualbert_small.npz")
    np.savez_compressed(path, **out)
    print("visualbert_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
