#!/usr/bin/env python3
"""Golden vectors for LayoutLMv3 from `transformers.LayoutLMv3Model`, `LayoutLMv3ForTokenClassification` (5 and 12 labels: one
nn.Linear and the dense -> tanh -> out_proj head), `LayoutLMv3ForQuestionAnswering` and `LayoutLMv3ForSequenceClassification`
themselves (runs in the build container only; the tests never import transformers for them).

No checkpoint can be fetched offline, so the models are built from a small config with build-owned seeded weights
(vltk_amd.layoutlmv3.make_layoutlmv3_state_dict / make_layoutlmv3_head_state_dict, regenerated from the seed by the tests, never
stored; `cls_token`, `pos_embed` and the three bias matrices are drawn non-zero like every other tensor) and run on the CPU in fp32
on seeded inputs.  Stored in tests/golden/layoutlmv3_small.npz: config, seed, inputs; per geometry and case the embedding stage
(what the encoder is fed), `last_hidden_state` and the heads' logits; the `state_dict()` names and shapes of the five classes for
the small and the default config; `create_visual_bbox` for 2 x 2 and 14 x 14 patches; and per geometry and case the deviation of
transformers' own CPU run in bf16 and in fp16 from its fp32 run, max |delta| / max |fp32| of `last_hidden_state` (`dev16/...`).
Should the CPU lack an fp16 op, bf16's figure is stored in its place and `dev16/fp16_is_bf16` is 1.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.layoutlmv3 import (layoutlmv3_config, layoutlmv3_head_param_spec, layoutlmv3_param_spec,  # noqa: E402
                                 make_layoutlmv3_head_state_dict, make_layoutlmv3_state_dict)

SMALL = dict(vocab_size=60, hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=128,
             max_position_embeddings=80, coordinate_size=8, shape_size=16, input_size=32, patch_size=16)
HEADS = {"token5": ("token", 5), "token12": ("token", 12), "qa": ("qa", 2), "seq": ("seq", 5)}
SEED = 2027
B = 2
GEOMETRY = {"short": 11, "long": 60}                       # Lt; L = Lt + 5: 16 (one wave's 16 queries), 65 (one key in the second tile)
CASES = [(geo, case) for geo in GEOMETRY for case in ("plain", "masked", "textonly")]


def draw_inputs(cfg, geo, seed=SEED):
    """Every input of one geometry.  `input_ids` has no pad id; `input_ids_masked` pads the tail of each row (the mask is 0 there)
    and carries one more pad id in the middle of row 0, which the mask keeps."""
    Lt = GEOMETRY[geo]
    g = np.random.Generator(np.random.PCG64([seed, Lt]))
    pad = cfg["pad_token_id"]
    ids = g.integers(pad + 1, cfg["vocab_size"], (B, Lt))
    tts = g.integers(0, 2, (B, Lt))
    xs, ys = np.sort(g.integers(0, 1001, (B, Lt, 2)), -1), np.sort(g.integers(0, 1001, (B, Lt, 2)), -1)
    bbox = np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)
    bbox[0, 0] = (0, 0, 1000, 1000)
    bbox[0, 1] = (417, 20, 417, 61)                        # zero width
    bbox[1, 2] = (3, 999, 640, 999)                        # zero height
    amask = np.ones((B, Lt), np.float32)
    amask[0, Lt - 2:], amask[1, Lt - 5:] = 0, 0
    masked = np.where(amask > 0, ids, pad)
    masked[0, Lt // 2] = pad
    pix = g.standard_normal((B, 3, cfg["input_size"], cfg["input_size"])).astype(np.float32)
    return dict(input_ids=ids, input_ids_masked=masked, token_type_ids=tts, bbox=bbox, attention_mask=amask, pixel_values=pix)


def case_inputs(inp, case):
    """The keyword arguments of one stored case (`<geometry>/<case>`)."""
    kw = dict(input_ids=inp["input_ids"], bbox=inp["bbox"])
    if case == "masked":
        kw.update(input_ids=inp["input_ids_masked"], attention_mask=inp["attention_mask"], token_type_ids=inp["token_type_ids"])
    if case != "textonly":
        kw.update(pixel_values=inp["pixel_values"])
    return kw


def spec_of(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def main():
    import transformers as tr
    classes = {"token": tr.LayoutLMv3ForTokenClassification, "qa": tr.LayoutLMv3ForQuestionAnswering,
               "seq": tr.LayoutLMv3ForSequenceClassification}
    out = {"seed": np.asarray(SEED)}
    out.update({f"cfg/{k}": np.asarray(v) for k, v in SMALL.items()})
    out.update({f"{h}/num_labels": np.asarray(n) for h, (_, n) in HEADS.items()})
    for tag, full in (("small", SMALL), ("default", {})):  # names, shapes and order of transformers' state_dict()
        c = layoutlmv3_config(**full)
        with torch.device("meta"):
            specs = {"model": spec_of(tr.LayoutLMv3Model(tr.LayoutLMv3Config(**c)))}
            for h, (kind, n) in HEADS.items():
                specs[h] = spec_of(classes[kind](tr.LayoutLMv3Config(num_labels=n, **c)))
        assert specs["model"] == [(k, tuple(s)) for k, s in layoutlmv3_param_spec(c)], "param spec differs from transformers' state_dict"
        for h, (kind, n) in HEADS.items():
            assert specs[h] == [(k, tuple(s)) for k, s in layoutlmv3_head_param_spec(c, kind, n)], f"{h} param spec differs"
        for k, spec in specs.items():
            out[f"spec/{tag}/{k}/names"] = np.asarray([name for name, _ in spec])
            out[f"spec/{tag}/{k}/shapes"] = np.asarray([tuple(s) + (0,) * (4 - len(s)) for _, s in spec], np.int64)

    cfg = layoutlmv3_config(**SMALL)
    hf = tr.LayoutLMv3Model(tr.LayoutLMv3Config(**cfg)).eval()
    hf.load_state_dict({k: torch.from_numpy(v) for k, v in make_layoutlmv3_state_dict(cfg, SEED).items()}, strict=True)
    for g in (2, 14):
        out[f"vbox/{g}"] = hf.create_visual_bbox(image_size=(g, g)).numpy()
    heads = {}
    for h, (kind, n) in HEADS.items():
        heads[h] = classes[kind](tr.LayoutLMv3Config(num_labels=n, **cfg)).eval()
        heads[h].load_state_dict({k: torch.from_numpy(v) for k, v in make_layoutlmv3_head_state_dict(cfg, kind, n, SEED).items()}, strict=True)
    grabbed = []
    hf.encoder.register_forward_pre_hook(lambda mod, args: grabbed.append(args[0].detach().float().numpy().copy()))

    def tensors(kw, dtype=None):
        t = {k: torch.from_numpy(v) for k, v in kw.items()}
        if dtype is not None and "pixel_values" in t:
            t["pixel_values"] = t["pixel_values"].to(dtype)
        return t

    inputs = {geo: draw_inputs(cfg, geo) for geo in GEOMETRY}
    for geo, inp in inputs.items():
        out.update({f"{geo}/{k}": v for k, v in inp.items()})
    with torch.no_grad():
        for geo, case in CASES:
            kw, tag = tensors(case_inputs(inputs[geo], case)), f"{geo}/{case}"
            del grabbed[:]
            o = hf(**kw)
            assert len(grabbed) == 1
            out[f"{tag}/embedding_output"] = grabbed[0]
            out[f"{tag}/last_hidden_state"] = o.last_hidden_state.numpy()
            for h in ("token5", "token12", "seq"):
                out[f"{tag}/{h}_logits"] = heads[h](**kw).logits.numpy()
            qa = heads["qa"](**kw)
            out[f"{tag}/start_logits"], out[f"{tag}/end_logits"] = qa.start_logits.numpy(), qa.end_logits.numpy()
            print(tag, "emb |max| %.3f seq |max| %.3f" % tuple(np.abs(out[f"{tag}/{k}"]).max() for k in ("embedding_output", "last_hidden_state")),
                  "shape", out[f"{tag}/last_hidden_state"].shape)
        # transformers' own 16-bit CPU runs against its fp32 run: each a fresh copy of the fp32 model rounded once (`.to` converts in
        # place, so one model taken through both types would carry bf16's weight rounding into fp16)
        fp16_is_bf16 = 0
        hf16 = {name: copy.deepcopy(hf).to(dtype) for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16))}
        assert all(p.dtype == torch.float32 for p in hf.parameters())
        for geo, case in CASES:
            ref = torch.from_numpy(out[f"{geo}/{case}/last_hidden_state"])
            dev = {}
            for name, m16 in hf16.items():
                dtype = next(m16.parameters()).dtype
                try:
                    got = m16(**tensors(case_inputs(inputs[geo], case), dtype)).last_hidden_state.float()
                    dev[name] = float((got - ref).abs().max() / ref.abs().max())
                except RuntimeError as e:
                    print("CPU", name, "failed:", e)
                    fp16_is_bf16 = 1
                    dev[name] = dev["bf16"]
                out[f"dev16/{geo}/{case}/{name}"] = np.asarray(dev[name])
            print(f"{geo}/{case} transformers 16-bit CPU vs fp32: bf16 {dev['bf16']:.3e} fp16 {dev['fp16']:.3e}")
        out["dev16/fp16_is_bf16"] = np.asarray(fp16_is_bf16)
    path = os.path.join(ROOT, "tests", "golden", "layoutlmv3_small.npz")
    np.savez_compressed(path, **out)
    print("layoutlmv3_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
