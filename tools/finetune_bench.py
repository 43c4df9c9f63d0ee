"""Measure a training step of `EncoderTrainer` beside `HeadTrainer` on one MI355X -> profiles/finetune_bench.json.

bf16 VisualBERT-QA at transformers' default geometry (hidden 768, 12 layers, 20 text + 36 visual tokens of 2048), eager:
ms per step at B = 64 / 256 / 1024 for `HeadTrainer.step` and for `EncoderTrainer.step` with 1, 2 and 12 trained layers; at
B = 1024 the share of each kernel entry (vk_attention_grad, vk_gemm_f32, ...) in a step, by device events around every call
(`vk_add_f32`, the residual adds that `vk_gemm_f32`'s accumulate would have absorbed, is one of them: its share is its cost);
and LayoutLM at 512 tokens, B = 32, one trained layer.  Times are host clock around a device synchronise over `--steps` steps
after `--warmup` steps (the first step of a trainer pays for kernel attributes and the allocator's growth).

    python tools/finetune_bench.py [--steps 10] [--warmup 3] [--out profiles/finetune_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vltk_amd import EncoderTrainer, HeadTrainer                                         # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.layoutlm import LayoutLMForSequenceClassification, layoutlm_config, make_layoutlm_head_state_dict      # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering, make_visualbert_qa_state_dict, visualbert_config     # noqa: E402


def ms_per_step(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def shares(step):
    """One step with a pair of device events around every call into the library -> {entry: share of the summed device time}."""
    real, spans = L.call, []

    def timed(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *a)
        e1.record()
        spans.append((name, e0, e1))
    L.call = timed
    try:
        step()
    finally:
        L.call = real
    torch.cuda.synchronize()
    by = {}
    for name, e0, e1 in spans:
        by[name] = by.get(name, 0.0) + e0.elapsed_time(e1)
    total = sum(by.values())
    return {k: round(v / total, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])}, round(total, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.json"))
    a = ap.parse_args()
    r = np.random.Generator(np.random.PCG64(0))
    res = {"device": torch.cuda.get_device_name(0), "precision": "bf16", "steps": a.steps, "warmup": a.warmup, "visualbert": {}, "layoutlm": {}}

    cfg, labels_n, Lt, V = visualbert_config(visual_embedding_dim=2048), 3129, 20, 36
    sd = make_visualbert_qa_state_dict(cfg, labels_n, seed=0)
    model = VisualBertForQuestionAnswering(cfg, labels_n, precision="bf16").load_state_dict(sd)
    for B in (64, 256, 1024):
        ids = torch.from_numpy(r.integers(1, cfg["vocab_size"], (B, Lt)))
        feats = torch.from_numpy(np.maximum(r.standard_normal((B, V, 2048)), 0).astype(np.float32)).cuda()
        am = torch.ones((B, Lt), dtype=torch.int64)
        labels = r.integers(0, labels_n, B).astype(np.int64)
        row = {}
        head = HeadTrainer(model)
        row["head_trainer_ms"] = round(ms_per_step(lambda: head.step(ids, feats, labels=labels, attention_mask=am), a.warmup, a.steps), 3)
        for n in (1, 2, 12):
            tr = EncoderTrainer(model, sd, train_layers=n, max_grad_norm=5.0)
            step = lambda: tr.step(ids, feats, labels=labels, attention_mask=am)          # noqa: E731
            row[f"encoder_trainer_n{n}_ms"] = round(ms_per_step(step, a.warmup, a.steps), 3)
            if B == 1024:
                row[f"encoder_trainer_n{n}_shares"], row[f"encoder_trainer_n{n}_device_ms"] = shares(step)
            del tr
            torch.cuda.empty_cache()
        res["visualbert"][f"B{B}"] = row
        print(json.dumps({f"B{B}": row}), flush=True)
    del model, sd

    cfg = layoutlm_config()
    sd = make_layoutlm_head_state_dict(cfg, "classifier", 16, seed=0)
    model = LayoutLMForSequenceClassification(cfg, 16, precision="bf16").load_state_dict(sd)
    B, Lt = 32, 512
    ids = torch.from_numpy(r.integers(1, cfg["vocab_size"], (B, Lt)))
    labels = r.integers(0, 16, B).astype(np.int64)
    tr = EncoderTrainer(model, sd, train_layers=1, max_grad_norm=5.0)
    step = lambda: tr.step(ids, labels=labels)                                            # noqa: E731
    row = {"encoder_trainer_n1_ms": round(ms_per_step(step, a.warmup, a.steps), 3)}
    row["encoder_trainer_n1_shares"], row["encoder_trainer_n1_device_ms"] = shares(step)
    res["layoutlm"]["B32_L512"] = row
    print(json.dumps({"layoutlm B32 L512": row}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
