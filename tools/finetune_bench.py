"""Measure a training step of `EncoderTrainer` beside `HeadTrainer` on one MI355X -> profiles/finetune_bench.json.

bf16 VisualBERT-QA at transformers' default geometry (hidden 768, 12 layers, 20 text + 36 visual tokens of 2048), eager:
ms per step at B = 64 / 256 / 1024 for `HeadTrainer.step` and for `EncoderTrainer.step` with 1, 2 and 12 trained layers; at
B = 1024 the share of each kernel entry (vk_attention_grad, vk_gemm_f32, ...) in a step, by device events around every call
(`vk_add_f32`, the residual adds that `vk_gemm_f32`'s accumulate would have absorbed, is one of them: its share is its cost);
and LayoutLM at 512 tokens, B = 32, one trained layer.  Times are host clock around a device synchronise over `--steps` steps
after `--warmup` steps (the first step of a trainer pays for kernel attributes and the allocator's growth).

In the same job, beside every fp32 `EncoderTrainer` figure, the mixed-precision mode (`compute_dtype=torch.bfloat16`, DESIGN.md
section 28) under the same keys with `_mixed` appended, and each of its kernels alone beside the fp32 kernel it stands in for:
`vk_attention_grad_16` vs `vk_attention_grad` at (B, heads, L, d) = (1024, 12, 56, 64) and (32, 12, 512, 64), `vk_gemm_16` vs
`vk_gemm_f32` in the three forms at a layer's shapes at B = 1024 (57 344 rows; 768 x 3072 and 768 x 768), device events around
`--steps` launches after `--warmup`.  Both modes and the kernel table go to `--mixed-out`; `--out` keeps its columns.

    python tools/finetune_bench.py [--steps 10] [--warmup 3] [--out profiles/finetune_bench.json]
                                   [--mixed-out profiles/finetune_mixed_bench.json]
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


def device_ms(launch, warmup, steps):
    """ms per launch by device events around `steps` launches."""
    for _ in range(warmup):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def kernels_alone(warmup, steps):
    """Each new kernel beside the fp32 kernel it stands in for -> {name: {fp32_ms, bf16_ms, speedup, tflops of both}}."""
    from vltk_amd.train import attention_grad, gemm_16, gemm_f32
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {}
    for B, heads, Lx, d in ((1024, 12, 56, 64), (32, 12, 512, 64)):
        H = heads * d
        qkv, ctx, dctx = (torch.randn((B * Lx, w), device="cuda", generator=g) for w in (3 * H, H, H))
        h16 = [t.to(torch.bfloat16) for t in (qkv, ctx, dctx)]
        t32 = device_ms(lambda: attention_grad(qkv, None, ctx, dctx, B, Lx, heads), warmup, steps)
        t16 = device_ms(lambda: attention_grad(*h16[:1], None, *h16[1:], B, Lx, heads), warmup, steps)      # bf16: vk_attention_grad_16
        flop = 10.0 * B * heads * Lx * Lx * d
        out[f"attention_grad B{B} h{heads} L{Lx} d{d}"] = dict(fp32_ms=round(t32, 3), bf16_ms=round(t16, 3), speedup=round(t32 / t16, 2),
                                                                   fp32_tflops=round(flop / t32 * 1e-9, 2), bf16_tflops=round(flop / t16 * 1e-9, 2))
        del qkv, ctx, dctx, h16
    M = 1024 * 56
    for tag, I, Hd in (("ffn", 3072, 768), ("proj", 768, 768)):
        x, dy, w = (torch.randn(s, device="cuda", generator=g) for s in ((M, Hd), (M, I), (I, Hd)))
        x16, dy16, w16 = (t.to(torch.bfloat16) for t in (x, dy, w))
        forms = {"NT Y = X W^T": (lambda f, a, b, c: f(a, c, trans_b=True), (x, dy, w), (x16, dy16, w16)),
                 "NN dX = dY W": (lambda f, a, b, c: f(b, c), (x, dy, w), (x16, dy16, w16)),
                 "TN dW = dY^T X": (lambda f, a, b, c: f(b, a, trans_a=True), (x, dy, w), (x16, dy16, w16))}
        for name, (call, a32, a16) in forms.items():
            t32 = device_ms(lambda: call(gemm_f32, *a32), warmup, steps)
            t16 = device_ms(lambda: call(gemm_16, *a16), warmup, steps)
            flop = 2.0 * M * I * Hd
            out[f"gemm {tag} {M}x{I}x{Hd} {name}"] = dict(fp32_ms=round(t32, 3), bf16_ms=round(t16, 3), speedup=round(t32 / t16, 2),
                                                          fp32_tflops=round(flop / t32 * 1e-9, 1), bf16_tflops=round(flop / t16 * 1e-9, 1))
        del x, dy, w, x16, dy16, w16
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.json"))
    ap.add_argument("--mixed-out", default=os.path.join(ROOT, "profiles", "finetune_mixed_bench.json"))
    a = ap.parse_args()
    r = np.random.Generator(np.random.PCG64(0))
    mixed = {"device": torch.cuda.get_device_name(0), "precision": "bf16", "compute_dtype": "bfloat16", "steps": a.steps, "warmup": a.warmup,
             "visualbert": {}, "layoutlm": {}}
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
        both = {k: v for k, v in row.items() if k != "head_trainer_ms"}
        for n in (1, 2, 12):
            tr = EncoderTrainer(model, sd, train_layers=n, max_grad_norm=5.0, compute_dtype=torch.bfloat16)
            step = lambda: tr.step(ids, feats, labels=labels, attention_mask=am)          # noqa: E731
            both[f"encoder_trainer_n{n}_ms_mixed"] = round(ms_per_step(step, a.warmup, a.steps), 3)
            if B == 1024:
                both[f"encoder_trainer_n{n}_shares_mixed"], both[f"encoder_trainer_n{n}_device_ms_mixed"] = shares(step)
            del tr
            torch.cuda.empty_cache()
        mixed["visualbert"][f"B{B}"] = both
        print(json.dumps({f"B{B} mixed": {k: v for k, v in both.items() if k.endswith("_mixed")}}), flush=True)
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
    del tr
    tr = EncoderTrainer(model, sd, train_layers=1, max_grad_norm=5.0, compute_dtype=torch.bfloat16)
    both = dict(row)
    both["encoder_trainer_n1_ms_mixed"] = round(ms_per_step(step, a.warmup, a.steps), 3)
    both["encoder_trainer_n1_shares_mixed"], both["encoder_trainer_n1_device_ms_mixed"] = shares(step)
    mixed["layoutlm"]["B32_L512"] = both
    print(json.dumps({"layoutlm B32 L512 mixed": {k: v for k, v in both.items() if k.endswith("_mixed")}}), flush=True)
    del tr, model
    torch.cuda.empty_cache()
    mixed["kernels"] = kernels_alone(a.warmup, a.steps)
    print(json.dumps({"kernels": mixed["kernels"]}), flush=True)
    with open(a.mixed_out, "w") as f:
        json.dump(mixed, f, indent=1)
        f.write("\n")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
