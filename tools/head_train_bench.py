#!/usr/bin/env python3
"""What training LXMERT's answer head over the frozen encoder costs on one MI355X: bf16 encoder, transformers' default geometry
(hidden 768, 3129 answers, 20 text tokens, 36 boxes), B = 64 / 256 / 1024, all in one job:

  encoder_ms         the frozen forward alone (`model.head_features`)
  step_ms            `HeadTrainer.step`: that forward, then the head's forward, loss, backward and AdamW step in fp32
  step_features_ms   `HeadTrainer.step_features` alone, on cached features
  gemm               `vk_gemm_f32` alone at the head's six GEMM shapes, by device events: 2 M N K / time in TFLOP/s, beside the
                     instruction's 157.3 TFLOP/s peak.  The sixth, fc0's dX, is what an encoder backward would take next; a step
                     over a frozen encoder does not run it.
  adamw              `vk_adamw_step` alone over the head's six tensors: 28 bytes per element (p, g, m, v read; p, m, v written)
                     / time in GB/s, beside the card's HBM rate (8.0 TB/s peak, about 6.3 TB/s reached by a plain copy)

usage: python tools/head_train_bench.py [--batches 64,256,1024] [--out profiles/head_train_bench.json]

The work runs in one child process under a time limit; a child that fails or runs out of time ends the job.  Call times are a
host clock around a device synchronise, warmed up, over >= 0.5 s of work; kernel times are device events around 50 launches.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from visualbert_bench import timed  # noqa: E402

TEXT_TOKENS, BOXES, ANSWERS = 20, 36, 3129
F32_MFMA_PEAK_TFLOPS, HBM_PEAK_TBS, HBM_COPY_TBS = 157.3, 8.0, 6.3


def head_gemms(B, H, N):
    """(name, form, M, N, K) of the head's GEMMs at batch B, hidden H, N answers."""
    return [("fc0 forward", "NT", B, 2 * H, H), ("fc3 forward", "NT", B, N, 2 * H), ("fc3 dW", "TN", N, 2 * H, B),
            ("fc3 dX", "NN", B, 2 * H, N), ("fc0 dW", "TN", 2 * H, H, B), ("fc0 dX", "NN", B, H, 2 * H)]


def child(batches):
    import numpy as np
    import torch
    from vltk_amd import train as T
    from vltk_amd.lxmert import LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict

    sync = torch.cuda.synchronize
    gen = np.random.Generator(np.random.PCG64(0))
    cfg = lxmert_config()
    H, D = cfg["hidden_size"], cfg["visual_feat_dim"]
    model = LxmertForQuestionAnswering(cfg, ANSWERS, precision="bf16").load_state_dict(make_lxmert_qa_state_dict(cfg, ANSWERS, 1))

    def events(fn, reps=50):
        fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    out = dict(text_tokens=TEXT_TOKENS, boxes=BOXES, hidden=H, answers=ANSWERS, batches={})
    for B in batches:
        ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, TEXT_TOKENS))).cuda()
        feats = torch.from_numpy(np.maximum(gen.standard_normal((B, BOXES, D)), 0).astype(np.float32)).cuda().bfloat16()
        pos = torch.from_numpy(gen.uniform(0, 1, (B, BOXES, 4)).astype(np.float32)).cuda().bfloat16()
        labels = gen.integers(0, ANSWERS, B)
        labels[::9] = -100
        tr = T.HeadTrainer(model, lr=1e-4, schedule=T.step_lr(200, 0.9))
        r = {}
        t, n = timed(lambda: model.head_features(ids, feats, pos), sync)
        r["encoder_ms"], r["calls_timed"] = round(t * 1e3, 3), n
        t, _ = timed(lambda: tr.step(ids, feats, pos, labels=labels), sync)
        r["step_ms"] = round(t * 1e3, 3)
        pooled = model.head_features(ids, feats, pos)
        t, n = timed(lambda: tr.step_features(pooled, labels), sync)
        r["step_features_ms"], r["step_features_calls_timed"] = round(t * 1e3, 3), n
        r["loss_after"], r["steps_taken"] = float(tr.step_features(pooled, labels)), tr.steps
        r["gemm"], flops = [], 0.0
        for name, form, M, N, K in head_gemms(B, H, ANSWERS):
            ta, tb = form[0] == "T", form[1] == "T"
            a = torch.empty((K, M) if ta else (M, K), dtype=torch.float32, device="cuda").normal_()
            b = torch.empty((N, K) if tb else (K, N), dtype=torch.float32, device="cuda").normal_()
            c = torch.empty((M, N), dtype=torch.float32, device="cuda")
            ms = events(lambda: T.gemm_f32(a, b, out=c, trans_a=ta, trans_b=tb))
            r["gemm"].append(dict(name=name, form=form, M=M, N=N, K=K, us=round(ms * 1e3, 2), tflops=round(2.0 * M * N * K / ms / 1e9, 2)))
            if name != "fc0 dX":
                flops += 2.0 * M * N * K
        r["head_gemm_gflop_per_step"] = round(flops / 1e9, 2)
        n_el = sum(t.numel() for t in tr.p.values())
        ms = events(lambda: T.adamw_step(tr._table, len(tr.keys), tr._max_n, 1e-4, tr.betas, tr.eps, tr.weight_decay, 10, tr.device))
        r["adamw"] = dict(elements=n_el, tensors=len(tr.keys), us=round(ms * 1e3, 2), gb_per_s=round(28.0 * n_el / ms / 1e6, 1))
        out["batches"][str(B)] = r
        del tr, a, b, c
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_bench.json"))
    ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if a.child:
        return child(batches)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batches", a.batches]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired as e:
        sys.exit(f"no result within {a.child_timeout:.0f} s; stopping\n{e.stdout or ''}")
    if p.returncode != 0:
        sys.exit(f"exit status {p.returncode}; stopping\n{p.stdout[-4000:]}")
    r = [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")][0]
    for B, v in r["batches"].items():
        print(f"B={B}: encoder {v['encoder_ms']:.2f} ms | step {v['step_ms']:.2f} ms | step_features {v['step_features_ms']:.3f} ms | "
              f"adamw {v['adamw']['us']:.1f} us = {v['adamw']['gb_per_s']:.0f} GB/s")
        for g in v["gemm"]:
            print(f"    {g['name']:12s} {g['form']} {g['M']:5d} x {g['N']:5d} x {g['K']:5d}  {g['us']:8.1f} us  {g['tflops']:7.2f} TFLOP/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/head_train_bench.py", device="MI355X (gfx950), one GPU", encoder_precision="bf16", head_precision="fp32",
                       f32_mfma_peak_tflops=F32_MFMA_PEAK_TFLOPS, hbm_peak_tb_per_s=HBM_PEAK_TBS, hbm_copy_tb_per_s=HBM_COPY_TBS, result=r),
                  f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
