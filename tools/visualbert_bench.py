#!/usr/bin/env python3
"""Forward time of the single-stream VisualBERT encoder on one MI355X, bf16, with LxmertEncoder at the same batch and box
count in the same job as the number to read it beside.

usage: python tools/visualbert_bench.py [--batches 32 256 1024] [--boxes 36 100] [--out profiles/visualbert_bench.json]

Geometry: transformers' VisualBertConfig defaults (12 layers, hidden 768, 12 heads) with this extractor's 2048-wide features,
20 text tokens + V boxes per example.  Each (model, V) runs in a child process of its own under a time limit; a child that
fails or runs out of time ends the job (nothing more is started on the GPU).  Per configuration: eager and replayed-graph
forward time (host clock around a device synchronise, warmed up, >= 0.5 s of work), examples/s, algorithmic TFLOP/s, and for
VisualBERT the share of one forward spent in the embedding kernel and in the attention kernel (device events around those
launches alone, same shapes).
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
TEXT_TOKENS = 20


def visualbert_gflop(cfg, B, Lt, V):
    """Per example layers * (2 L (4 H^2 + 2 H I) + 4 L^2 H), L = Lt + V: the four H x H and two H x I products of a BERT layer
    (2 FLOP per MAC) and the two L x L x H products of its attention; the visual projection and the pooler are left out."""
    H, I, Lx = cfg["hidden_size"], cfg["intermediate_size"], Lt + V
    return B * cfg["num_hidden_layers"] * (2 * Lx * (4 * H * H + 2 * H * I) + 4 * Lx * Lx * H) / 1e9


def timed(fn, sync, min_seconds=0.5):
    """Mean seconds per call over a window of at least `min_seconds` (and at least 5 calls), after two warm-up calls."""
    for _ in range(2):
        fn()
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    n = max(5, int(math.ceil(min_seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n, n


def child(model, V, batches):
    import numpy as np
    import torch
    from lxmert_bench import gflop as lxmert_gflop
    from vltk_amd.lxmert import LxmertEncoder, lxmert_config, make_lxmert_state_dict
    from vltk_amd.visualbert import VisualBertModel, make_visualbert_state_dict, visualbert_config

    sync = torch.cuda.synchronize
    gen = np.random.Generator(np.random.PCG64(0))
    if model == "visualbert":
        cfg = visualbert_config(visual_embedding_dim=2048)
        m = VisualBertModel(cfg, precision="bf16").load_state_dict(make_visualbert_state_dict(cfg, 1))
    else:
        cfg = lxmert_config()
        m = LxmertEncoder(cfg, precision="bf16").load_state_dict(make_lxmert_state_dict(cfg, 1))
    for B in batches:
        ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, TEXT_TOKENS))).cuda()
        feats = torch.from_numpy(np.maximum(gen.standard_normal((B, V, 2048)), 0).astype(np.float32)).cuda().bfloat16()
        args = (ids, feats) if model == "visualbert" else (ids, feats, torch.from_numpy(gen.uniform(0, 1, (B, V, 4)).astype(np.float32)).cuda().bfloat16())
        gf = visualbert_gflop(cfg, B, TEXT_TOKENS, V) if model == "visualbert" else lxmert_gflop(cfg, B, TEXT_TOKENS, V)
        eager, n = timed(lambda: m(*args), sync)
        replay = m.capture(*args)
        graph, _ = timed(lambda: replay(*args), sync)
        rec = dict(model=model, B=B, text_tokens=TEXT_TOKENS, boxes=V, precision="bf16", algorithmic_gflop=round(gf, 1), calls_timed=n,
                   eager_ms=round(eager * 1e3, 3), eager_examples_per_s=round(B / eager), eager_tflops=round(gf / eager / 1e3, 1),
                   graph_ms=round(graph * 1e3, 3), graph_examples_per_s=round(B / graph), graph_tflops=round(gf / graph / 1e3, 1))
        if model == "visualbert":                        # the two kernels this model brings in or leans on, alone, by device events
            Lx, H = TEXT_TOKENS + V, cfg["hidden_size"]
            none5 = (None,) * 5
            x, mask = m._embed(ids, feats, *none5)
            qkv = m._linear(x, "encoder.layer.0.attention.self.qkv")
            _, route = m.attention_entry(Lx, Lx, 3 * H, 3 * H, 3 * H, 1)

            def events(fn, reps=20):
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                sync()
                return e0.elapsed_time(e1) / reps
            emb_ms = events(lambda: m._embed(ids, feats, *none5))      # visual projection GEMM + mask + the embedding kernel
            att_ms = events(lambda: m._attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask, B, Lx, Lx))
            rec.update(attention_route=("mfma", "lds", "tiled", "stream")[route], embed_stage_ms=round(emb_ms, 4),
                       attention_ms_per_layer=round(att_ms, 4),
                       embed_stage_share_of_graph=round(emb_ms / (graph * 1e3), 4),
                       attention_share_of_graph=round(att_ms * cfg["num_hidden_layers"] / (graph * 1e3), 4))
        print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256, 1024])
    ap.add_argument("--boxes", type=int, nargs="+", default=[36, 100])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visualbert_bench.json"))
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds one (model, V) child may take")
    ap.add_argument("--child", nargs=2, metavar=("MODEL", "V"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.batches)
    results = []
    for V in a.boxes:
        for model in ("visualbert", "lxmert"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", model, str(V), "--batches"] + [str(b) for b in a.batches]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired as e:
                sys.exit(f"{model} V={V}: no result within {a.child_timeout:.0f} s; stopping\n{e.stdout or ''}")
            if p.returncode != 0:
                sys.exit(f"{model} V={V}: exit status {p.returncode}; stopping\n{p.stdout[-4000:]}")
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    results.append(r)
                    print(f"{r['model']:10s} B={r['B']:5d} V={r['boxes']:3d}: eager {r['eager_ms']:8.2f} ms {r['eager_examples_per_s']:8d} ex/s"
                          f" {r['eager_tflops']:6.1f} TFLOP/s | graph {r['graph_ms']:8.2f} ms {r['graph_examples_per_s']:8d} ex/s"
                          f" {r['graph_tflops']:6.1f} TFLOP/s" + (f" | embed stage {100 * r['embed_stage_share_of_graph']:.1f} %"
                                                                  f" attention ({r['attention_route']}) {100 * r['attention_share_of_graph']:.1f} %"
                                                                  if "attention_route" in r else ""), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/visualbert_bench.py", device="MI355X (gfx950), one GPU", precision="bf16", text_tokens=TEXT_TOKENS,
                       flop_model="per example layers*(2L(4H^2+2HI)+4L^2H), L=20+V (VisualBERT); tools/lxmert_bench.py gflop (LXMERT)",
                       results=results), f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
