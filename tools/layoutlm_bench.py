#!/usr/bin/env python3
"""Forward time of the LayoutLM encoder on one MI355X, bf16, 512-token pages, with VisualBERT at B = 1024 / 36 boxes in the
same job as the number to read it beside.

usage: python tools/layoutlm_bench.py [--batches 8 32 128] [--tokens 512] [--out profiles/layoutlm_bench.json]

Geometry: transformers' LayoutLMConfig defaults (12 layers, hidden 768, 12 heads, 1024-row 2-D position tables).  Each model
runs in a child process of its own under a time limit; a child that fails or runs out of time ends the job (nothing more is
started on the GPU).  Per batch: eager and replayed-graph forward time (host clock around a device synchronise, warmed up,
>= 0.5 s of work), examples/s, algorithmic TFLOP/s, and by device events around those launches alone, same shapes: the
embedding stage (vk_layoutlm_embed and the mask), one layer's attention, the word vote (vk_token_word_labels: 7 labels, three
tokens per word) and the span decode (vk_span_select: answers of up to 30 tokens, every token in the context).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from visualbert_bench import TEXT_TOKENS, timed, visualbert_gflop  # noqa: E402

NUM_LABELS = 7
TOKENS_PER_WORD = 3
MAX_ANSWER = 30


def layoutlm_gflop(cfg, B, Lt):
    """Per example layers * (2 L (4 H^2 + 2 H I) + 4 L^2 H): the four H x H and two H x I products of a BERT layer (2 FLOP per
    MAC) and the two L x L x H products of its attention; the pooler and the heads are left out."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    return B * cfg["num_hidden_layers"] * (2 * Lt * (4 * H * H + 2 * H * I) + 4 * Lt * Lt * H) / 1e9


def record(model, B, gf, eager, graph, n, **more):
    return dict(model=model, B=B, precision="bf16", algorithmic_gflop=round(gf, 1), calls_timed=n, eager_ms=round(eager * 1e3, 3),
                eager_examples_per_s=round(B / eager), eager_tflops=round(gf / eager / 1e3, 1), graph_ms=round(graph * 1e3, 3),
                graph_examples_per_s=round(B / graph), graph_tflops=round(gf / graph / 1e3, 1), **more)


def child_layoutlm(batches, Lt):
    import numpy as np
    import torch
    from vltk_amd import _lib as L
    from vltk_amd.layers import stream
    from vltk_amd.layoutlm import LayoutLMModel, layoutlm_config, make_layoutlm_state_dict

    sync = torch.cuda.synchronize
    gen = np.random.Generator(np.random.PCG64(0))
    cfg = layoutlm_config()
    m = LayoutLMModel(cfg, precision="bf16").load_state_dict(make_layoutlm_state_dict(cfg, 1))
    H, dev = cfg["hidden_size"], m.device

    def events(fn, reps=20):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps
    for B in batches:
        ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, Lt))).cuda()
        xs, ys = np.sort(gen.integers(0, 1001, (B, Lt, 2)), -1), np.sort(gen.integers(0, 1001, (B, Lt, 2)), -1)
        bbox = torch.from_numpy(np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)).cuda()
        mask = torch.ones((B, Lt), device=dev)
        args = (ids, bbox, mask)
        gf = layoutlm_gflop(cfg, B, Lt)
        eager, n = timed(lambda: m(*args), sync)
        replay = m.capture(*args)
        graph, _ = timed(lambda: replay(*args), sync)
        # the stages this model brings in or leans on, alone
        x, amask = m._embed(ids, bbox, mask, None)
        qkv = m._linear(x, "encoder.layer.0.attention.self.qkv")
        _, route = m.attention_entry(Lt, Lt, 3 * H, 3 * H, 3 * H, 1)
        emb_ms = events(lambda: m._embed(ids, bbox, mask, None))
        att_ms = events(lambda: m._attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], amask, B, Lt, Lt))
        W = Lt // TOKENS_PER_WORD
        logits = torch.from_numpy(gen.standard_normal((B, Lt, 8)).astype(np.float32)).cuda().bfloat16()
        wid = torch.from_numpy(np.tile(np.minimum(np.arange(Lt) // TOKENS_PER_WORD, W - 1).astype(np.int32), (B, 1))).cuda()
        tok = torch.empty((B, Lt), dtype=torch.int32, device=dev)
        words = torch.empty((B, W), dtype=torch.int32, device=dev)
        vote_ms = events(lambda: L.call("vk_token_word_labels", logits.data_ptr(), 8, wid.data_ptr(), B, Lt, NUM_LABELS, W, tok.data_ptr(),
                                        words.data_ptr(), m.dt, stream(dev)))
        ctx = torch.ones((B, Lt), dtype=torch.int32, device=dev)
        s, e = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        sc = torch.empty((B,), dtype=torch.float32, device=dev)
        span_ms = events(lambda: L.call("vk_span_select", logits.data_ptr(), 8, logits.data_ptr() + 2, 8, ctx.data_ptr(), B, Lt, MAX_ANSWER,
                                        s.data_ptr(), e.data_ptr(), sc.data_ptr(), m.dt, stream(dev)))
        rec = record("layoutlm", B, gf, eager, graph, n, tokens=Lt, attention_route=("mfma", "lds", "tiled", "stream")[route],
                     embed_stage_ms=round(emb_ms, 4), attention_ms_per_layer=round(att_ms, 4),
                     embed_stage_share_of_graph=round(emb_ms / (graph * 1e3), 4),
                     attention_share_of_graph=round(att_ms * cfg["num_hidden_layers"] / (graph * 1e3), 4),
                     word_vote_ms=round(vote_ms, 4), words_per_example=W, labels=NUM_LABELS,
                     span_select_ms=round(span_ms, 4), max_answer_tokens=MAX_ANSWER)
        print("RESULT " + json.dumps(rec), flush=True)


def child_visualbert(B, V):
    import numpy as np
    import torch
    from vltk_amd.visualbert import VisualBertModel, make_visualbert_state_dict, visualbert_config

    sync = torch.cuda.synchronize
    gen = np.random.Generator(np.random.PCG64(0))
    cfg = visualbert_config(visual_embedding_dim=2048)
    m = VisualBertModel(cfg, precision="bf16").load_state_dict(make_visualbert_state_dict(cfg, 1))
    ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, TEXT_TOKENS))).cuda()
    feats = torch.from_numpy(np.maximum(gen.standard_normal((B, V, 2048)), 0).astype(np.float32)).cuda().bfloat16()
    eager, n = timed(lambda: m(ids, feats), sync)
    replay = m.capture(ids, feats)
    graph, _ = timed(lambda: replay(ids, feats), sync)
    print("RESULT " + json.dumps(record("visualbert", B, visualbert_gflop(cfg, B, TEXT_TOKENS, V), eager, graph, n,
                                        text_tokens=TEXT_TOKENS, boxes=V)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--yardstick", type=int, nargs=2, default=[1024, 36], metavar=("B", "V"), help="the VisualBERT run beside it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layoutlm_bench.json"))
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds one child may take")
    ap.add_argument("--child", choices=("layoutlm", "visualbert"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "layoutlm":
        return child_layoutlm(a.batches, a.tokens)
    if a.child == "visualbert":
        return child_visualbert(*a.yardstick)
    results = []
    for model in ("layoutlm", "visualbert"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", model, "--tokens", str(a.tokens), "--yardstick"] + \
              [str(v) for v in a.yardstick] + ["--batches"] + [str(b) for b in a.batches]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired as e:
            sys.exit(f"{model}: no result within {a.child_timeout:.0f} s; stopping\n{e.stdout or ''}")
        if p.returncode != 0:
            sys.exit(f"{model}: exit status {p.returncode}; stopping\n{p.stdout[-4000:]}")
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                results.append(r)
                print(f"{r['model']:10s} B={r['B']:5d}: eager {r['eager_ms']:8.2f} ms {r['eager_examples_per_s']:8d} ex/s {r['eager_tflops']:6.1f} TFLOP/s"
                      f" | graph {r['graph_ms']:8.2f} ms {r['graph_examples_per_s']:8d} ex/s {r['graph_tflops']:6.1f} TFLOP/s" +
                      (f" | embed {r['embed_stage_ms']:.3f} ms attention ({r['attention_route']}) {100 * r['attention_share_of_graph']:.1f} %"
                       f" vote {r['word_vote_ms']:.3f} ms span {r['span_select_ms']:.3f} ms" if "word_vote_ms" in r else ""), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/layoutlm_bench.py", device="MI355X (gfx950), one GPU", precision="bf16", tokens=a.tokens,
                       flop_model="per example layers*(2L(4H^2+2HI)+4L^2H); L = tokens (LayoutLM), L = 20 + V (VisualBERT)",
                       results=results), f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
