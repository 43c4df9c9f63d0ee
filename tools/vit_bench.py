#!/usr/bin/env python3
"""Forward time of the ViT-B/16 image encoder on one MI355X, bf16, and of images -> ViT -> VisualBertForQuestionAnswering.

usage: python tools/vit_bench.py [--out profiles/vit_bench.json]

Encoder: B = 32 and 256 at 224 x 224 (197 tokens), B = 32 at 384 x 384 with interpolated positions (577 tokens).  Per
configuration: eager and replayed-graph forward time (host clock around a device synchronise, warmed up, >= 0.5 s of work),
images/s, algorithmic TFLOP/s, and the share of one forward spent in the embedding stage and in its two new kernels
(vk_vit_patchify, vk_vit_assemble; device events around those launches alone, same shapes).
Pipeline: 256 images of 224 x 224 -> ViT-B/16 -> the 196 patch tokens as `visual_embeds` of a default-geometry
VisualBertForQuestionAnswering (20 text tokens, 3129 answers), eager, beside the records profiles/visualbert_bench.json holds for
that encoder fed with 36 and 100 region features at the same batch.
Each part runs in a child process of its own under a time limit; a child that fails or runs out of time ends the job (nothing
more is started on the GPU).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ENCODER_CASES = [(32, 224, False), (256, 224, False), (32, 384, True)]       # B, image side, interpolate_pos_encoding
TEXT_TOKENS, PIPELINE_B, NUM_ANSWERS = 20, 256, 3129
VISUALBERT_TFLOPS_B1024 = 599.0          # profiles/visualbert_bench.json: VisualBERT, B = 1024, 20 + 36 tokens, replayed graph


def vit_gflop(cfg, B, side):
    """Per image layers * (2 L (4 H^2 + 2 H I) + 4 L^2 H) with L = 1 + (side / P)^2, plus the patch projection 2 N (C P^2) H;
    the pooler is left out.  -> (total, embedding stage alone)."""
    H, I, P, C = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"], cfg["num_channels"]
    N = (side // P) ** 2
    Lx = N + 1
    emb = 2 * N * C * P * P * H
    return B * (cfg["num_hidden_layers"] * (2 * Lx * (4 * H * H + 2 * H * I) + 4 * Lx * Lx * H) + emb) / 1e9, B * emb / 1e9


def events(fn, sync, reps=20):
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1) / reps


def child_encoder():
    import numpy as np
    import torch
    from visualbert_bench import timed
    from vltk_amd import _lib as L
    from vltk_amd.layers import stream
    from vltk_amd.vit import ViTModel, make_vit_state_dict, vit_config

    sync = torch.cuda.synchronize
    cfg = vit_config()
    m = ViTModel(cfg, precision="bf16").load_state_dict(make_vit_state_dict(cfg, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    H, P, C = cfg["hidden_size"], cfg["patch_size"], cfg["num_channels"]
    for B, side, interp in ENCODER_CASES:
        pix = torch.from_numpy(gen.standard_normal((B, C, side, side)).astype(np.float32)).cuda()
        gf, gf_emb = vit_gflop(cfg, B, side)
        eager, n = timed(lambda: m(pix, interpolate_pos_encoding=interp), sync)
        replay = m.capture(pix, interpolate_pos_encoding=interp)
        graph, _ = timed(lambda: replay(pix), sync)
        N = (side // P) ** 2
        Lx = N + 1
        _, route = m.attention_entry(Lx, Lx, 3 * H, 3 * H, 3 * H, 1)
        # the embedding stage (patch rows + projection GEMM + assembly) and its two new kernels alone
        Kp = m._lin[m._PROJ][3]
        rows = torch.empty((B * N, Kp), dtype=m.tdt, device=m.device)
        x = torch.empty((B * Lx, H), dtype=m.tdt, device=m.device)
        pos = m.position_table(side // P, side // P)
        proj = m._linear(rows, m._PROJ)
        emb_ms = events(lambda: m._embed(pix), sync)
        pat_ms = events(lambda: L.call("vk_vit_patchify", pix.data_ptr(), B, C, side, side, P, rows.data_ptr(), Kp, m.dt, stream(m.device)), sync)
        asm_ms = events(lambda: L.call("vk_vit_assemble", proj.data_ptr(), proj.stride(0), m._cls.data_ptr(), pos.data_ptr(), B, N,
                                       x.data_ptr(), H, m.dt, stream(m.device)), sync)
        pat_bytes, asm_bytes = pix.numel() * 4 + rows.numel() * 2, (proj.numel() + x.numel()) * 2
        rec = dict(part="encoder", model="ViT-B/16", B=B, image=side, tokens=Lx, interpolate_pos_encoding=interp, precision="bf16",
                   algorithmic_gflop=round(gf, 1), embedding_stage_gflop=round(gf_emb, 1), calls_timed=n,
                   eager_ms=round(eager * 1e3, 3), eager_images_per_s=round(B / eager), eager_tflops=round(gf / eager / 1e3, 1),
                   graph_ms=round(graph * 1e3, 3), graph_images_per_s=round(B / graph), graph_tflops=round(gf / graph / 1e3, 1),
                   graph_tflops_vs_visualbert_b1024=round(gf / graph / 1e3 / VISUALBERT_TFLOPS_B1024, 3),
                   attention_route=("mfma", "lds", "tiled", "stream")[route],
                   embed_stage_ms=round(emb_ms, 4), patchify_ms=round(pat_ms, 4), assemble_ms=round(asm_ms, 4),
                   patchify_gb_per_s=round(pat_bytes / pat_ms / 1e6, 1), assemble_gb_per_s=round(asm_bytes / asm_ms / 1e6, 1),
                   embed_stage_share_of_graph=round(emb_ms / (graph * 1e3), 4),
                   new_kernels_share_of_graph=round((pat_ms + asm_ms) / (graph * 1e3), 4))
        print("RESULT " + json.dumps(rec), flush=True)
        del replay, pix, rows, x, proj


def child_pipeline():
    import numpy as np
    import torch
    from visualbert_bench import timed, visualbert_gflop
    from vltk_amd.visualbert import VisualBertForQuestionAnswering, make_visualbert_qa_state_dict, visualbert_config
    from vltk_amd.vit import ViTModel, make_vit_state_dict, patch_tokens, vit_config

    sync = torch.cuda.synchronize
    cfg = vit_config()
    vit = ViTModel(cfg, precision="bf16").load_state_dict(make_vit_state_dict(cfg, 1))
    vcfg = visualbert_config(visual_embedding_dim=cfg["hidden_size"])
    qa = VisualBertForQuestionAnswering(vcfg, NUM_ANSWERS, precision="bf16").load_state_dict(make_visualbert_qa_state_dict(vcfg, NUM_ANSWERS, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    B, side = PIPELINE_B, cfg["image_size"]
    pix = torch.from_numpy(gen.standard_normal((B, 3, side, side)).astype(np.float32)).cuda()
    ids = torch.from_numpy(gen.integers(1, vcfg["vocab_size"], (B, TEXT_TOKENS))).cuda()
    V = (side // cfg["patch_size"]) ** 2

    def step():
        seq, _ = vit(pix)
        return qa(ids, patch_tokens(seq))
    logits = step()
    assert logits.shape == (B, NUM_ANSWERS) and bool(torch.isfinite(logits.float()).all())
    total, n = timed(step, sync)
    vit_s, _ = timed(lambda: vit(pix), sync)
    gf = vit_gflop(cfg, B, side)[0] + visualbert_gflop(vcfg, B, TEXT_TOKENS, V)
    rec = dict(part="pipeline", pipeline="images -> ViT-B/16 -> VisualBertForQuestionAnswering", B=B, image=side, text_tokens=TEXT_TOKENS,
               visual_tokens=V, precision="bf16", mode="eager", calls_timed=n, algorithmic_gflop=round(gf, 1),
               step_ms=round(total * 1e3, 3), images_per_s=round(B / total), tflops=round(gf / total / 1e3, 1),
               vit_ms=round(vit_s * 1e3, 3), visualbert_qa_ms=round((total - vit_s) * 1e3, 3))
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_bench.json"))
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds one child may take")
    ap.add_argument("--child", choices=["encoder", "pipeline"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_encoder() if a.child == "encoder" else child_pipeline()
    results = []
    for part in ("encoder", "pipeline"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired as e:
            sys.exit(f"{part}: no result within {a.child_timeout:.0f} s; stopping\n{e.stdout or ''}")
        if p.returncode != 0:
            sys.exit(f"{part}: exit status {p.returncode}; stopping\n{p.stdout[-4000:]}")
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                results.append(r)
                if part == "encoder":
                    print(f"ViT-B/16 B={r['B']:4d} {r['image']}^2 ({r['tokens']} tokens, {r['attention_route']}): eager {r['eager_ms']:8.2f} ms"
                          f" {r['eager_images_per_s']:7d} img/s {r['eager_tflops']:6.1f} TFLOP/s | graph {r['graph_ms']:8.2f} ms"
                          f" {r['graph_images_per_s']:7d} img/s {r['graph_tflops']:6.1f} TFLOP/s | embed stage"
                          f" {100 * r['embed_stage_share_of_graph']:.2f} % (patchify + assemble {100 * r['new_kernels_share_of_graph']:.2f} %)", flush=True)
                else:
                    print(f"images -> ViT -> VisualBERT QA, B={r['B']}: {r['step_ms']:.2f} ms {r['images_per_s']} img/s {r['tflops']:.1f} TFLOP/s"
                          f" (ViT {r['vit_ms']:.2f} ms)", flush=True)
    beside = []
    vb_path = os.path.join(ROOT, "profiles", "visualbert_bench.json")
    if os.path.exists(vb_path):                           # the same encoder fed with region features, as measured by its own tool
        with open(vb_path) as f:
            beside = [r for r in json.load(f)["results"] if r["model"] == "visualbert" and r["B"] == PIPELINE_B]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/vit_bench.py", device="MI355X (gfx950), one GPU", precision="bf16",
                       flop_model="per image layers*(2L(4H^2+2HI)+4L^2H) + 2N(CP^2)H, L=1+N, N=(side/P)^2 (ViT); tools/visualbert_bench.py's (VisualBERT)",
                       visualbert_tflops_b1024=VISUALBERT_TFLOPS_B1024, results=results,
                       visualbert_fed_with_region_features=beside), f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
