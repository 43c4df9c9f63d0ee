#!/usr/bin/env python3
"""LayoutLMv3 measured on one MI355X: vk_attention_relpos alone -> profiles/layoutlmv3_bench.json, and the
12-layer model -> profiles/layoutlmv3_model_bench.json.

usage: python tools/layoutlmv3_bench.py [--out PATH]              the attention kernel
       python tools/layoutlmv3_bench.py --model [--out PATH]      the model
       python tools/layoutlmv3_bench.py --grad [--out PATH]       the attention backward -> profiles/layoutlmv3_grad_bench.json

The model section: LayoutLMv3Model in bf16 at transformers' base geometry, 512 text tokens + 197 patch rows (L = 709), B = 8 and 32,
one forward captured into a graph and replayed.  In the same process and the same alternating windows: LayoutLMModel (v1) at 512
tokens and the same B, also replayed.  Per B: ms and pages/s of both, and by device events around those launches alone the
embedding stage (patchify, projection GEMM and vk_layoutlmv3_embed) and one layer's attention, as shares of the replayed forward.

The backward section: vk_attention_relpos_grad beside vk_attention_grad_16 on the same q, k, v, o and dout (the bias-free floor) at
B = 8 and 32, 12 heads, d = 64, bf16, L = 709 and 197, in alternating windows; once with random triples and once document-like
(about 12 tokens a text line share y, x grows along the line: the same-address collisions of the table-gradient histogram show
there).  The new entry is called as the floor is, through `L.call` with a workspace and `dlut` allocated once.  A second child process
times one `EncoderTrainer` step on LayoutLMv3ForSequenceClassification (base geometry, B = 8) at train_layers 1 and 12; a third loads the tools build (make ABLATION=1) with VK_RELPOS_GRAD_HIST=0 and times the same launches
without the histogram, where that library exists.

The kernel section:

One job; the GPU step is a child process under its own time limit.  At B = 32, 12 heads, d = 64, bf16, L = 709 (512 text tokens +
197 patches) and L = 197, alternating in the same windows:
  relpos   vk_attention_relpos at LayoutLMv3's radii 128 / 256 (the bias formed in the kernel from a 5132-byte table a head)
  tiled    vk_attention_tiled on the same q, k, v: the floor, no bias at all
  sdpa     torch's scaled_dot_product_attention given the bias materialised as [B, heads, L, L] in bf16 (already divided by
           sqrt(d)): the vendor yardstick, with the bytes of the bias it reads per call
The relpos output is compared with sdpa's at the timed size.  Times are device events around a window of at least 0.2 s after a
warm-up, the median of three windows; TFLOP/s are algorithmic (4 L L d per head)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, HEADS, D, R1, R2 = 32, 12, 64, 128, 256
LENGTHS = (709, 197)
MODEL_BATCHES = (8, 32)


def step_kernel():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from long_attention_bench import _time_ms
    from vltk_amd import _lib as L
    from vltk_amd.layoutlmv3 import attention_relpos, attention_relpos_form, relpos_triples
    rows, H = [], HEADS * D
    for Lx in LENGTHS:
        gen = np.random.Generator(np.random.PCG64(Lx))
        qkv = torch.from_numpy(gen.standard_normal((B * Lx, 3 * H)).astype(np.float32)).cuda().bfloat16()
        q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
        lut = torch.from_numpy(gen.standard_normal((HEADS, 2 * R1 + 1 + 2 * (2 * R2 + 1))).astype(np.float32)).cuda()
        # text tokens: reading order and boxes over the page; the visual rows restart their positions, as the model's do
        pos = np.concatenate([np.arange(max(Lx - 197, 0)), np.arange(min(Lx, 197))])
        bbox = gen.integers(0, 1001, (B, Lx, 4))
        rel = relpos_triples(torch.from_numpy(np.broadcast_to(pos, (B, Lx)).copy()), torch.from_numpy(bbox)).cuda()
        out_tiled = torch.empty((B * Lx, H), dtype=torch.bfloat16, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def relpos():
            return attention_relpos(q, k, v, rel, rel, lut, R1, R2, HEADS)

        def tiled():
            L.call("vk_attention_tiled", q.data_ptr(), 3 * H, k.data_ptr(), 3 * H, v.data_ptr(), 3 * H, None, out_tiled.data_ptr(), H, B, HEADS,
                   Lx, Lx, D, L.VK_BF16, stream)
        dl = rel.long()[:, None, :, :] - rel.long()[:, :, None, :]
        n1, n2 = 2 * R1 + 1, 2 * R2 + 1
        bias = (lut[:, dl[..., 0].clamp(-R1, R1) + R1] + (lut[:, dl[..., 1].clamp(-R2, R2) + R2 + n1] +
                                                          lut[:, dl[..., 2].clamp(-R2, R2) + R2 + n1 + n2])).transpose(0, 1)
        bias16 = (bias / D ** 0.5).bfloat16().contiguous()
        del bias, dl
        qh, kh, vh = (t.reshape(B, Lx, HEADS, D).transpose(1, 2) for t in (q, k, v))

        def sdpa():
            return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias16)
        got = relpos().float().reshape(B, Lx, HEADS, D).transpose(1, 2)
        want = sdpa().float()
        diff = float((got - want).abs().max() / want.abs().max())
        t_rel, t_tiled, t_sdpa = _time_ms([relpos, tiled, sdpa])
        flops = 4.0 * Lx * Lx * D * B * HEADS
        rows.append(dict(L=Lx, form=attention_relpos_form(Lx, Lx, D, torch.bfloat16, 3 * H, 3 * H, 3 * H), relpos_ms=t_rel, tiled_ms=t_tiled,
                         sdpa_ms=t_sdpa, relpos_tflops=flops / t_rel / 1e9, tiled_tflops=flops / t_tiled / 1e9, sdpa_tflops=flops / t_sdpa / 1e9,
                         relpos_over_tiled=t_rel / t_tiled, sdpa_over_relpos=t_sdpa / t_rel, sdpa_bias_bytes=bias16.numel() * 2,
                         relpos_table_bytes=lut.numel() * 4, max_rel_diff_vs_sdpa=diff))
        del bias16
    return rows


GRAD_BATCHES = (8, 32)


def step_grad():
    import numpy as np
    import torch
    from long_attention_bench import _time_ms
    from vltk_amd import _lib as L
    from vltk_amd.layoutlmv3 import attention_relpos, attention_relpos_grad
    rows, H = [], HEADS * D
    stream = torch.cuda.current_stream().cuda_stream
    for Bg in GRAD_BATCHES:
        for Lx in LENGTHS:
            gen = np.random.Generator(np.random.PCG64([Bg, Lx]))
            qkv = torch.from_numpy(gen.standard_normal((Bg * Lx, 3 * H)).astype(np.float32)).cuda().bfloat16()
            q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
            dout = torch.from_numpy(gen.standard_normal((Bg * Lx, H)).astype(np.float32)).cuda().bfloat16()
            lut = torch.from_numpy(gen.standard_normal((HEADS, 2 * R1 + 1 + 2 * (2 * R2 + 1))).astype(np.float32)).cuda()
            pos = np.broadcast_to(np.concatenate([np.arange(max(Lx - 197, 0)), np.arange(min(Lx, 197))]), (Bg, Lx))
            tok = np.arange(Lx)
            doc = np.stack([pos, np.broadcast_to(40 + 75 * (tok % 12), (Bg, Lx)), np.broadcast_to(30 + 16 * (tok // 12), (Bg, Lx))], -1)
            rand = np.stack([pos, gen.integers(0, 1001, (Bg, Lx)), gen.integers(0, 1001, (Bg, Lx))], -1)
            rel = {n: torch.from_numpy(t.astype(np.int32)).cuda().contiguous() for n, t in (("random", rand), ("document", doc))}
            o = {n: attention_relpos(q, k, v, r, r, lut, R1, R2, HEADS) for n, r in rel.items()}
            dqkv = torch.empty((Bg * Lx, 3 * H), dtype=torch.float32, device="cuda")
            outs = tuple(dqkv[:, i * H:(i + 1) * H] for i in range(3))
            need = L.load().vk_attention_grad_16_workspace_bytes(Bg, HEADS, Lx)
            ws = torch.empty((need // 4,), dtype=torch.float32, device="cuda")

            def floor():
                L.call("vk_attention_grad_16", q.data_ptr(), 3 * H, k.data_ptr(), 3 * H, v.data_ptr(), 3 * H, None, o["random"].data_ptr(), H,
                       dout.data_ptr(), H, outs[0].data_ptr(), 3 * H, outs[1].data_ptr(), 3 * H, outs[2].data_ptr(), 3 * H, Bg, HEADS, Lx, Lx, D,
                       L.VK_BF16, ws.data_ptr(), need, stream)

            need_g = L.load().vk_attention_relpos_grad_workspace_bytes(Bg, HEADS, Lx, R1, R2)
            ws_g = torch.empty((need_g // 8,), dtype=torch.int64, device="cuda")
            dlut = torch.empty_like(lut)
            check = attention_relpos_grad(q, k, v, o["random"], dout, rel["random"], rel["random"], lut, R1, R2, HEADS)[3]

            def grad(name):          # the entry itself with a workspace and dlut allocated once, as the floor is timed
                r = rel[name].data_ptr()
                return lambda: L.call("vk_attention_relpos_grad", q.data_ptr(), 3 * H, k.data_ptr(), 3 * H, v.data_ptr(), 3 * H, None, r, r,
                                      lut.data_ptr(), R1, R2, o[name].data_ptr(), H, dout.data_ptr(), H, outs[0].data_ptr(), 3 * H,
                                      outs[1].data_ptr(), 3 * H, outs[2].data_ptr(), 3 * H, dlut.data_ptr(), Bg, HEADS, Lx, Lx, D, L.VK_BF16,
                                      ws_g.data_ptr(), need_g, stream)
            grad("random")()
            torch.cuda.synchronize()
            assert torch.equal(dlut, check), "the raw call and the wrapper disagree"
            t_rand, t_doc, t_floor = _time_ms([grad("random"), grad("document"), floor])
            rows.append(dict(B=Bg, L=Lx, histogram=os.environ.get("VK_RELPOS_GRAD_HIST") != "0", relpos_grad_random_ms=t_rand,
                             relpos_grad_document_ms=t_doc, grad16_ms=t_floor, random_over_floor=t_rand / t_floor,
                             document_over_floor=t_doc / t_floor))
    return rows


def step_train():
    """One EncoderTrainer step on LayoutLMv3ForSequenceClassification at the base geometry (512 text tokens + 197 patch rows, B = 8,
    bf16 model, compute_dtype bf16) with the last 1 and all 12 layers trained; a step ends with a device synchronisation."""
    import numpy as np
    import torch
    from long_attention_bench import _time_ms
    from vltk_amd import EncoderTrainer
    from vltk_amd import layoutlmv3 as V3
    gen = np.random.Generator(np.random.PCG64(0))
    cfg = V3.layoutlmv3_config(max_position_embeddings=514)
    sd = V3.make_layoutlmv3_head_state_dict(cfg, "seq", 16, 1)
    model = V3.LayoutLMv3ForSequenceClassification(cfg, 16, precision="bf16").load_state_dict(sd)
    Bm, Lt = 8, 512
    ids = torch.from_numpy(gen.integers(2, cfg["vocab_size"], (Bm, Lt)))
    xs, ys = np.sort(gen.integers(0, 1001, (Bm, Lt, 2)), -1), np.sort(gen.integers(0, 1001, (Bm, Lt, 2)), -1)
    bbox = torch.from_numpy(np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1))
    pix = torch.from_numpy(gen.standard_normal((Bm, 3, 224, 224)).astype(np.float32))
    labels = gen.integers(0, 16, Bm)
    rows = []
    for n in (1, 12):
        tr = EncoderTrainer(model, sd, train_layers=n, compute_dtype=torch.bfloat16, max_grad_norm=1.0)
        (t,) = _time_ms([lambda: tr.step(ids, bbox, None, None, pix, labels=labels)])
        rows.append(dict(B=Bm, L=Lt + 197, train_layers=n, step_ms=t, pages_per_s=Bm / t * 1e3))
        del tr
    return rows


def step_model():
    import numpy as np
    import torch
    from long_attention_bench import _time_ms
    from vltk_amd import layoutlm as V1
    from vltk_amd import layoutlmv3 as V3
    gen = np.random.Generator(np.random.PCG64(0))
    cfg3, cfg1 = V3.layoutlmv3_config(max_position_embeddings=514), V1.layoutlm_config()
    m3 = V3.LayoutLMv3Model(cfg3, precision="bf16").load_state_dict(V3.make_layoutlmv3_state_dict(cfg3, 1))
    m1 = V1.LayoutLMModel(cfg1, precision="bf16").load_state_dict(V1.make_layoutlm_state_dict(cfg1, 1))
    H, Lt = cfg3["hidden_size"], 512
    rows = []
    for Bm in MODEL_BATCHES:
        ids = torch.from_numpy(gen.integers(2, cfg1["vocab_size"], (Bm, Lt))).cuda()
        xs, ys = np.sort(gen.integers(0, 1001, (Bm, Lt, 2)), -1), np.sort(gen.integers(0, 1001, (Bm, Lt, 2)), -1)
        bbox = torch.from_numpy(np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)).cuda()
        mask = torch.ones((Bm, Lt), device="cuda")
        pix = torch.from_numpy(gen.standard_normal((Bm, 3, 224, 224)).astype(np.float32)).cuda()
        in3, in1 = (ids, bbox, mask, None, pix), (ids, bbox, mask, None)
        m3._check(*in3), m1._check(*in1)
        g3, out3 = m3._capture(m3._forward, list(in3))
        g1, _ = m1._capture(m1._forward, list(in1))
        eager = m3(*in3).clone()
        g3.replay()
        torch.cuda.synchronize()
        assert torch.equal(out3, eager), "the replayed graph differs from the eager forward"
        x, amask = m3._embed(*in3)
        Lx = x.shape[0] // Bm
        qkv = m3._linear(x, "encoder.layer.0.attention.self.qkv")
        t3, t1, t_emb, t_att = _time_ms([g3.replay, g1.replay, lambda: m3._embed(*in3),
                                         lambda: m3._self_attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], amask, Bm, Lx)])
        rows.append(dict(B=Bm, L=Lx, text_tokens=Lt, patch_rows=Lx - Lt, embed_form=m3.embed_form(), relpos_form=m3.relpos_form(Lx),
                         v3_graph_ms=t3, v3_pages_per_s=Bm / t3 * 1e3, v1_graph_ms=t1, v1_pages_per_s=Bm / t1 * 1e3, v3_over_v1=t3 / t1,
                         embed_stage_ms=t_emb, embed_stage_share=t_emb / t3, attention_ms_per_layer=t_att,
                         attention_share=t_att * cfg3["num_hidden_layers"] / t3))
    return rows


def main_grad(out):
    """The shipped library, then the tools build without the histogram where it exists: one child process each, one at a time."""
    result = {"geometry": dict(heads=HEADS, d=D, r1=R1, r2=R2, dtype="bf16", batches=GRAD_BATCHES, lengths=LENGTHS), "steps": {}}
    legs = [("grad", "grad", {}), ("train_step", "train", {})]
    if os.path.exists(os.path.join(ROOT, "vltk_amd", "libvltk_hip_ablation.so")):
        legs.append(("grad_no_histogram", "grad", {"VLTK_AMD_ABLATION_LIB": "1", "VK_RELPOS_GRAD_HIST": "0"}))
    status = 0
    for name, step, env in legs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=300, capture_output=True, text=True,
                               env=dict(os.environ, **env))
        except subprocess.TimeoutExpired:
            result["steps"][name] = {"error": "no result within 300 s"}
            status = 1
            break                                   # nothing more on the GPU after a step that did not end
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result["steps"][name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            status = 1
            break
        result["steps"][name] = json.loads(lines[-1][len("RESULT "):])
    print(json.dumps(result["steps"]), flush=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true", help="measure the 12-layer model instead of the attention kernel")
    ap.add_argument("--grad", action="store_true", help="measure the attention backward beside vk_attention_grad_16")
    ap.add_argument("--out")
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "layoutlmv3_bench needs a GPU"
        print("RESULT " + json.dumps({"model": step_model, "kernel": step_kernel, "grad": step_grad, "train": step_train}[a.step]()), flush=True)
        return 0
    if a.grad:
        return main_grad(a.out or os.path.join(ROOT, "profiles", "layoutlmv3_grad_bench.json"))
    step = "model" if a.model else "kernel"
    a.out = a.out or os.path.join(ROOT, "profiles", "layoutlmv3_model_bench.json" if a.model else "layoutlmv3_bench.json")
    geometry = dict(model="LayoutLMv3 base: 12 layers, hidden 768, 12 heads", text_tokens=512, patch_rows=197, dtype="bf16",
                    beside="LayoutLM (v1) base at 512 tokens") if a.model else dict(B=B, heads=HEADS, d=D, r1=R1, r2=R2, dtype="bf16")
    result = {"geometry": geometry, "steps": {}}
    status = 0
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=420, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result["steps"][step] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            status = 1
        else:
            result["steps"][step] = json.loads(lines[-1][len("RESULT "):])
    except subprocess.TimeoutExpired:
        result["steps"][step] = {"error": "no result within 420 s"}
        status = 1
    print(json.dumps(result["steps"][step]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
