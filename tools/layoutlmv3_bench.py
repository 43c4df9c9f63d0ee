#!/usr/bin/env python3
"""vk_attention_relpos measured on one MI355X: writes profiles/layoutlmv3_bench.json.

usage: python tools/layoutlmv3_bench.py [--out PATH]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layoutlmv3_bench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "layoutlmv3_bench needs a GPU"
        print("RESULT " + json.dumps(step_kernel()), flush=True)
        return 0
    result = {"geometry": dict(B=B, heads=HEADS, d=D, r1=R1, r2=R2, dtype="bf16"), "steps": {}}
    status = 0
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "kernel"], timeout=420, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result["steps"]["kernel"] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            status = 1
        else:
            result["steps"]["kernel"] = json.loads(lines[-1][len("RESULT "):])
    except subprocess.TimeoutExpired:
        result["steps"]["kernel"] = {"error": "no result within 420 s"}
        status = 1
    print(json.dumps(result["steps"]["kernel"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
