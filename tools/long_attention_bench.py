#!/usr/bin/env python3
"""Attention past the small kernels, measured on one MI355X: writes profiles/long_attention_bench.json.

usage: python tools/long_attention_bench.py [--out PATH]

One job; every GPU step is a child process of its own under its own time limit, and the first step that fails ends the job
(the steps already done are still written).  Steps:
  shared   vk_attention (the parent's kernel at these shapes: the scalar LDS kernel) and vk_attention_tiled, alternating, at
           B = 256, 12 heads, d = 64, bf16, (Lq, Lk) = (49, 49), (100, 100), (20, 100), (100, 20); outputs compared
  large    the tiled kernel at (196, 196), (576, 576), (1024, 1024), algorithmic TFLOP/s (4 Lq Lk d per head)
  stream   the streaming kernel in fp32 at (196, 196)
  encoder_tiled / encoder_old   the default geometry, bf16, 20 text tokens, V = 36, 100, 196 at B = 1024, eager and HIP-graph
           replay, with VK_ATTENTION_TILED unset / = 0
Times are device events around a window of at least 0.2 s after a warm-up, the median of three windows."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

B, HEADS, D = 256, 12, 64
SHARED = [(49, 49), (100, 100), (20, 100), (100, 20)]
LARGE = [(196, 196), (576, 576), (1024, 1024)]
STEPS = [("shared", {}, 240), ("large", {}, 240), ("stream", {}, 240), ("encoder_tiled", {}, 420),
         ("encoder_old", {"VK_ATTENTION_TILED": "0"}, 420)]


def _setup(dt_name, Lq, Lk):
    import numpy as np
    import torch
    from vltk_amd import _lib as L
    dt, td = {"bf16": (L.VK_BF16, torch.bfloat16), "fp32": (L.VK_F32, torch.float32)}[dt_name]
    H = HEADS * D
    gen = np.random.Generator(np.random.PCG64(Lq * Lk))
    q = torch.from_numpy(gen.standard_normal((B * Lq, H)).astype(np.float32)).cuda().to(td)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H)).astype(np.float32)).cuda().to(td)
    out = torch.empty((B * Lq, H), dtype=td, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch(entry):
        L.call(entry, q.data_ptr(), H, kv.data_ptr(), 2 * H, kv.data_ptr() + H * kv.element_size(), 2 * H, None, out.data_ptr(), H,
               B, HEADS, Lq, Lk, D, dt, stream)

    def route(entry):
        return ("mfma", "lds", "tiled", "stream")[L.load().vk_attention_route(Lq, Lk, D, dt, H, 2 * H, 2 * H, 1,
                                                                                int(entry == "vk_attention_tiled"))]
    return launch, route, out


def _window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _time_ms(fns):
    """Median of three alternating windows per function, each at least 0.2 s long."""
    import statistics
    iters = []
    for fn in fns:
        for _ in range(3):
            fn()
        t = _window(fn, 10)
        iters.append(max(10, int(200.0 / max(t, 1e-3)) + 1))
    got = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            got[i].append(_window(fn, iters[i]))
    return [statistics.median(g) for g in got]


def _tflops(Lq, Lk, ms):
    return 4.0 * Lq * Lk * D * B * HEADS / (ms * 1e-3) / 1e12


def step_shared():
    import torch
    rows = []
    for Lq, Lk in SHARED:
        launch, route, out = _setup("bf16", Lq, Lk)
        launch("vk_attention")
        torch.cuda.synchronize()
        old = out.float().clone()
        launch("vk_attention_tiled")
        torch.cuda.synchronize()
        diff = float((out.float() - old).abs().max() / old.abs().max())
        t_old, t_new = _time_ms([lambda: launch("vk_attention"), lambda: launch("vk_attention_tiled")])
        rows.append(dict(Lq=Lq, Lk=Lk, old_kernel=route("vk_attention"), new_kernel=route("vk_attention_tiled"), old_ms=t_old, new_ms=t_new,
                         speedup=t_old / t_new, new_tflops=_tflops(Lq, Lk, t_new), max_rel_diff=diff))
    return rows


def step_large():
    rows = []
    for Lq, Lk in LARGE:
        launch, route, _ = _setup("bf16", Lq, Lk)
        (t,) = _time_ms([lambda: launch("vk_attention_tiled")])
        rows.append(dict(Lq=Lq, Lk=Lk, kernel=route("vk_attention_tiled"), ms=t, tflops=_tflops(Lq, Lk, t)))
    return rows


def step_stream():
    launch, route, _ = _setup("fp32", 196, 196)
    (t,) = _time_ms([lambda: launch("vk_attention")])
    return [dict(Lq=196, Lk=196, dtype="fp32", kernel=route("vk_attention"), ms=t, tflops=_tflops(196, 196, t))]


def step_encoder():
    import numpy as np
    import torch
    from vltk_amd.lxmert import LxmertEncoder, lxmert_config, make_lxmert_state_dict
    cfg = lxmert_config()
    m = LxmertEncoder(cfg, precision="bf16").load_state_dict(make_lxmert_state_dict(cfg, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    rows, EB = [], 1024
    for V in (36, 100, 196):
        ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (EB, 20))).cuda()
        feats = torch.from_numpy(np.maximum(gen.standard_normal((EB, V, 2048)), 0).astype(np.float32)).cuda().bfloat16()
        pos = torch.from_numpy(gen.uniform(0, 1, (EB, V, 4)).astype(np.float32)).cuda().bfloat16()
        replay = m.capture(ids, feats, pos)
        t_eager, t_graph = _time_ms([lambda: m(ids, feats, pos), lambda: replay(ids, feats, pos)])
        rows.append(dict(V=V, B=EB, tiled_switch=os.environ.get("VK_ATTENTION_TILED", "unset"), eager_ms=t_eager,
                         eager_examples_per_s=EB / t_eager * 1e3, graph_ms=t_graph, graph_examples_per_s=EB / t_graph * 1e3))
        del replay
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_attention_bench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "long_attention_bench needs a GPU"
        fn = {"shared": step_shared, "large": step_large, "stream": step_stream, "encoder_tiled": step_encoder,
              "encoder_old": step_encoder}[a.step]
        print("RESULT " + json.dumps(fn()), flush=True)
        return 0
    result = {"geometry": dict(B=B, heads=HEADS, d=D), "steps": {}}
    status = 0
    for name, env, limit in STEPS:
        e = dict(os.environ)
        e.pop("VK_ATTENTION_TILED", None)
        e.update(env)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], env=e, timeout=limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            result["steps"][name] = {"error": f"no result within {limit} s"}
            status = 1
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result["steps"][name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            status = 1
            break                                   # nothing more is started on the GPU after a failed step
        result["steps"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, json.dumps(result["steps"][name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
