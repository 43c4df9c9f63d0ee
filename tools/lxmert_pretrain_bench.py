#!/usr/bin/env python3
"""What LXMERT's pre-training heads and losses cost on one MI355X, bf16, transformers' default geometry, B = 1024, 20 text tokens,
36 boxes, all in one job:

  encoder            `LxmertEncoder` alone
  heads_and_losses   `LxmertForPreTraining` with every label, logits=True
  loss_only          the same with logits=False, 15 % of the text rows labelled (the reference's `word_mask_rate`)
  cross_entropy      `vk_cross_entropy` alone on 20 480 x 30 522 logits (row stride 30 528), by device events: bytes read / time,
                     beside the card's HBM rate (8.0 TB/s peak, about 6.3 TB/s reached by a plain copy)

usage: python tools/lxmert_pretrain_bench.py [--batch 1024] [--out profiles/lxmert_pretrain_bench.json]

The work runs in one child process under a time limit; a child that fails or runs out of time ends the job.  Call times are a
host clock around a device synchronise, warmed up, over >= 0.5 s of work.
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

TEXT_TOKENS, BOXES, MASK_RATE = 20, 36, 0.15
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3


def child(B):
    import numpy as np
    import torch
    from vltk_amd import _lib as L
    from vltk_amd.layers import stream
    from vltk_amd.lxmert_pretrain import LxmertForPreTraining, lxmert_pretraining_config, make_lxmert_pretraining_state_dict

    sync = torch.cuda.synchronize
    gen = np.random.Generator(np.random.PCG64(0))
    cfg = lxmert_pretraining_config()
    m = LxmertForPreTraining(cfg, precision="bf16").load_state_dict(make_lxmert_pretraining_state_dict(cfg, 1))
    dev = m.lxmert.device
    Lt, V, D = TEXT_TOKENS, BOXES, cfg["visual_feat_dim"]
    ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, Lt))).cuda()
    feats = torch.from_numpy(np.maximum(gen.standard_normal((B, V, D)), 0).astype(np.float32)).cuda().bfloat16()
    pos = torch.from_numpy(gen.uniform(0, 1, (B, V, 4)).astype(np.float32)).cuda().bfloat16()
    labels = np.full(B * Lt, -100)
    picked = gen.choice(B * Lt, int(round(MASK_RATE * B * Lt)), replace=False)
    labels[picked] = gen.integers(0, cfg["vocab_size"], len(picked))
    lab = dict(labels=torch.from_numpy(labels.reshape(B, Lt)), matched_label=torch.from_numpy(gen.integers(0, 2, B)),
               ans=torch.from_numpy(gen.integers(0, cfg["num_qa_labels"], B)),
               obj_labels={"obj": (torch.from_numpy(gen.integers(0, cfg["num_object_labels"], (B, V))), torch.from_numpy(gen.uniform(0, 1, (B, V)).astype(np.float32))),
                           "attr": (torch.from_numpy(gen.integers(0, cfg["num_attr_labels"], (B, V))), torch.from_numpy(gen.uniform(0, 1, (B, V)).astype(np.float32))),
                           "feat": (torch.from_numpy(gen.standard_normal((B, V, D)).astype(np.float32)), torch.from_numpy((gen.uniform(size=(B, V)) < MASK_RATE).astype(np.float32)))})
    # on the device already: the class labels are read back for the host checks, conf and the feature target stay where they are
    lab = {k: (v.cuda() if k != "obj_labels" else {kk: (a.cuda(), b.cuda()) for kk, (a, b) in v.items()}) for k, v in lab.items()}
    out = dict(B=B, text_tokens=Lt, boxes=V, labelled_text_rows=int(len(picked)), text_rows=B * Lt)
    t, n = timed(lambda: m.lxmert(ids, feats, pos), sync)
    out["encoder_ms"], out["calls_timed"] = round(t * 1e3, 3), n
    t, _ = timed(lambda: m(ids, feats, pos, **lab), sync)
    out["heads_and_losses_ms"] = round(t * 1e3, 3)
    full = m(ids, feats, pos, **lab)
    t, _ = timed(lambda: m(ids, feats, pos, **lab, logits=False), sync)
    out["loss_only_ms"] = round(t * 1e3, 3)
    only = m(ids, feats, pos, **lab, logits=False)
    out["loss"] = {k: float(v) for k, v in full.losses.items()}
    out["loss_only_mlm"], out["total"] = float(only.losses["mlm"]), float(full.loss)
    del full, only
    # vk_cross_entropy alone, every row labelled: the logits are read once
    M, C, ld = 20480, cfg["vocab_size"], (cfg["vocab_size"] + 7) // 8 * 8
    x = torch.empty((M, ld), dtype=torch.bfloat16, device=dev).normal_()
    y = torch.from_numpy(gen.integers(0, C, M)).cuda()
    rows = torch.empty((M,), dtype=torch.float32, device=dev)

    def ce():
        L.call("vk_cross_entropy", x.data_ptr(), ld, M, C, y.data_ptr(), -100, rows.data_ptr(), m.lxmert.dt, stream(dev))
    ce()
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ce()
    e1.record()
    sync()
    ms = e0.elapsed_time(e1) / reps
    nbytes = M * C * 2
    out["cross_entropy"] = dict(M=M, C=C, ld=ld, form=("vec", "scalar")[L.load().vk_cross_entropy_form(C, ld, m.lxmert.dt, 1)], ms=round(ms, 4),
                                bytes_read=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3), hbm_peak_tb_per_s=HBM_PEAK_TBS,
                                hbm_copy_tb_per_s=HBM_COPY_TBS, mean_row_loss=float(rows.mean()))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lxmert_pretrain_bench.json"))
    ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.batch)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch)]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    except subprocess.TimeoutExpired as e:
        sys.exit(f"no result within {a.child_timeout:.0f} s; stopping\n{e.stdout or ''}")
    if p.returncode != 0:
        sys.exit(f"exit status {p.returncode}; stopping\n{p.stdout[-4000:]}")
    r = [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")][0]
    ce = r["cross_entropy"]
    print(f"B={r['B']}: encoder {r['encoder_ms']:.2f} ms | + heads and losses (logits=True) {r['heads_and_losses_ms']:.2f} ms | "
          f"loss-only at {r['labelled_text_rows']} of {r['text_rows']} text rows {r['loss_only_ms']:.2f} ms | "
          f"vk_cross_entropy {ce['M']} x {ce['C']} ({ce['form']}) {ce['ms']:.3f} ms = {ce['tb_per_s']:.2f} TB/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/lxmert_pretrain_bench.py", device="MI355X (gfx950), one GPU", precision="bf16",
                       loss_only_not_slower=bool(r["loss_only_ms"] <= r["heads_and_losses_ms"]), result=r), f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
