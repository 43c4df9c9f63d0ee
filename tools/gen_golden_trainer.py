#!/usr/bin/env python3
"""tests/golden/trainer_steps.json: what `EncoderTrainer` and `HeadTrainer` ask of the library in a step, and the bits they leave.

Six scenarios on the suite's own fixtures (tests/finetune_util.py, tests/train_util.py, the small golden configs), two steps each:

  encoder_fp32     VisualBERT-QA at hidden 32, 16 sequences of 16 rows, train_layers=2, max_grad_norm=1.0, fp32
  encoder_mixed    the wide fixture (hidden 128, d = 32), train_layers=2, max_grad_norm=1.0, compute_dtype=torch.bfloat16
  layoutlm_fp32    LayoutLM's small golden config, train_layers=1: the pooled path
  layoutlm_mixed   the same with compute_dtype=torch.bfloat16
  head_lxmert      `HeadTrainer.step_features` on LXMERT's answer head (hidden 32, batch 64)
  head_linear      `HeadTrainer.step_features` on VisualBERT's single-Linear `cls`

Per scenario `record()` keeps
  trace    the second step's calls through `_lib.call` in order: [name, arguments], a pointer argument (by `_lib.SIGNATURES`)
           reduced to whether it is non-null, every integer and float kept as passed.  The same on every device.
  sha256   over the two losses' bytes, then `grads()` and `state_dict()` in key order after the second step.  The file keeps it
           under the device's name (`torch.cuda.get_device_name(0)`): another device may round in another order.

The file is a record of the trainers as they were BEFORE the layer walk, the Linear backward and the trainer base were folded
into one (its "recorded_at" names that commit): tests/test_gpu_trainer_trace.py holds every later version to it.  It is written
once and not regenerated from a later trainer; `--out` elsewhere and `cmp` show whether a run reproduces it.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_trainer.py --recorded-at <commit> [--out tests/golden/trainer_steps.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
sys.dont_write_bytecode = True

from vltk_amd import EncoderTrainer, HeadTrainer, step_lr                                # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENARIOS = ("encoder_fp32", "encoder_mixed", "layoutlm_fp32", "layoutlm_mixed", "head_lxmert", "head_linear")
STEPS = 2


def _is_pointer(ctype):
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer)


def reduce_call(name, args):
    """[name, arguments] as the file keeps it: pointers to non-null / null, numbers as passed."""
    types = L.SIGNATURES[name][1]
    assert len(types) == len(args), (name, len(types), len(args))
    kept = []
    for t, a in zip(types, args):
        if _is_pointer(t):
            kept.append(bool(a))
        elif isinstance(a, (bool, int, np.integer)):
            kept.append(int(a))
        else:
            kept.append(float(a))
    return [name, kept]


class Recorder:
    """`with Recorder() as calls:` every call through `_lib.call` as (name, arguments), the real call made."""

    def __enter__(self):
        self.calls, self.real = [], L.call
        L.call = lambda name, *a: (self.calls.append((name, a)), self.real(name, *a))[1]
        return self.calls

    def __exit__(self, *exc):
        L.call = self.real


def _encoder(wide, mixed):
    import finetune_util as U
    from vltk_amd.visualbert import VisualBertForQuestionAnswering
    cfg, sd, inputs, labels = U.trajectory_fixture(wide=wide)
    model = VisualBertForQuestionAnswering(cfg, U.FIXTURE_LABELS, precision="fp32").load_state_dict(sd)
    tr = EncoderTrainer(model, sd, train_layers=2, lr=U.FIXTURE_LR, schedule=step_lr(*U.FIXTURE_STEP_LR), max_grad_norm=1.0,
                        compute_dtype=torch.bfloat16 if mixed else None)
    t = {k: torch.from_numpy(v) for k, v in inputs.items()}
    return tr, lambda: tr.step(t["input_ids"], t["visual_embeds"], labels=labels, attention_mask=t["attention_mask"],
                               visual_attention_mask=t["visual_attention_mask"])


def _layoutlm(mixed):
    from layoutlm_util import case_kwargs, golden_head
    from finetune_util import IGNORE_INDEX
    from vltk_amd.layoutlm import LayoutLMForSequenceClassification
    g = np.load(os.path.join(GOLDEN, "layoutlm_small.npz"))
    cfg, nlab, sd = golden_head(g, "seq")
    kw = {k: torch.from_numpy(v) for k, v in case_kwargs(g, "short", "masked").items()}
    ids = torch.from_numpy(g["short/input_ids"])
    labels = np.array([1, IGNORE_INDEX, nlab - 1], np.int64)
    model = LayoutLMForSequenceClassification(cfg, nlab, precision="fp32").load_state_dict(sd)
    tr = EncoderTrainer(model, sd, train_layers=1, lr=1e-3, schedule=step_lr(20, 0.9), compute_dtype=torch.bfloat16 if mixed else None)
    return tr, lambda: tr.step(ids, labels=labels, **kw)


def _head_lxmert():
    import train_util as T
    from vltk_amd.lxmert import LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict
    cfg = lxmert_config(vocab_size=64, hidden_size=32, num_attention_heads=4, intermediate_size=64, l_layers=1, x_layers=1, r_layers=1,
                        max_position_embeddings=16, visual_feat_dim=64)
    _, head, feats, labels = T.head_fixture()
    sd = make_lxmert_qa_state_dict(cfg, 16, seed=1)
    sd.update(head)
    tr = HeadTrainer(LxmertForQuestionAnswering(cfg, 16, precision="fp32").load_state_dict(sd), lr=1e-3, schedule=step_lr(20, 0.9))
    x = torch.from_numpy(feats).cuda()
    return tr, lambda: tr.step_features(x, labels)


def _head_linear():
    import train_util as T
    from visualbert_util import golden_inputs, golden_qa_state_dict
    from vltk_amd.visualbert import VisualBertForQuestionAnswering
    g = np.load(os.path.join(GOLDEN, "visualbert_small.npz"))
    cfg, _, _ = golden_inputs(g, "short")
    answers = int(g["qa/num_labels"])
    _, head, feats, labels = T.head_fixture(cfg["hidden_size"], answers, kind="linear", prefix="cls")
    sd = dict(golden_qa_state_dict(g))
    sd.update(head)
    tr = HeadTrainer(VisualBertForQuestionAnswering(cfg, answers, precision="fp32").load_state_dict(sd), lr=1e-3, schedule=step_lr(20, 0.9))
    x = torch.from_numpy(feats).cuda()
    return tr, lambda: tr.step_features(x, labels)


_BUILD = {"encoder_fp32": lambda: _encoder(False, False), "encoder_mixed": lambda: _encoder(True, True),
          "layoutlm_fp32": lambda: _layoutlm(False), "layoutlm_mixed": lambda: _layoutlm(True),
          "head_lxmert": _head_lxmert, "head_linear": _head_linear}


def record(scenario):
    """A fresh trainer of the scenario, two steps -> dict(trace=[[name, arguments]] of the second step, sha256=hex digest)."""
    tr, step = _BUILD[scenario]()
    digest = hashlib.sha256()
    for i in range(STEPS):
        with Recorder() as calls:
            loss = step()
        digest.update(loss.cpu().numpy().tobytes())
    assert tr.steps == STEPS
    for held in (tr.grads(), tr.state_dict()):
        for k, v in held.items():
            digest.update(k.encode())
            digest.update(np.ascontiguousarray(v).tobytes())
    return dict(trace=[reduce_call(name, a) for name, a in calls], sha256=digest.hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorded-at", required=True, help="the commit whose trainers are recorded")
    ap.add_argument("--out", default=os.path.join(GOLDEN, "trainer_steps.json"))
    a = ap.parse_args()
    device = torch.cuda.get_device_name(0)
    lines = []
    for name in SCENARIOS:
        r = record(name)
        print(f"{name}: {len(r['trace'])} calls, sha256 {r['sha256'][:16]}")
        calls = ",\n".join("    " + json.dumps(c) for c in r["trace"])
        lines.append(f'  {json.dumps(name)}: {{"sha256": {json.dumps({device: r["sha256"]})}, "trace": [\n{calls}\n  ]}}')
    with open(a.out, "w") as f:
        f.write('{"recorded_at": %s, "scenarios": {\n%s\n}}\n' % (json.dumps(a.recorded_at), ",\n".join(lines)))
    json.load(open(a.out))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
