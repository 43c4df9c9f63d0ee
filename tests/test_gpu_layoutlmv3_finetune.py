"""-m gpu: EncoderTrainer on LayoutLMv3ForSequenceClassification, on the stored small checkpoint
(tests/golden/layoutlmv3_small.npz: 2 layers, hidden 64, 2 heads of d = 32; its long masked case: 60 text tokens + 5 visual rows).

The yardstick is a float64 restatement with the mode's roundings (mixed_util.Linear16, and the attention pair of
test_gpu_attention_relpos_grad.py with the bias built from the three matrices by indexing, so torch differentiates the fold), torch's
own AdamW and clipping; the rule is the mixed trainer's (tests/test_gpu_mixed_finetune.py): a distance to the pure float64 run of at
most 8 x the yardstick's own, floor 2^-7 of the largest element.  `key.bias` has a zero gradient in exact arithmetic: what is left is
the rounding of dK, at most 8 x 2^-7 sum_m |dK[m, c]|, and AdamW moves it by at most twice the step cap.  The frozen layers' state
of each step is the trainer's own (`_frozen_forward` under its current table): the restatement starts from it."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import EncoderTrainer                                      # noqa: E402
from vltk_amd.layoutlmv3 import LayoutLMv3ForSequenceClassification, relpos_bucket_map      # noqa: E402

import finetune_util as U                                                # noqa: E402
import mixed_util as X                                                   # noqa: E402
from layoutlmv3_util import case_kwargs, golden_state_dict              # noqa: E402
from test_gpu_attention_relpos_grad import RelAttention16, bias_of      # noqa: E402

BF16, FLOOR, LR, MAX_NORM, STEPS = torch.bfloat16, 2.0 ** -7, 1e-3, 0.5, 3
LABELS = np.array([1, 3])


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layoutlmv3_small.npz"))
    cfg, n, sd = golden_state_dict(g, "seq")
    return cfg, n, sd, {k: torch.from_numpy(np.asarray(v)) for k, v in case_kwargs(g, "long", "masked").items()}


def make(**kw):
    cfg, n, sd, _ = fixture()
    model = LayoutLMv3ForSequenceClassification(cfg, n, precision="fp32").load_state_dict(sd)
    kw.setdefault("compute_dtype", BF16)
    return model, EncoderTrainer(model, sd, lr=LR, **kw)


def layer(p, P, x, bias, mask, heads, eps, dtype, taps):
    """One post-LN BERT layer with LayoutLMv3's attention in float64: dtype None is plain, else the mode's roundings."""
    B, Lx, H = x.shape
    lin = (lambda t, k, ry=False, rdx=False: F.linear(t, p[k + ".weight"], p[k + ".bias"])) if dtype is None else \
          (lambda t, k, ry=False, rdx=False: X.Linear16.apply(t, p[k + ".weight"], p[k + ".bias"], dtype, ry, rdx))
    q, k, v = (lin(x, f"{P}.attention.self.{t}", True).view(B, Lx, heads, -1).transpose(1, 2) for t in ("query", "key", "value"))
    k.retain_grad()
    taps.append(k)
    scale = U.launcher_scale(H // heads)
    if dtype is None:
        o = torch.softmax((q @ k.transpose(-1, -2) + bias) * scale + mask[:, None, None, :], -1) @ v
    else:
        o = RelAttention16.apply(q, k, v, bias, mask, scale, dtype, {}, True)
    o = o.transpose(1, 2).reshape(B, Lx, H)
    h1 = F.layer_norm(lin(o, P + ".attention.output.dense", False, True) + x, (H,), p[P + ".attention.output.LayerNorm.weight"],
                      p[P + ".attention.output.LayerNorm.bias"], eps)
    z = F.gelu(lin(h1, P + ".intermediate.dense"))
    return F.layer_norm(lin(z, P + ".output.dense") + h1, (H,), p[P + ".output.LayerNorm.weight"], p[P + ".output.LayerNorm.bias"], eps)


def restated_run(keys, n, boundary, dtype):
    """`STEPS` clipped AdamW steps from the per-step boundary states [(x0, mask, rel)] -> first-step gradients, losses, tensors, and
    per step the column sums of |dK| per trained layer."""
    cfg, _, sd, _ = fixture()
    nl, heads = cfg["num_hidden_layers"], cfg["num_attention_heads"]
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=torch.float64, requires_grad=True) for k in keys}
    bucket = relpos_bucket_map(cfg["rel_pos_bins"], cfg["rel_2d_pos_bins"], cfg["max_rel_pos"], cfg["max_rel_2d_pos"]).long()
    n1, n2 = 2 * cfg["max_rel_pos"] + 1, 2 * cfg["max_rel_2d_pos"] + 1
    opt = torch.optim.AdamW([p[k] for k in keys], lr=LR, weight_decay=0.01)
    out = dict(losses=[], dk=[], first=None)
    for x0, mask, rel in boundary:
        opt.zero_grad()
        e = "layoutlmv3.encoder.rel_pos_"
        lut = torch.cat([p[e + t + "bias.weight"][:, bucket[o:o + m]] for t, o, m in (("", 0, n1), ("x_", n1, n2), ("y_", n1 + n2, n2))], 1)
        bias = bias_of(lut, rel, rel, cfg["max_rel_pos"], cfg["max_rel_2d_pos"])
        x, taps = x0, []
        for i in range(nl - n, nl):
            x = layer(p, f"layoutlmv3.encoder.layer.{i}", x, bias, mask, heads, cfg["layer_norm_eps"], dtype, taps)
        rows = torch.tanh(F.linear(x[:, 0], p["classifier.dense.weight"], p["classifier.dense.bias"]))
        loss = F.cross_entropy(F.linear(rows, p["classifier.out_proj.weight"], p["classifier.out_proj.bias"]), torch.from_numpy(LABELS))
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in keys], MAX_NORM)
        out["dk"].append([t.grad.abs().sum((0, 2)).reshape(-1).numpy() for t in taps])
        if out["first"] is None:
            out["first"] = {k: p[k].grad.numpy().copy() for k in keys}
        opt.step()
        out["losses"].append(float(loss))
    out["tensors"] = {k: p[k].detach().numpy() for k in keys}
    return out


@functools.lru_cache(maxsize=None)
def runs(n):
    """The trainer's STEPS steps and both restatements from its own boundary states, computed once."""
    model, tr = make(train_layers=n, max_grad_norm=MAX_NORM)
    _, _, _, kw = fixture()
    inputs = tr._inputs((), kw)
    boundary, losses, first = [], [], None
    for _ in range(STEPS):
        tr._lut = tr._build_lut()
        x, mask = tr._frozen_forward(inputs)
        B = LABELS.size
        boundary.append((x.double().cpu().reshape(B, -1, tr.H), mask.double().cpu(), tr.enc._rel.long().cpu()))
        losses.append(float(tr.step(labels=LABELS, **kw)))
        first = first or tr.grads()
    yard, run64 = (restated_run(tr.keys, n, boundary, dt) for dt in (BF16, None))
    return tr, losses, first, yard, run64


def key_bias_gamma(keys, key, run64, step):
    return 8 * FLOOR * run64["dk"][step][[k for k in keys if k.endswith("key.bias")].index(key)]


@pytest.mark.parametrize("n", [1, 2])
def test_first_step_gradients(n):
    tr, _, first, yard, run64 = runs(n)
    tables = [k for k in tr.keys if "rel_pos" in k]
    assert len(tables) == 3 and tuple(first) == tr.keys == tuple(tr.state_dict()) and tr.keys[-1] == "classifier.out_proj.bias"
    for k in tr.keys:
        g = first[k].astype(np.float64)
        if k.endswith("key.bias"):
            assert (np.abs(g) <= key_bias_gamma(tr.keys, k, run64, 0)).all(), k
            continue
        d_y, d_gpu = U.maxnorm_rel(yard["first"][k], run64["first"][k]), U.maxnorm_rel(g, run64["first"][k])
        print(f"n={n} grad {k}: d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_y, FLOOR):.3f}")
        assert run64["first"][k].any() and d_gpu <= 8 * max(d_y, FLOOR), k


@pytest.mark.parametrize("n", [1, 2])
def test_clipped_trajectory(n):
    tr, losses, _, yard, run64 = runs(n)
    assert tr.steps == STEPS and tr.grad_norm > MAX_NORM          # the clip acted
    b1, b2 = 0.9, 0.999
    cap = sum(LR * (1 - b1) / (1 - b1 ** t) * np.sqrt(sum((b1 * b1 / b2) ** j for j in range(t))) * np.sqrt((1 - b2 ** t) / (1 - b2))
              for t in range(1, STEPS + 1))
    got = tr.state_dict()
    for name, a, ay, a64 in [(k, got[k], yard["tensors"][k], run64["tensors"][k]) for k in tr.keys] + \
                            [(f"loss[{i}]", losses[i], yard["losses"][i], run64["losses"][i]) for i in range(STEPS)]:
        if name.endswith("key.bias"):
            assert np.abs(a - a64).max() <= 2 * cap + 8 * 2.0 ** -23 * np.abs(a64).max(), name
            continue
        d_y, d_gpu = U.maxnorm_rel(ay, a64), U.maxnorm_rel(a, a64)
        print(f"n={n} {name}: d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_y, FLOOR):.3f}")
        assert d_gpu <= 8 * max(d_y, FLOOR), name


def test_frozen_layers_read_the_trainers_tables(monkeypatch):
    """Step 2's frozen layer runs with the table built from the tensors step 1 left, not with the model's; the model's own table
    is untouched until commit(), after which the model answers as a fresh model loaded from the trainer's tensors."""
    cfg, n, sd, kw = fixture()
    model, tr = make(train_layers=1)
    enc, own, seen = tr.enc, tr.enc._lut.clone(), []
    inner = enc._hidden_after
    monkeypatch.setattr(enc, "_hidden_after", lambda *a: (seen.append(enc._lut.clone()), inner(*a))[1])
    before = model(**kw).clone()
    seen.clear()
    tr.step(labels=LABELS, **kw)
    after_one = tr._build_lut()
    tr.step(labels=LABELS, **kw)
    assert torch.equal(seen[0], own) and torch.equal(seen[1], after_one) and not torch.equal(seen[1], own)
    assert torch.equal(enc._lut, own) and torch.equal(model(**kw), before)
    tr.commit()
    fresh = LayoutLMv3ForSequenceClassification(cfg, n, precision="fp32").load_state_dict({**sd, **tr.state_dict()})
    out = model(**kw)
    assert torch.equal(out, fresh(**kw)) and not torch.equal(out, before) and not torch.equal(enc._lut, own)


@pytest.mark.parametrize("kw,match", [(dict(compute_dtype=None), "torch.bfloat16"), (dict(attention_dropout=0.25), "hidden_dropout"),
                                      (dict(train_embeddings=True, train_layers=2), "train_embeddings=False")], ids=["fp32", "attention dropout", "embeddings"])
def test_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        make(**kw)
