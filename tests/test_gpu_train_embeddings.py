"""GPU (-m gpu): `EncoderTrainer(train_embeddings=True)` end to end.  The yardstick is torch on the CPU: the embedding stage restated
(`F.embedding` with `padding_idx`, the sum in transformers' order, `F.layer_norm`) in front of finetune_util's layers and head, with
autograd, `clip_grad_norm_` and `torch.optim.AdamW`, in fp64 and in fp32.  The rule is test_gpu_finetune.py's:
the GPU may be at most 8 x as far from the fp64 run as torch's fp32 run is (`maxnorm_rel`, floor 2^-23); the mixed mode is held to
the rounding restatement (mixed_util, `visual_projection` a `Linear16`) with floor 2^-7 (section 28).  `key.bias` keeps its rule."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import EncoderTrainer                                                      # noqa: E402
from vltk_amd.layoutlm import LayoutLMForSequenceClassification                          # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering                           # noqa: E402

import finetune_util as U                                                                # noqa: E402
import mixed_util as X                                                                   # noqa: E402
from layoutlm_util import case_kwargs as llm_kwargs, golden_head                         # noqa: E402
from test_gpu_finetune import hold                                                       # noqa: E402
from test_gpu_mixed_finetune import hold_trajectory                                      # noqa: E402

BF16, LR, MAX_NORM = torch.bfloat16, 1e-3, 1.0
FLOORS = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -7}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layoutlm_small.npz")


@functools.lru_cache(maxsize=None)
def fixture(which):
    # pad ids (VisualBertConfig: 1, LayoutLMConfig: 0) and a repeated id; left == right in every third box: one x row twice per token
    if which == "llm":
        g = np.load(GOLDEN)
        cfg, nlab, sd = golden_head(g, "seq")
        inp = dict(input_ids=g["short/input_ids"].copy(), **{k: v.copy() for k, v in llm_kwargs(g, "short", "masked").items()})
        inp["input_ids"][:, -2:] = 0
        inp["bbox"][:, ::3, 2] = inp["bbox"][:, ::3, 0]
        return dict(cfg=cfg, sd=sd, labels=np.array([1, U.IGNORE_INDEX, nlab - 1], np.int64), inp=inp, kind="classifier", prefix="layoutlm.",
                    pad=cfg.get("pad_token_id", 0), nlab=nlab, rows=None, mask01=inp["attention_mask"])
    cfg, sd, inp, labels = U.trajectory_fixture(wide=which == "wide")
    inp["input_ids"][:, 2], inp["input_ids"][::2, 3], inp["input_ids"][:, 4] = 1, 1, 7
    return dict(cfg=cfg, sd=sd, labels=labels, inp=inp, kind="cls", prefix="visual_bert.", pad=1, nlab=U.FIXTURE_LABELS,
                rows=inp["attention_mask"].sum(1) - 2, mask01=np.concatenate((inp["attention_mask"], inp["visual_attention_mask"]), 1))


def model_of(fx, precision="fp32"):
    cls = LayoutLMForSequenceClassification if fx["kind"] == "classifier" else VisualBertForQuestionAnswering
    return cls(fx["cfg"], fx["nlab"], precision=precision).load_state_dict(fx["sd"])


def trainer(fx, model=None, **kw):
    kw.setdefault("train_layers", fx["cfg"]["num_hidden_layers"])
    kw.setdefault("train_embeddings", True)
    return EncoderTrainer(model or model_of(fx), fx["sd"], lr=LR, **kw)


def step(tr, fx):
    return float(tr.step(**{k: torch.from_numpy(v) for k, v in fx["inp"].items()}, labels=fx["labels"]))


def embedded(p, E, fx, dt16):
    inp, H = fx["inp"], fx["cfg"]["hidden_size"]
    ids = inp["input_ids"]
    B, Lt = ids.shape
    tt, pos = inp.get("token_type_ids", np.zeros_like(ids)), np.tile(np.arange(Lt), (B, 1))

    def emb(t, i, **kw):
        return F.embedding(torch.as_tensor(np.asarray(i, np.int64)), p[f"{E}{t}_embeddings.weight"], **kw)
    if fx["kind"] == "classifier":
        b = inp["bbox"]
        s = (emb("word", ids, padding_idx=fx["pad"]) + emb("position", pos) + emb("x_position", b[..., 0]) + emb("y_position", b[..., 1])
             + emb("x_position", b[..., 2]) + emb("y_position", b[..., 3]) + emb("h_position", b[..., 3] - b[..., 1])
             + emb("w_position", b[..., 2] - b[..., 0]) + emb("token_type", tt))
    else:
        w, bias = p[E + "visual_projection.weight"], p[E + "visual_projection.bias"]
        v = torch.as_tensor(inp["visual_embeds"]).to(w.dtype)
        ve = X.Linear16.apply(v, w, bias, dt16, False, False) if dt16 else F.linear(v, w, bias)
        zero = np.zeros(v.shape[:2])
        s = torch.cat((emb("word", ids, padding_idx=fx["pad"]) + emb("token_type", tt) + emb("position", pos),
                       ve + emb("visual_position", zero) + emb("visual_token_type", zero + 1)), 1)
    return F.layer_norm(s, (H,), p[E + "LayerNorm.weight"], p[E + "LayerNorm.bias"], fx["cfg"]["layer_norm_eps"])


@functools.lru_cache(maxsize=None)
def yardstick(which, mode, steps=3):
    """-> finetune_util.torch_finetune_run's dict.  mode "fp32" / "fp64": torch in that dtype; "bf16": fp64 with the mode's roundings."""
    fx = fixture(which)
    cfg, P = fx["cfg"], fx["prefix"]
    keys = tuple(k for k in fx["sd"] if k.startswith(P + "embeddings.")) + U.trained_keys(P, range(cfg["num_hidden_layers"]), fx["kind"])
    dt, dt16 = (torch.float32 if mode == "fp32" else torch.float64), (BF16 if mode == "bf16" else None)
    p = {k: torch.tensor(np.asarray(fx["sd"][k]), dtype=dt, requires_grad=True) for k in keys}
    layers = [f"{P}encoder.layer.{i}" for i in range(cfg["num_hidden_layers"])]
    mask, y = U.additive(fx["mask01"], dt), torch.tensor(fx["labels"])
    rows = None if fx["rows"] is None else torch.as_tensor(fx["rows"])
    opt = torch.optim.AdamW([p[k] for k in keys], lr=LR)
    out = dict(losses=[], dk=[], keybias=[], first=None)
    for _ in range(steps):
        opt.zero_grad()
        taps, x = [], embedded(p, P + "embeddings.", fx, dt16)
        tail = (cfg["num_attention_heads"], cfg["layer_norm_eps"], fx["kind"], rows, P)
        logits = X.tail_logits_16(p, x, mask, layers, *tail, dt16, taps) if dt16 else U.tail_logits(p, x, mask, layers, *tail, taps)
        loss = F.cross_entropy(logits, y, ignore_index=U.IGNORE_INDEX)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in keys], MAX_NORM)
        out["dk"].append([t.grad.detach().double().abs().sum((0, 1)).numpy() for t in taps])
        out["keybias"].append({k: p[k].grad.detach().double().numpy().copy() for k in keys if k.endswith("key.bias")})
        out["first"] = out["first"] or {k: p[k].grad.detach().double().numpy().copy() for k in keys}
        opt.step()
        out["losses"].append(float(loss.detach().double()))
    out["losses"], out["tensors"] = np.array(out["losses"]), {k: p[k].detach().double().numpy() for k in keys}
    return keys, out


@pytest.mark.parametrize("which,mode,steps", [("vb", "fp32", 3), ("wide", "bf16", 3), ("llm", "fp32", 1)])
def test_gradients_and_trajectory(which, mode, steps):
    fx, floor = fixture(which), FLOORS[mode]
    tr = trainer(fx, max_grad_norm=MAX_NORM, compute_dtype=BF16 if mode == "bf16" else None)
    losses = [step(tr, fx)]
    (keys, yard), (_, run64) = yardstick(which, mode), yardstick(which, "fp64")
    grads = tr.grads()
    assert tuple(grads) == keys
    word = fx["prefix"] + "embeddings.word_embeddings.weight"
    assert not grads[word][fx["pad"]].any() and (fx["inp"]["input_ids"] == fx["pad"]).any() and grads[word].any()
    for k in keys:
        g, g64 = grads[k].astype(np.float64), run64["first"][k]
        if k.endswith("key.bias"):                       # mathematically zero: held against noise (test_gpu_finetune.py's rule)
            layer = [q for q in keys if q.endswith("key.bias")].index(k)
            assert (np.abs(g) <= 8 * np.maximum(np.abs(yard["keybias"][0][k]).max(), floor * run64["dk"][0][layer])).all(), k
            continue
        d_y, d_gpu = U.maxnorm_rel(yard["first"][k], g64), U.maxnorm_rel(g, g64)
        print(f"{which} {mode} grad {k}: d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_y, floor):.3f}")
        assert d_gpu <= 8 * max(d_y, floor), k
    if steps > 1:
        losses = np.array(losses + [step(tr, fx) for _ in range(steps - 1)])
        rule = (lambda *a: hold(*a, lr=LR)) if mode == "fp32" else (lambda *a: hold_trajectory(*a, lambda s: LR))
        rule(f"{which} embeddings {steps} steps", keys, losses, tr.state_dict(), yard, run64)


def test_refusals():
    fx = fixture("vb")
    model = model_of(fx)
    with pytest.raises(ValueError, match="train_layers must be 2"):
        trainer(fx, model, train_layers=1)
    with pytest.raises(ValueError, match="position_embeddings"):
        EncoderTrainer(model, {k: v for k, v in fx["sd"].items() if not k.endswith(".position_embeddings.weight")}, train_layers=2,
                       train_embeddings=True)
    tr = trainer(fx, model)
    inp = {k: torch.from_numpy(v) for k, v in fx["inp"].items()}
    with pytest.raises(ValueError, match="image_text_alignment"):
        tr.step(**inp, image_text_alignment=torch.zeros(inp["visual_embeds"].shape[:2] + (2,), dtype=torch.int64), labels=fx["labels"])
    assert tr.steps == 0


def test_commit():
    fx = fixture("wide")
    inp = {k: torch.from_numpy(v) for k, v in fx["inp"].items()}
    for flag in (True, False):
        model = model_of(fx, "bf16")
        enc = model.visual_bert
        frozen = {"ln": enc._ln["embeddings.LayerNorm"][0], "lin": enc._lin["embeddings.visual_projection"][0], **enc._tab}
        before, logits = {k: t.clone() for k, t in frozen.items()}, model(**inp).float().cpu()
        tr = trainer(fx, model, train_embeddings=flag, train_layers=2 if flag else 1)
        step(tr, fx)
        tr.commit()
        assert not torch.equal(model(**inp).float().cpu(), logits)
        for k, t in frozen.items():
            assert torch.equal(t, before[k]) != flag, k                 # every buffer of the stage moved, or none did
        for name, t in enc._tab.items() if flag else ():                # the masters, rounded once to the storage type
            assert torch.equal(t, tr.p[f"visual_bert.embeddings.{name}.weight"].to(torch.bfloat16)), name
