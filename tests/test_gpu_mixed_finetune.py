"""GPU (-m gpu): `EncoderTrainer(compute_dtype=torch.bfloat16)`, the mixed-precision mode, end to end.

The yardstick is tests/mixed_util.py's restatement: the trained layers in float64 on the CPU with custom autograd functions that
round to bf16 exactly where the mode rounds (GEMM operands, the 16-bit GEMM outputs, P and dS, O and dO), torch's own AdamW and
clipping.  With d_y the max-norm relative distance of that run to the pure-float64 run, the GPU's distance to float64 may be at
most 8 * max(d_y, 2^-7), per gradient, per tensor and per step's loss: test_gpu_finetune.py's rule with bf16's epsilon in place of
fp32's.  Both runs start from the boundary hidden state the model's own frozen layers give.

`attention.self.key.bias` keeps its own rule (its gradient is mathematically zero) with the 16-bit unit:
|g[c]| <= gamma[c] = 8 * max(max |g_yardstick|, 2^-7 * sum_m |dK[m, c]|).  Its parameter bound is capped by the largest move AdamW
can make: with m = (1 - b1) sum b1^(t-i) g_i and v = (1 - b2) sum b2^(t-i) g_i^2, Cauchy-Schwarz gives
|m_hat| / sqrt(v_hat) <= c_t = (1 - b1) / (1 - b1^t) * sqrt(sum_{k<t} (b1^2 / b2)^k) * sqrt((1 - b2^t) / (1 - b2)), which is 1, 1.0014,
1.0037 for t = 1, 2, 3 at the default betas: a step moves a parameter by at most lr * c_t whatever its gradient (weight decay aside,
which both runs apply alike), so two runs are at most 2 * sum_t lr_t c_t apart.

Fixtures (tests/finetune_util.py): WIDE, hidden 128 in 4 heads of d = 32, 16 sequences of 16 rows; LONG, 2 heads of d = 64, 2
sequences of 140 rows (three 64-row tiles in the attention kernels); LayoutLM's small golden config."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import EncoderTrainer, step_lr                                             # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.layoutlm import LayoutLMForSequenceClassification                          # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering                           # noqa: E402

import finetune_util as U                                                                # noqa: E402
import mixed_util as X                                                                   # noqa: E402
from layoutlm_util import case_kwargs as llm_kwargs, golden_head                         # noqa: E402
from test_gpu_finetune import FX, FXL, Recorder, args, full_inputs, run_gpu              # noqa: E402

BF16 = torch.bfloat16
FLOOR = X.EPS16[BF16]                                     # 2^-7
ADAM_EPS, BETAS = 1e-8, (0.9, 0.999)
NL = U.FIXTURE_CFG["num_hidden_layers"]
MIXED_CALLS = {"vk_gemm_16", "vk_cast_16", "vk_attention_tiled", "vk_attention_grad_16"}


def cfg_sd(fx):
    """The fixture a bf16-capable head dim runs: the wide one (FX.W*: d = 32) or the long one (d = 64)."""
    return (fx.CFG, fx.SD) if fx.long else (fx.WCFG, fx.WSD)


def make(fx, precision="fp32"):
    cfg, sd = cfg_sd(fx)
    return VisualBertForQuestionAnswering(cfg, U.FIXTURE_LABELS, precision=precision).load_state_dict(sd)


def trainer(n, fx=FX, model=None, **kw):
    kw.setdefault("lr", U.FIXTURE_LR)
    kw.setdefault("schedule", step_lr(*U.FIXTURE_STEP_LR))
    kw.setdefault("compute_dtype", BF16)
    return EncoderTrainer(make(fx) if model is None else model, cfg_sd(fx)[1], train_layers=n, **kw)


@functools.lru_cache(maxsize=None)
def boundary(n, fx):
    """The fp32 model's own hidden state after its first NL - n layers -> [B, L, H] numpy."""
    x, _ = make(fx).visual_bert._hidden_after(NL - n, *full_inputs(fx))
    torch.cuda.synchronize()
    return x.float().cpu().numpy().reshape(fx.INPUTS["input_ids"].shape[0], -1, cfg_sd(fx)[0]["hidden_size"])


@functools.lru_cache(maxsize=None)
def yardstick(n, steps, fx, max_norm=None):
    """-> (keys, the bf16 yardstick's run, the pure-float64 run), computed once and shared."""
    runs = [X.fixture_run(n, steps, boundary(n, fx), dt, wide=not fx.long, long=fx.long, max_norm=max_norm) for dt in (BF16, None)]
    return runs[0][0], runs[0][1], runs[1][1]


def adam_move_cap(steps, lr_of):
    """sum_t lr_t c_t of the module docstring."""
    b1, b2 = BETAS
    total = 0.0
    for t in range(1, steps + 1):
        c = (1 - b1) / (1 - b1 ** t) * np.sqrt(sum((b1 * b1 / b2) ** k for k in range(t))) * np.sqrt((1 - b2 ** t) / (1 - b2))
        total += lr_of(t - 1) * c
    return total


def key_bias_gamma(key, keys, yard, run64, step):
    layer = [k for k in keys if k.endswith("key.bias")].index(key)
    return 8 * np.maximum(np.abs(yard["keybias"][step][key]).max(), FLOOR * run64["dk"][step][layer])


def hold_gradients(tag, keys, grads, yard, run64):
    worst = 0.0
    for k in keys:
        g = grads[k].astype(np.float64)
        if k.endswith("key.bias"):
            gamma = key_bias_gamma(k, keys, yard, run64, 0)
            print(f"{tag} grad {k}: max |g| {np.abs(g).max():.2e} (yardstick {np.abs(yard['first'][k]).max():.2e}) worst |g| / gamma {(np.abs(g) / gamma).max():.3f}")
            assert (np.abs(g) <= gamma).all(), k
            continue
        d_y, d_gpu = U.maxnorm_rel(yard["first"][k], run64["first"][k]), U.maxnorm_rel(g, run64["first"][k])
        worst = max(worst, d_gpu / max(d_y, FLOOR))
        print(f"{tag} grad {k}: d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_y, FLOOR):.3f}")
        assert d_gpu <= 8 * max(d_y, FLOOR), k
    print(f"{tag}: worst gradient ratio {worst:.3f}")


def hold_trajectory(tag, keys, losses, tensors, yard, run64, lr_of):
    worst, steps = 0.0, len(losses)
    rows = [(k, tensors[k], yard["tensors"][k], run64["tensors"][k]) for k in keys] + \
           [(f"loss[{i}]", losses[i], yard["losses"][i], run64["losses"][i]) for i in range(steps)]
    for name, got, ay, a64 in rows:
        if name.endswith("key.bias"):
            gamma = max(key_bias_gamma(name, keys, yard, run64, s).max() for s in range(steps))
            noise = sum(lr_of(s) for s in range(steps)) * gamma / ADAM_EPS
            bound = min(noise, 2 * adam_move_cap(steps, lr_of)) + 8 * 2.0 ** -23 * np.abs(a64).max()      # the masters are fp32
            dist = np.abs(np.asarray(got, np.float64) - a64).max()
            print(f"{tag} {name}: |p - p64| {dist:.2e} (yardstick {np.abs(ay - a64).max():.2e}) bound {bound:.2e} ratio {dist / bound:.3f}")
            assert dist <= bound, (tag, name, dist, bound)
            continue
        d_y, d_gpu = U.maxnorm_rel(ay, a64), U.maxnorm_rel(got, a64)
        worst = max(worst, d_gpu / max(d_y, FLOOR))
        print(f"{tag} {name}: d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_y, FLOOR):.3f}")
        assert d_gpu <= 8 * max(d_y, FLOOR), (tag, name, d_y, d_gpu)
    print(f"{tag}: worst ratio {worst:.3f}")


FIXTURES = {"wide": FX, "long": FXL}


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("which", ["wide", "long"])
def test_first_step_gradients(which, n):
    fx = FIXTURES[which]
    tr = trainer(n, fx)
    assert tr.compute_dtype is BF16
    run_gpu(tr, 1, fx)
    keys, yard, run64 = yardstick(n, 3, fx)
    grads = tr.grads()
    assert tuple(grads) == keys == tuple(tr.state_dict()) and all(g.dtype == np.float32 for g in grads.values())
    hold_gradients(f"{which} n={n}", keys, grads, yard, run64)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("which", ["wide", "long"])
def test_trajectory(which, n):
    fx = FIXTURES[which]
    tr = trainer(n, fx)
    losses = run_gpu(tr, 3, fx)
    assert tr.steps == 3 and tr.lr == U.FIXTURE_LR and tr.grad_norm is None
    keys, yard, run64 = yardstick(n, 3, fx)
    hold_trajectory(f"{which} n={n} 3 steps", keys, losses, tr.state_dict(), yard, run64, lambda s: step_lr(*U.FIXTURE_STEP_LR)(U.FIXTURE_LR, s))


def test_loss_falls():
    """60 steps on one batch of the wide fixture: the last loss is at most half the first, the project's cap; the yardstick's own
    figure beside it (test_mixed_host.py shows it clears the cap on the CPU oracle's boundary state)."""
    losses = run_gpu(trainer(1), 60)
    _, yard, _ = yardstick(1, 60, FX)
    print(f"mixed n=1: loss {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[-1] / losses[0]:.4f} x); yardstick {yard['losses'][0]:.4f} -> "
          f"{yard['losses'][-1]:.4f} ({yard['losses'][-1] / yard['losses'][0]:.4f} x)")
    assert losses[-1] <= 0.5 * losses[0]


def test_a_mixed_step_is_the_mixed_kernels(monkeypatch):
    """A recorded step over a bf16 model: the model's own launches through the frozen layer, then only the 16-bit kernels for the
    layer's products and attention: no vk_attention_grad, no vk_attention, and vk_gemm_f32 for the head's three products alone."""
    model = make(FX, "bf16")
    tr = trainer(1, model=model)
    pos, kw = args()
    rec = Recorder(monkeypatch)
    model.visual_bert.embeddings(*pos, **kw)
    n_embed = len(rec.calls)
    del rec.calls[:]
    model(*pos, **kw)
    whole = list(rec.calls)
    per_layer = (len(whole) - n_embed - 3) // NL                  # the pooler, the gather and `cls` close the model's forward
    del rec.calls[:]
    loss = tr.step(*pos, labels=FX.LABELS, **kw)
    frozen = n_embed + (NL - 1) * per_layer
    assert rec.calls[:frozen] == whole[:frozen]
    rest = rec.calls[frozen:]
    assert rest[:4] == ["vk_cast_16"] * 4 and rest[4:6] == ["vk_cast_16", "vk_gemm_16"]      # the four weight matrices, then x and the projection
    count = {name: rest.count(name) for name in set(rest)}
    # forward: QKV, attention output, intermediate, output; backward: four dW and dX of three (the lowest trained layer needs no dX)
    assert count["vk_gemm_16"] == 4 + 4 + 3
    # the four weight matrices; x, a, h; dt2, dz, dt1, dqkv
    assert count["vk_cast_16"] == 4 + 3 + 4
    assert count["vk_attention_tiled"] == 1 and count["vk_attention_grad_16"] == 1
    assert count["vk_gemm_f32"] == 3                                                     # logits, the head's dW and dX
    for name in ("vk_attention_grad", "vk_attention", "vk_linear"):
        assert name not in rest, name
    head_at = rest.index("vk_gemm_f32")
    assert MIXED_CALLS.issuperset(n for n in rest[:head_at] if "gemm" in n or "attention" in n or "cast" in n)
    assert np.isfinite(float(loss)) and tr.steps == 1
    # the fp32 mode on the same model issues none of them
    del rec.calls[:]
    trainer(1, model=model, compute_dtype=None).step(*pos, labels=FX.LABELS, **kw)
    assert not {"vk_gemm_16", "vk_cast_16", "vk_attention_grad_16"} & set(rec.calls) and "vk_attention_grad" in rec.calls


def same_bits(a, b):
    for x, y in ((a.grads(), b.grads()), (a.state_dict(), b.state_dict())):
        assert tuple(x) == tuple(y)
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


def test_none_is_the_trainer_without_the_argument():
    """compute_dtype=None beside a trainer built without the argument, in one process: the same bits, on the fixture whose head
    dim (8) the mixed mode refuses, and on the long one."""
    for fx in (FX, FXL):
        def build(**kw):
            model = VisualBertForQuestionAnswering(fx.CFG, U.FIXTURE_LABELS, precision="fp32").load_state_dict(fx.SD)
            return EncoderTrainer(model, fx.SD, train_layers=2, lr=U.FIXTURE_LR, schedule=step_lr(*U.FIXTURE_STEP_LR), max_grad_norm=1.0, **kw)
        a, b = build(), build(compute_dtype=None)
        assert a.compute_dtype is None and b.compute_dtype is None
        la, lb = run_gpu(a, 2, fx), run_gpu(b, 2, fx)
        assert la.tobytes() == lb.tobytes()
        same_bits(a, b)


def test_two_mixed_trainers_same_bits():
    a, b = trainer(2, max_grad_norm=1.0), trainer(2, max_grad_norm=1.0)
    la, lb = run_gpu(a, 3), run_gpu(b, 3)
    assert la.tobytes() == lb.tobytes()
    same_bits(a, b)


def test_huge_max_norm_is_bit_equal_to_none():
    a, b = trainer(2), trainer(2, max_grad_norm=1e9)
    la, lb = run_gpu(a, 3), run_gpu(b, 3)
    assert la.tobytes() == lb.tobytes() and b.grad_norm > 0 and a.grad_norm is None
    same_bits(a, b)


def test_clipping_follows_the_yardstick():
    tr = trainer(1, max_grad_norm=1.0)
    pos, kw = args()
    keys, yard, run64 = yardstick(1, 3, FX, 1.0)
    losses = []
    for i in range(3):
        losses.append(float(tr.step(*pos, labels=FX.LABELS, **kw)))
        d_y, d_gpu = abs(yard["norms"][i] - run64["norms"][i]) / run64["norms"][i], abs(tr.grad_norm - run64["norms"][i]) / run64["norms"][i]
        print(f"mixed step {i}: grad_norm {tr.grad_norm:.6f} (fp64 {run64['norms'][i]:.6f}) d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e}")
        assert d_gpu <= 8 * max(d_y, FLOOR)
    assert run64["norms"][0] > 1.0                          # the clip engaged
    hold_trajectory("wide n=1 clipped", keys, np.array(losses), tr.state_dict(), yard, run64, lambda s: step_lr(*U.FIXTURE_STEP_LR)(U.FIXTURE_LR, s))


def test_commit():
    """After 5 mixed steps over a bf16 model: nothing changes before commit(); after it the model's scores agree with the float64
    restatement on state_dict() under test_gpu_finetune.py's bf16 cap, and every frozen buffer keeps its bits."""
    cap = 8e-3
    model = make(FX, "bf16")
    enc, cfg = model.visual_bert, FX.WCFG
    pos, kw = args()
    before = model(*pos, **kw).float().cpu().numpy()
    tr = trainer(1, model=model, lr=1e-2, schedule=None)
    for _ in range(5):
        tr.step(*pos, labels=FX.LABELS, **kw)
    assert np.array_equal(model(*pos, **kw).float().cpu().numpy(), before), "the model changed before commit()"
    last = f"encoder.layer.{NL - 1}"
    frozen = {("lin", k): [t.clone() for t in v[:2]] for k, v in enc._lin.items() if not k.startswith(last) and k != "cls"}
    frozen.update({("ln", k): [t.clone() for t in v] for k, v in enc._ln.items() if not k.startswith(last)})
    frozen.update({("tab", k): [v.clone()] for k, v in enc._tab.items()})
    assert any(k.startswith("encoder.layer.0") for _, k in frozen)
    x0, _ = enc._hidden_after(NL - 1, *full_inputs())
    x0 = x0.float().cpu().numpy().reshape(before.shape[0], -1, cfg["hidden_size"])
    assert tr.commit() is model
    for (kind, k), old in frozen.items():
        new = {"lin": enc._lin, "ln": enc._ln, "tab": enc._tab}[kind][k]
        for o, n in zip(old, [new] if kind == "tab" else new):
            assert torch.equal(o.view(torch.uint8), n.view(torch.uint8)), f"frozen tensor {k} changed"
    after = model(*pos, **kw).float().cpu().numpy().astype(np.float64)
    st = tr.state_dict()
    assert all(v.dtype == np.float32 for v in st.values())
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in st.items()}
    mask01 = np.concatenate((FX.INPUTS["attention_mask"], FX.INPUTS["visual_attention_mask"]), 1)
    rows = torch.as_tensor(FX.INPUTS["attention_mask"].sum(1) - 2)
    ref = U.tail_logits(p, torch.tensor(x0, dtype=torch.float64), U.additive(mask01, torch.float64), [f"visual_bert.{last}"],
                        cfg["num_attention_heads"], cfg["layer_norm_eps"], "cls", rows, "visual_bert.").numpy()
    err = np.abs(after - ref).max() / np.abs(ref).max()
    moved = np.abs(after - before).max() / np.abs(before).max()
    print(f"commit after mixed steps: rel err of the trained model's scores {err:.2e}; moved by {moved:.2e}")
    assert err <= cap
    assert moved > 10 * cap, "the scores did not move"


def test_refusals():
    narrow = VisualBertForQuestionAnswering(FX.CFG, U.FIXTURE_LABELS, precision="fp32").load_state_dict(FX.SD)      # hidden 32 in 4 heads
    with pytest.raises(ValueError, match="head dim is 8"):
        EncoderTrainer(narrow, FX.SD, compute_dtype=BF16)
    model = make(FX)
    with pytest.raises(ValueError, match="loss scaling"):
        EncoderTrainer(model, FX.WSD, compute_dtype=torch.float16)
    with pytest.raises(ValueError, match="float64"):
        EncoderTrainer(model, FX.WSD, compute_dtype=torch.float64)
    assert EncoderTrainer(narrow, FX.SD, compute_dtype=None).compute_dtype is None
    tr = EncoderTrainer(model, FX.WSD, compute_dtype=BF16)
    with pytest.raises(AttributeError):
        tr.compute_dtype = None


def test_layoutlm(golden_dir):
    """LayoutLM's small golden config (hidden 128, 4 heads), one trained layer and the pooler, one step: gradients held."""
    g = np.load(os.path.join(golden_dir, "layoutlm_small.npz"))
    cfg, nlab, sd = golden_head(g, "seq")
    kw = {k: torch.from_numpy(v) for k, v in llm_kwargs(g, "short", "masked").items()}
    ids = torch.from_numpy(g["short/input_ids"])
    labels = np.array([1, U.IGNORE_INDEX, nlab - 1], np.int64)
    model = LayoutLMForSequenceClassification(cfg, nlab, precision="fp32").load_state_dict(sd)
    nl = cfg["num_hidden_layers"]
    x0, _ = model.layoutlm._hidden_after(nl - 1, ids, kw["bbox"], kw["attention_mask"], kw["token_type_ids"])
    x0 = x0.float().cpu().numpy().reshape(ids.shape[0], -1, cfg["hidden_size"])
    keys = U.trained_keys("layoutlm.", [nl - 1], "classifier")
    runs = [X.finetune_run(sd, keys, x0, kw["attention_mask"].numpy(), labels, 1, [f"layoutlm.encoder.layer.{nl - 1}"], cfg["num_attention_heads"],
                           cfg["layer_norm_eps"], "classifier", None, "layoutlm.", lr=1e-3, step_lr=(20, 0.9), compute_dtype=dt) for dt in (BF16, None)]
    tr = EncoderTrainer(model, sd, train_layers=1, lr=1e-3, schedule=step_lr(20, 0.9), compute_dtype=BF16)
    assert tuple(tr.state_dict()) == keys
    loss = float(tr.step(ids, labels=labels, **kw))
    d_y, d_gpu = abs(runs[0]["losses"][0] - runs[1]["losses"][0]) / runs[1]["losses"][0], abs(loss - runs[1]["losses"][0]) / runs[1]["losses"][0]
    print(f"layoutlm loss {loss:.5f} (fp64 {runs[1]['losses'][0]:.5f}) d_yardstick {d_y:.2e} d_gpu {d_gpu:.2e}")
    assert d_gpu <= 8 * max(d_y, FLOOR)
    hold_gradients("layoutlm n=1", keys, tr.grads(), runs[0], runs[1])
