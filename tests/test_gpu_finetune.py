"""GPU (-m gpu): `vltk_amd.EncoderTrainer` end to end.  The yardstick is torch itself: the same steps on the CPU in fp32 and in
fp64 (tests/finetune_util.py `torch_finetune_run`) from the boundary hidden state the model's own frozen layers give.  With d_cpu
the max-norm relative distance of torch's fp32 run to its fp64 run, the GPU's distance to fp64 may be at most
8 * max(d_cpu, 2^-23), per tensor, per gradient and per step's loss (test_gpu_head_train.py's rule, for its reason: fp32 arithmetic
in another order).

`attention.self.key.bias` has its own rule: its gradient is mathematically zero (soft-max ignores a shift of a score row), so what
anyone computes for it is rounding noise, and AdamW divides noise below its eps by eps.  Gradient: |g[c]| <= gamma[c] =
8 * max(max |g32|, 2^-23 * sum_m |dK[m, c]|).  Tensor after `steps` steps: |p - p64| <= steps * lr * gamma / eps + 8 * 2^-23 * max |p|,
gamma the largest of the steps.  The measured ratios are printed (DESIGN.md section 27 records them).

The fixture runs 16 rows of d = 8, so its fp32 forward is the LDS kernel; the `long` fixture (140 rows of d = 64) is past that
kernel's image and runs attention_stream_kernel, which divides by l where the backward multiplies by 1 / l: the same rules."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import EncoderTrainer, step_lr                                             # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.layoutlm import LayoutLMForSequenceClassification                          # noqa: E402
from vltk_amd.lxmert import LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict        # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering, make_visualbert_qa_state_dict           # noqa: E402
from vltk_amd.vit import ViTForImageClassification                                       # noqa: E402

import finetune_util as U                                                                # noqa: E402
from layoutlm_util import case_kwargs as llm_kwargs, golden_head                         # noqa: E402
from vit_util import golden_classifier                                                   # noqa: E402

EPS = {"fp32": 2e-5, "bf16": 8e-3}                        # test_gpu_head_train.py's: one rounding of the storage type (+ margin)
FLOOR = 2.0 ** -23
ADAM_EPS = 1e-8
NL = U.FIXTURE_CFG["num_hidden_layers"]


class _Fixture:
    """The trajectory fixture, built at first use (collection builds nothing): .CFG, .SD, .INPUTS, .LABELS at hidden 32, and .WCFG,
    .WSD at hidden 128, what a bf16 model can run; its inputs and labels are the same draws.  `long`: the fixture of 140 rows."""

    def __init__(self, long=False):
        self.long = long

    def __getattr__(self, name):
        wide = name.startswith("W")
        made = dict(zip(("CFG", "SD", "INPUTS", "LABELS"), U.trajectory_fixture(wide=wide, long=self.long)))
        if name[wide:] not in made:
            raise AttributeError(name)
        for k, v in made.items():
            setattr(self, "W" * wide + k, v)
        return self.__dict__[name]


FX = _Fixture()
FXL = _Fixture(long=True)                                 # Lx = 140, d = 64: the trainer's fp32 forward runs the streaming kernel


class Recorder:
    """L.call with every call's name kept."""

    def __init__(self, monkeypatch):
        self.calls, real = [], L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (self.calls.append(name), real(name, *a))[1])


def make(precision="fp32", fx=FX):
    """The fixture's model; a bf16 model is the wide one (its pooler takes hidden sizes in multiples of 64)."""
    cfg, sd = (fx.CFG, fx.SD) if precision == "fp32" else (fx.WCFG, fx.WSD)
    return VisualBertForQuestionAnswering(cfg, U.FIXTURE_LABELS, precision=precision).load_state_dict(sd)


def args(fx=FX):
    """(positional inputs, keyword inputs) of the fixture as tensors."""
    t = {k: torch.from_numpy(v) for k, v in fx.INPUTS.items()}
    return (t["input_ids"], t["visual_embeds"]), dict(attention_mask=t["attention_mask"], visual_attention_mask=t["visual_attention_mask"])


def full_inputs(fx=FX):
    pos, kw = args(fx)
    return pos + (kw["attention_mask"], kw["visual_attention_mask"], None, None, None)


def trainer(n, model=None, sd=None, fx=FX, **kw):
    kw.setdefault("lr", U.FIXTURE_LR)
    kw.setdefault("schedule", step_lr(*U.FIXTURE_STEP_LR))
    return EncoderTrainer(make(fx=fx) if model is None else model, fx.SD if sd is None else sd, train_layers=n, **kw)


def run_gpu(tr, steps, fx=FX):
    pos, kw = args(fx)
    return np.array([float(tr.step(*pos, labels=fx.LABELS, **kw)) for _ in range(steps)], np.float64)


@functools.lru_cache(maxsize=None)
def boundary(n, fx=FX):
    """The fp32 model's own hidden state after its first NL - n layers -> [B, L, H] numpy."""
    enc = make(fx=fx).visual_bert
    x, _ = enc._hidden_after(NL - n, *full_inputs(fx))
    torch.cuda.synchronize()
    return x.float().cpu().numpy().reshape(fx.INPUTS["input_ids"].shape[0], -1, fx.CFG["hidden_size"])


@functools.lru_cache(maxsize=None)
def yardstick(n, steps, max_norm=None, fx=FX):
    runs = [U.fixture_run(n, steps, dt, boundary(n, fx), max_norm=max_norm, long=fx.long) for dt in (torch.float32, torch.float64)]
    return runs[0][0], runs[0][1], runs[1][1]


def key_bias_gamma(key, keys, run32, run64, step):
    """gamma[c] of one step for one key.bias tensor."""
    layer = [k for k in keys if k.endswith("key.bias")].index(key)
    return 8 * np.maximum(np.abs(run32["keybias"][step][key]).max(), FLOOR * run64["dk"][step][layer])


def hold(tag, keys, losses, tensors, run32, run64, lr=U.FIXTURE_LR):
    worst, steps = 0.0, len(losses)
    rows = [(k, tensors[k], run32["tensors"][k], run64["tensors"][k]) for k in keys] + \
           [(f"loss[{i}]", losses[i], run32["losses"][i], run64["losses"][i]) for i in range(steps)]
    for name, got, a32, a64 in rows:
        if name.endswith("key.bias"):
            gamma = max(key_bias_gamma(name, keys, run32, run64, s).max() for s in range(steps))
            bound = steps * lr * gamma / ADAM_EPS + 8 * FLOOR * np.abs(a64).max()
            dist = np.abs(np.asarray(got, np.float64) - a64).max()
            print(f"{tag} {name}: |p - p64| {dist:.2e} (torch fp32 {np.abs(a32 - a64).max():.2e}) bound {bound:.2e} ratio {dist / bound:.3f}")
            assert dist <= bound, (tag, name, dist, bound)
            continue
        d_cpu, d_gpu = U.maxnorm_rel(a32, a64), U.maxnorm_rel(got, a64)
        ratio = d_gpu / max(d_cpu, FLOOR)
        worst = max(worst, ratio)
        print(f"{tag} {name}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {ratio:.2f}")
        assert d_gpu <= 8 * max(d_cpu, FLOOR), (tag, name, d_cpu, d_gpu)
    print(f"{tag}: worst ratio {worst:.2f}")


def first_step_gradients(n, fx):
    tr = trainer(n, fx=fx)
    run_gpu(tr, 1, fx)
    keys, run32, run64 = yardstick(n, 3, fx=fx)
    grads = tr.grads()
    assert tuple(grads) == keys == tuple(tr.state_dict())
    for k in keys:
        g = grads[k].astype(np.float64)
        if k.endswith("key.bias"):
            gamma = key_bias_gamma(k, keys, run32, run64, 0)
            print(f"grad {k}: max |g| {np.abs(g).max():.2e} (torch fp32 {np.abs(run32['first'][k]).max():.2e}) worst |g| / gamma {(np.abs(g) / gamma).max():.3f}")
            assert (np.abs(g) <= gamma).all(), k
            continue
        d_cpu, d_gpu = U.maxnorm_rel(run32["first"][k], run64["first"][k]), U.maxnorm_rel(g, run64["first"][k])
        print(f"grad {k}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, FLOOR):.2f}")
        assert d_gpu <= 8 * max(d_cpu, FLOOR), k


@pytest.mark.parametrize("n", [1, 2])
def test_first_step_gradients(n):
    first_step_gradients(n, FX)


def trajectory(n, steps, fx, tag=""):
    tr = trainer(n, fx=fx)
    losses = run_gpu(tr, steps, fx)
    assert tr.steps == steps and tr.lr == U.FIXTURE_LR and tr.grad_norm is None
    keys, run32, run64 = yardstick(n, steps, fx=fx)
    hold(f"{tag}n={n} {steps} steps", keys, losses, tr.state_dict(), run32, run64)


@pytest.mark.parametrize("steps", [3, 10])
@pytest.mark.parametrize("n", [1, 2])
def test_trajectory(n, steps):
    trajectory(n, steps, FX)


# ---- the trainer where its forward streams: Lx = 140 rows, 2 heads of d = 64 (the LDS kernel's image would be 187 600 bytes) -----------
def streams(fx):
    """The fixture's attention runs attention_stream_kernel: asked of the dispatcher on the trainer's packed projection."""
    Lx = fx.INPUTS["input_ids"].shape[1] + fx.INPUTS["visual_embeds"].shape[1]
    H, heads = fx.CFG["hidden_size"], fx.CFG["num_attention_heads"]
    assert (Lx, H // heads, 3 * H) == (140, 64, 384) and fx.INPUTS["input_ids"].shape[0] == 2
    assert not fx.INPUTS["attention_mask"].all() and not fx.INPUTS["visual_attention_mask"].all()          # both masks are partial
    return L.load().vk_attention_route(140, 140, 64, L.VK_F32, 384, 384, 384, 1, 0) == L.VK_ATT_ROUTE_STREAM


def test_first_step_gradients_where_the_forward_streams(monkeypatch):
    """The forward divides by l (attention_stream_kernel), the backward multiplies by 1 / l: the pair under the file's rules."""
    assert streams(FXL)
    rec = Recorder(monkeypatch)
    first_step_gradients(2, FXL)
    assert rec.calls.count("vk_attention") == NL and rec.calls.count("vk_attention_grad") == 2


def test_trajectory_where_the_forward_streams():
    assert streams(FXL)
    trajectory(2, 3, FXL, "Lx=140 ")


@pytest.mark.parametrize("n", [1, 2])
def test_clipping(n):
    tr = trainer(n, max_grad_norm=1.0)
    pos, kw = args()
    keys, run32, run64 = yardstick(n, 3, 1.0)
    losses = []
    for i in range(3):
        losses.append(float(tr.step(*pos, labels=FX.LABELS, **kw)))
        d_cpu, d_gpu = abs(run32["norms"][i] - run64["norms"][i]) / run64["norms"][i], abs(tr.grad_norm - run64["norms"][i]) / run64["norms"][i]
        print(f"n={n} step {i}: grad_norm {tr.grad_norm:.6f} (fp64 {run64['norms'][i]:.6f}) d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e}")
        assert d_gpu <= 8 * max(d_cpu, FLOOR)
    assert run64["norms"][0] > 1.0                          # the clip engaged
    hold(f"n={n} clipped", keys, np.array(losses), tr.state_dict(), run32, run64)


def test_huge_max_norm_is_bit_equal_to_none():
    a, b = trainer(2), trainer(2, max_grad_norm=1e9)
    la, lb = run_gpu(a, 3), run_gpu(b, 3)
    assert la.tobytes() == lb.tobytes() and b.grad_norm > 0
    for x, y in ((a.grads(), b.grads()), (a.state_dict(), b.state_dict())):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


@pytest.mark.parametrize("n", [1, 2])
def test_loss_falls(n):
    """60 steps on one batch: the last loss is at most half the first (test_finetune_host.py shows torch's own run clears it)."""
    losses = run_gpu(trainer(n), 60)
    print(f"n={n}: loss {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[-1] / losses[0]:.3f} x)")
    assert losses[-1] <= 0.5 * losses[0]


def test_two_trainers_same_bits():
    a, b = trainer(2, max_grad_norm=1.0), trainer(2, max_grad_norm=1.0)
    la, lb = run_gpu(a, 3), run_gpu(b, 3)
    assert la.tobytes() == lb.tobytes()
    for x, y in ((a.grads(), b.grads()), (a.state_dict(), b.state_dict())):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


def test_bf16_step_runs_the_models_own_frozen_launches(monkeypatch):
    assert all(np.array_equal(FX.INPUTS[k], FX.WINPUTS[k]) for k in FX.INPUTS) and np.array_equal(FX.LABELS, FX.WLABELS)
    model = make("bf16")
    tr = trainer(1, model=model, sd=FX.WSD)
    pos, kw = args()
    rec = Recorder(monkeypatch)
    model.visual_bert.embeddings(*pos, **kw)
    n_embed = len(rec.calls)
    del rec.calls[:]
    model(*pos, **kw)
    whole = list(rec.calls)
    per_layer = (len(whole) - n_embed - 3) // NL                  # the pooler, the gather and `cls` close the model's forward
    assert whole[:n_embed + NL * per_layer] == whole[:n_embed] + whole[n_embed:n_embed + per_layer] * NL
    del rec.calls[:]
    loss = tr.step(*pos, labels=FX.LABELS, **kw)
    frozen = n_embed + (NL - 1) * per_layer
    assert rec.calls[:frozen] == whole[:frozen]
    assert rec.calls[frozen] == "vk_gemm_f32" and "vk_linear" not in rec.calls[frozen:] and "vk_attention_grad" in rec.calls
    assert np.isfinite(float(loss)) and tr.steps == 1


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_commit(precision):
    model = make(precision)
    enc = model.visual_bert
    cfg = enc.cfg
    pos, kw = args()
    before = model(*pos, **kw).float().cpu().numpy()
    seq_before = enc(*pos, **kw)[0].float().cpu().numpy()
    replay = enc.capture(*pos, **kw)
    tr = trainer(1, model=model, sd=FX.SD if precision == "fp32" else FX.WSD, lr=1e-2, schedule=None)
    for _ in range(5):
        tr.step(*pos, labels=FX.LABELS, **kw)
    assert np.array_equal(model(*pos, **kw).float().cpu().numpy(), before), "the model changed before commit()"
    last = f"encoder.layer.{NL - 1}"
    frozen = {("lin", k): [t.clone() for t in v[:2]] for k, v in enc._lin.items() if not k.startswith(last) and k != "cls"}
    frozen.update({("ln", k): [t.clone() for t in v] for k, v in enc._ln.items() if not k.startswith(last)})
    frozen.update({("tab", k): [v.clone()] for k, v in enc._tab.items()})
    assert any(k.startswith("encoder.layer.0") for _, k in frozen) and ("lin", "pooler.dense") in frozen
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
    print(f"commit {precision}: rel err of the trained model's scores {err:.2e}; moved by {moved:.2e}")
    assert err <= EPS[precision]
    assert moved > 10 * EPS[precision], "the scores did not move"
    # the graph captured before commit() reads the same buffers: it replays with the new weights
    seq_replayed = replay(*pos, **kw)[0].float().cpu().numpy()
    seq_eager = enc(*pos, **kw)[0].float().cpu().numpy()
    assert np.array_equal(seq_replayed, seq_eager) and not np.array_equal(seq_replayed, seq_before)


def test_layoutlm(golden_dir):
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
    assert "layoutlm.pooler.dense.weight" in keys
    runs = [U.torch_finetune_run(sd, keys, x0, kw["attention_mask"].numpy(), labels, 3, dt, [f"layoutlm.encoder.layer.{nl - 1}"],
                                 cfg["num_attention_heads"], cfg["layer_norm_eps"], "classifier", None, "layoutlm.", lr=1e-3, step_lr=(20, 0.9))
            for dt in (torch.float32, torch.float64)]
    tr = EncoderTrainer(model, sd, train_layers=1, lr=1e-3, schedule=step_lr(20, 0.9))
    assert tuple(tr.state_dict()) == keys
    losses = np.array([float(tr.step(ids, labels=labels, **kw)) for _ in range(3)])
    hold("layoutlm 3 steps", keys, losses, tr.state_dict(), runs[0], runs[1], lr=1e-3)


def test_refusals(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, "vit_small.npz"))
    cfg, sd, n = golden_classifier(g)
    with pytest.raises(TypeError, match="pre-LN"):
        EncoderTrainer(ViTForImageClassification(cfg, n, precision="fp32").load_state_dict(sd), sd)
    lcfg = lxmert_config(vocab_size=64, hidden_size=32, num_attention_heads=4, intermediate_size=64, l_layers=1, x_layers=1, r_layers=1,
                         max_position_embeddings=16, visual_feat_dim=64)
    lsd = make_lxmert_qa_state_dict(lcfg, 16, seed=1)
    with pytest.raises(TypeError, match="cross-attention"):
        EncoderTrainer(LxmertForQuestionAnswering(lcfg, 16, precision="fp32").load_state_dict(lsd), lsd)
    model = make()
    with pytest.raises(ValueError, match="HeadTrainer"):
        EncoderTrainer(model, FX.SD, train_layers=0)
    with pytest.raises(ValueError, match="train_layers"):
        EncoderTrainer(model, FX.SD, train_layers=NL + 1)
    with pytest.raises(ValueError, match="checkpoint"):
        EncoderTrainer(model, make_visualbert_qa_state_dict(FX.CFG, U.FIXTURE_LABELS, U.FIXTURE_SEED + 1))
    tr = trainer(1, model=model)
    pos, kw = args()
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="-100"):
        tr.step(*pos, labels=np.full(len(FX.LABELS), -100, np.int64), **kw)
    bad = FX.LABELS.copy()
    bad[5] = U.FIXTURE_LABELS
    with pytest.raises(IndexError):
        tr.step(*pos, labels=bad, **kw)
    with pytest.raises(ValueError):
        tr.step(*pos, labels=FX.LABELS[:-1], **kw)
    assert rec.calls == [] and tr.steps == 0
