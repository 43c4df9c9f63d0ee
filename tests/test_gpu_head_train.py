"""GPU (-m gpu): `vltk_amd.HeadTrainer` end to end.  The yardstick of a training run is torch itself: the same steps on the CPU in
fp32 and in fp64 (tests/train_util.py `torch_run`).  With d_cpu the max-norm relative distance of the fp32 run to the fp64 run, the
GPU's distance to fp64 may be at most 8 * max(d_cpu, 2^-23), per tensor and per step's loss: both are fp32 arithmetic in another
order, and the factor covers the erf / exp / rsqrt implementations and the GEMM's summation order.  The measured ratios are
printed (DESIGN.md section 26 records them)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import HeadTrainer, step_lr                                                # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.lxmert import LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict        # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering                           # noqa: E402
from vltk_amd.vit import ViTForImageClassification                                       # noqa: E402

import train_util as U                                                                   # noqa: E402
from lxmert_util import case_kwargs, golden_inputs                                       # noqa: E402
from visualbert_util import golden_inputs as vb_inputs, golden_qa_state_dict             # noqa: E402
from vit_util import golden_classifier                                                   # noqa: E402

EPS = {"fp32": 2e-5, "fp16": 1e-3, "bf16": 8e-3}          # one rounding of the storage type (+ margin): test_gpu_lxmert.py's
TINY = dict(vocab_size=64, hidden_size=32, num_attention_heads=4, intermediate_size=64, l_layers=1, x_layers=1, r_layers=1,
            max_position_embeddings=16, visual_feat_dim=64)
FLOOR = 2.0 ** -23


class Recorder:
    """L.call with every call's name kept."""

    def __init__(self, monkeypatch):
        self.calls, real = [], L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (self.calls.append(name), real(name, *a))[1])


@pytest.fixture(scope="module")
def tiny_lxmert():
    """-> make(): a fresh LxmertForQuestionAnswering (hidden 32, 16 answers, fp32) whose head holds the fixture's weights."""
    cfg = lxmert_config(**TINY)
    keys, head, feats, labels = U.head_fixture()
    sd = make_lxmert_qa_state_dict(cfg, 16, seed=1)
    sd.update(head)
    return lambda: LxmertForQuestionAnswering(cfg, 16, precision="fp32").load_state_dict(sd), keys, head, feats, labels


@functools.lru_cache(maxsize=None)
def yardstick(kind, steps, hidden=32, answers=16, prefix="cls"):
    keys, head, feats, labels = U.head_fixture(hidden, answers, kind=kind, prefix=prefix)
    return [U.torch_run(head, keys, feats, labels, steps, dt, step_lr=(20, 0.9)) for dt in (torch.float32, torch.float64)]


def hold_to_yardstick(tag, keys, losses, tensors, run32, run64, what="tensor"):
    worst = 0.0
    for name, got, a32, a64 in [(k, tensors[k], run32[1][k], run64[1][k]) for k in keys] + \
            [(f"loss[{i}]", losses[i], run32[0][i], run64[0][i]) for i in range(len(losses))]:
        d_cpu, d_gpu = U.maxnorm_rel(a32, a64), U.maxnorm_rel(got, a64)
        ratio = d_gpu / max(d_cpu, FLOOR)
        worst = max(worst, ratio)
        print(f"{tag} {name}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {ratio:.2f}")
        assert d_gpu <= 8 * max(d_cpu, FLOOR), (tag, name, d_cpu, d_gpu)
    print(f"{tag}: worst ratio {worst:.2f}")


def run_gpu(trainer, feats, labels, steps):
    x = torch.from_numpy(feats).cuda()
    return np.array([float(trainer.step_features(x, labels)) for _ in range(steps)], np.float64)


@pytest.mark.parametrize("steps", [5, 20])
def test_trajectory_lxmert_head(tiny_lxmert, steps):
    make, keys, head, feats, labels = tiny_lxmert
    tr = HeadTrainer(make(), lr=1e-3, schedule=step_lr(20, 0.9))
    losses = run_gpu(tr, feats, labels, steps)
    assert tr.steps == steps and tr.lr == (1e-3 if steps < 20 else 1e-3 * 0.9)
    hold_to_yardstick(f"lxmert {steps} steps", keys, losses, tr.state_dict(), *yardstick("lxmert", steps))


def test_first_step_gradients(tiny_lxmert):
    make, keys, head, feats, labels = tiny_lxmert
    tr = HeadTrainer(make(), lr=1e-3)
    run_gpu(tr, feats, labels, 1)
    (_, _, g32), (_, _, g64) = yardstick("lxmert", 5)
    grads = tr.grads()
    assert set(grads) == set(keys)
    for k in keys:
        d_cpu, d_gpu = U.maxnorm_rel(g32[k], g64[k]), U.maxnorm_rel(grads[k], g64[k])
        print(f"grad {k}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, FLOOR):.2f}")
        assert d_gpu <= 8 * max(d_cpu, FLOOR), k


def test_loss_falls(tiny_lxmert):
    """60 steps at 1e-3 on one batch: the last loss is at most half the first (test_train_host.py shows torch's own run on this
    fixture clears the cap)."""
    make, keys, head, feats, labels = tiny_lxmert
    losses = run_gpu(HeadTrainer(make(), lr=1e-3), feats, labels, 60)
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[-1] / losses[0]:.3f} x)")
    assert losses[-1] <= 0.5 * losses[0]


def _single_linear_models(golden_dir):
    g = np.load(os.path.join(golden_dir, "visualbert_small.npz"))
    cfg, _, _ = vb_inputs(g, "short")
    yield "cls", VisualBertForQuestionAnswering, (cfg, int(g["qa/num_labels"])), golden_qa_state_dict(g)
    g = np.load(os.path.join(golden_dir, "vit_small.npz"))
    cfg, sd, n = golden_classifier(g)
    yield "classifier", ViTForImageClassification, (cfg, n), sd


@pytest.mark.parametrize("which", [0, 1], ids=["visualbert", "vit"])
def test_trajectory_single_linear_heads(golden_dir, which):
    prefix, cls, args, sd = list(_single_linear_models(golden_dir))[which]
    hidden, answers = args[0]["hidden_size"], args[1]
    keys, head, feats, labels = U.head_fixture(hidden, answers, kind="linear", prefix=prefix)
    sd = dict(sd)
    sd.update(head)
    tr = HeadTrainer(cls(*args, precision="fp32").load_state_dict(sd), lr=1e-3, schedule=step_lr(20, 0.9))
    assert tuple(tr.state_dict()) == keys
    losses = run_gpu(tr, feats, labels, 3)
    hold_to_yardstick(f"{prefix} 3 steps", keys, losses, tr.state_dict(), *yardstick("linear", 3, hidden, answers, prefix))


# ---- through the encoder: the golden small LXMERT ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(golden_dir):
    g = np.load(os.path.join(golden_dir, "lxmert_small.npz"))
    cfg, _, feats = golden_inputs(g)
    nqa = int(g["qa/num_labels"])
    sd = make_lxmert_qa_state_dict(cfg, nqa, int(g["seed"]))
    inputs = (torch.from_numpy(g["input_ids"]), torch.from_numpy(feats), torch.from_numpy(g["visual_pos"]))
    kw = {k: torch.from_numpy(v) for k, v in case_kwargs(g, "masked").items()}
    return cfg, nqa, sd, inputs, kw


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_step_equals_step_features(small, precision):
    cfg, nqa, sd, inputs, kw = small
    model = LxmertForQuestionAnswering(cfg, nqa, precision=precision).load_state_dict(sd)
    labels = np.array([1, -100, nqa - 1], np.int64)
    a, b = HeadTrainer(model, lr=1e-3), HeadTrainer(model, lr=1e-3)
    la = a.step(*inputs, labels=labels, **kw)
    lb = b.step_features(model.head_features(*inputs, **kw), labels)
    assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    for x, y in ((a.grads(), b.grads()), (a.state_dict(), b.state_dict())):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_commit(small, precision):
    cfg, nqa, sd, inputs, kw = small
    model = LxmertForQuestionAnswering(cfg, nqa, precision=precision).load_state_dict(sd)
    enc = model.lxmert
    before = model(*inputs, **kw).float().cpu().numpy()
    tr = HeadTrainer(model, lr=1e-2)
    feats = model.head_features(*inputs, **kw)
    for _ in range(5):
        tr.step_features(feats, np.array([1, 2, nqa - 1], np.int64))
    assert np.array_equal(model(*inputs, **kw).float().cpu().numpy(), before), "the model changed before commit()"
    head_lin, head_ln = ("answer.fc0", "answer.fc3"), ("answer_head.logit_fc.2",)
    frozen = {("lin", k): [t.clone() for t in v[:2]] for k, v in enc._lin.items() if k not in head_lin}
    frozen.update({("ln", k): [t.clone() for t in v] for k, v in enc._ln.items() if k not in head_ln})
    frozen.update({("tab", k): [v.clone()] for k, v in enc._tab.items()})
    assert tr.commit() is model
    for (kind, k), old in frozen.items():
        new = {"lin": enc._lin, "ln": enc._ln, "tab": enc._tab}[kind][k]
        for o, n in zip(old, [new] if kind == "tab" else new):
            assert torch.equal(o.view(torch.uint8), n.view(torch.uint8)), f"encoder tensor {k} changed"
    after = model(*inputs, **kw).float().cpu().numpy().astype(np.float64)
    st = tr.state_dict()
    assert tuple(st) == U.LXMERT_KEYS and all(v.dtype == np.float32 for v in st.values())
    ref = U.head_logits({k: torch.from_numpy(v).double() for k, v in st.items()}, feats.double().cpu(), U.LXMERT_KEYS).numpy()
    err = np.abs(after - ref).max() / np.abs(ref).max()
    print(f"commit {precision}: rel err of the trained head's scores {err:.2e}; moved by {np.abs(after - before).max() / np.abs(before).max():.2e}")
    assert err <= EPS[precision]
    assert np.abs(after - before).max() > 10 * EPS[precision] * np.abs(before).max(), "the scores did not move"


def test_refusals(tiny_lxmert, monkeypatch):
    make, keys, head, feats, labels = tiny_lxmert
    tr = HeadTrainer(make())
    x = torch.from_numpy(feats).cuda()
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="-100"):
        tr.step_features(x, np.full(len(feats), -100, np.int64))
    bad = labels.copy()
    bad[5] = 16
    with pytest.raises(IndexError):
        tr.step_features(x, bad)
    with pytest.raises(ValueError):
        tr.step_features(x, labels[:-1])
    with pytest.raises(ValueError):
        tr.step_features(x[:, :-1], labels)
    assert rec.calls == [] and tr.steps == 0
    with pytest.raises(TypeError):
        HeadTrainer(make().lxmert)
