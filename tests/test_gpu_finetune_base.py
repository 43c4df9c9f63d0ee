"""GPU (-m gpu): `EncoderTrainer` at BERT-base width, in fp32 and in the mixed-precision mode.

tests/test_gpu_finetune.py and test_gpu_mixed_finetune.py hold the trainer to float64 at hidden 32 and 128 with I <= 256, where
`vk_gemm_f32` and `vk_gemm_16` always pick their 64 x 64 tile.  The BASE fixture (tests/finetune_util.py: hidden 768 in 12 heads of
d = 64, I = 3072, 2 layers, 16 sequences of 20 + 36 = 56 rows, so 896 rows) runs the top layer's products on both tiles (asserted
from the recorded calls by the launcher's rule) under the same rules and the same caps: first-step gradients and a 3-step
trajectory, the fp32 trainer against torch's fp32 and fp64 runs (`hold` of test_gpu_finetune.py), the mixed mode against
mixed_util's float64 restatement that rounds where the mode rounds (`hold_gradients`, `hold_trajectory` of
test_gpu_mixed_finetune.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import EncoderTrainer, step_lr                                             # noqa: E402
from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.visualbert import VisualBertForQuestionAnswering                           # noqa: E402

import finetune_util as U                                                                # noqa: E402
import mixed_util as X                                                                   # noqa: E402
import test_gpu_finetune as TF                                                           # noqa: E402
import test_gpu_mixed_finetune as MF                                                     # noqa: E402
from test_gpu_lxmert_pretrain import Recorder                                            # noqa: E402
from test_gpu_mixed_kernels import large_tile                                            # noqa: E402

BF16 = torch.bfloat16
LR_OF = lambda s: step_lr(*U.FIXTURE_STEP_LR)(U.FIXTURE_LR, s)                           # noqa: E731


class _Base:
    """The BASE fixture, built at first use: .CFG, .SD, .INPUTS, .LABELS."""
    long = False

    def __getattr__(self, name):
        made = dict(zip(("CFG", "SD", "INPUTS", "LABELS"), U.trajectory_fixture(base=True)))
        if name not in made:
            raise AttributeError(name)
        self.__dict__.update(made)
        return made[name]


FXB = _Base()


def trainer(**kw):
    model = VisualBertForQuestionAnswering(FXB.CFG, U.FIXTURE_LABELS, precision="fp32").load_state_dict(FXB.SD)
    return EncoderTrainer(model, FXB.SD, train_layers=1, lr=U.FIXTURE_LR, schedule=step_lr(*U.FIXTURE_STEP_LR), **kw)


def boundary():
    x = TF.boundary(1, FXB)
    assert x.shape == (16, 56, 768)
    return x


@functools.lru_cache(maxsize=None)
def yardstick32():
    """-> (keys, torch's fp32 run, torch's fp64 run) of 3 steps."""
    runs = [U.fixture_run(1, 3, dt, boundary(), base=True) for dt in (torch.float32, torch.float64)]
    return runs[0][0], runs[0][1], runs[1][1]


@functools.lru_cache(maxsize=None)
def yardstick16():
    """-> (keys, the bf16 yardstick's run, the fp64 run) of 3 steps; the fp64 run is yardstick32's."""
    keys, yard = X.fixture_run(1, 3, boundary(), BF16, base=True)
    return keys, yard, yardstick32()[2]


@functools.lru_cache(maxsize=None)
def gpu_run(mixed):
    """One trainer, one step, its gradients; two more steps, its losses and tensors."""
    tr = trainer(compute_dtype=BF16 if mixed else None)
    losses = list(TF.run_gpu(tr, 1, FXB))
    grads = tr.grads()
    losses += list(TF.run_gpu(tr, 2, FXB))
    assert tr.steps == 3 and tr.grad_norm is None
    return grads, np.array(losses), tr.state_dict()


def test_fp32_first_step_gradients():
    keys, run32, run64 = yardstick32()
    grads = gpu_run(False)[0]
    assert tuple(grads) == keys
    worst = 0.0
    for k in keys:
        g = grads[k].astype(np.float64)
        if k.endswith("key.bias"):
            gamma = TF.key_bias_gamma(k, keys, run32, run64, 0)
            print(f"base grad {k}: max |g| {np.abs(g).max():.2e} (torch fp32 {np.abs(run32['first'][k]).max():.2e}) worst |g| / gamma {(np.abs(g) / gamma).max():.3f}")
            assert (np.abs(g) <= gamma).all(), k
            continue
        d_cpu, d_gpu = U.maxnorm_rel(run32["first"][k], run64["first"][k]), U.maxnorm_rel(g, run64["first"][k])
        worst = max(worst, d_gpu / max(d_cpu, TF.FLOOR))
        print(f"base grad {k}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, TF.FLOOR):.2f}")
        assert d_gpu <= 8 * max(d_cpu, TF.FLOOR), k
    print(f"base fp32: worst gradient ratio {worst:.2f}")


def test_fp32_trajectory():
    keys, run32, run64 = yardstick32()
    _, losses, tensors = gpu_run(False)
    TF.hold("base n=1 3 steps", keys, losses, tensors, run32, run64)


def test_mixed_first_step_gradients():
    keys, yard, run64 = yardstick16()
    grads = gpu_run(True)[0]
    assert tuple(grads) == keys and all(g.dtype == np.float32 for g in grads.values())
    MF.hold_gradients("base mixed n=1", keys, grads, yard, run64)


def test_mixed_trajectory():
    keys, yard, run64 = yardstick16()
    _, losses, tensors = gpu_run(True)
    MF.hold_trajectory("base mixed n=1 3 steps", keys, losses, tensors, yard, run64, LR_OF)


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed"])
def test_a_step_runs_both_gemm_tiles_and_the_expected_attention(monkeypatch, mixed):
    """The tile of every recorded GEMM by the launcher's rule on its own (M, N); the forward's kernel asked of the dispatcher on
    the recorded arguments."""
    tr = trainer(compute_dtype=BF16 if mixed else None)
    pos, kw = TF.args(FXB)
    rec = Recorder(monkeypatch)                                                          # keeps (name, arguments)
    of = lambda name: [a for n, a in rec.calls if n == name]                             # noqa: E731
    loss = tr.step(*pos, labels=FXB.LABELS, **kw)
    assert np.isfinite(float(loss))
    gemm = "vk_gemm_16" if mixed else "vk_gemm_f32"
    shapes = [(a[9], a[10], a[11]) for a in of(gemm)]                                # M, N, K: the same positions in both entries
    tiles = {large_tile(M, N) for M, N, _ in shapes}
    print(f"{gemm}: " + ", ".join(f"{s} {'128' if large_tile(s[0], s[1]) else '64'}" for s in shapes))
    assert tiles == {False, True}, shapes
    assert (896, 2304, 768) in shapes and (896, 3072, 768) in shapes                     # the packed QKV projection, the intermediate
    entry, grad = ("vk_attention_tiled", "vk_attention_grad_16") if mixed else ("vk_attention", "vk_attention_grad")
    q, ldq, k, ldk, v, ldv, _, _, ldo, B, heads, Lq, Lk, d, dt, _ = of(entry)[-1]     # the trained layer's
    assert (ldq, ldk, ldv, ldo, B, heads, Lq, Lk, d) == (2304, 2304, 2304, 768, 16, 12, 56, 56, 64)
    assert dt == (L.VK_BF16 if mixed else L.VK_F32)
    route = L.load().vk_attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, int((q | k | v) % 16 == 0), int(mixed))
    assert route == (L.VK_ATT_ROUTE_TILED if mixed else L.VK_ATT_ROUTE_LDS), route
    assert len(of(grad)) == 1 and not of("vk_attention_grad" if mixed else "vk_attention_grad_16")
