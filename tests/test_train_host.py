"""CPU (-m "not gpu"): the host side of head training (vltk_amd/train.py, csrc/train.hip's entry points): the schedules against
torch's schedulers, the written-out AdamW against torch.optim.AdamW, the GEMM's argument check, the ABI, and the refusal without
a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import train as T

import train_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_gemm_f32", "vk_gemm_f32_check", "vk_col_sums", "vk_col_sums_workspace_bytes", "vk_cross_entropy_grad", "vk_act_f32",
       "vk_act_grad_f32", "vk_layernorm_grad", "vk_layernorm_grad_workspace_bytes", "vk_adamw_step")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _torch_rates(make_sched, base, n):
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=base)
    sched = make_sched(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def test_step_lr_is_torch_steplr():
    rate = T.step_lr(200, 0.9)
    want = _torch_rates(lambda o: torch.optim.lr_scheduler.StepLR(o, 200, 0.9), 1e-4, 451)
    assert [rate(1e-4, t) for t in range(451)] == want
    assert want[0] == 1e-4 and want[200] != want[199] and want[400] != want[399]
    with pytest.raises(ValueError):
        T.step_lr(0, 0.9)


def test_linear_warmup_is_transformers_lambda():
    """get_linear_schedule_with_warmup's lambda (written out here, as transformers/optimization.py has it) under LambdaLR."""
    def lr_lambda(step, warm=10, total=100):
        if step < warm:
            return float(step) / float(max(1, warm))
        return max(0.0, float(total - step) / float(max(1, total - warm)))
    rate = T.linear_warmup(10, 100)
    want = _torch_rates(lambda o: torch.optim.lr_scheduler.LambdaLR(o, lr_lambda), 1e-4, 451)
    assert [rate(1e-4, t) for t in range(451)] == want
    assert want[0] == 0.0 and want[10] == 1e-4 and want[100] == 0.0 and want[450] == 0.0


@pytest.mark.parametrize("decay", [True, False])
def test_written_out_adamw_is_torch_adamw(decay):
    """The rule, not a kernel: float64, 5 steps, 1e-15 relative."""
    r = np.random.Generator(np.random.PCG64(3))
    p0 = r.standard_normal(257)
    grads = [r.standard_normal(257) * 10.0 ** r.integers(-6, 1) for _ in range(5)]
    grads[2][::7] = 0.0
    wd = 0.01 if decay else 0.0
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(257), np.zeros(257)
    for step, g in enumerate(grads, 1):
        pt.grad = torch.tensor(g)
        opt.step()
        p, m, v, _ = U.adamw_f64(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, decay=decay)
        assert np.abs(p - pt.detach().numpy()).max() <= 1e-15 * np.abs(p).max()
    st = opt.state[pt]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-15 * np.abs(m).max()
    assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-15 * np.abs(v).max()
    assert T.bias_corrections(0.9, 0.999, 3) == (1 - 0.9 ** 3, 1 - 0.999 ** 3)


def test_gemm_check_refuses_each_bad_argument(lib):
    ok = dict(M=5, N=7, K=3, lda=3, ldb=3, ldc=7, transA=0, transB=1)

    def check(**kw):
        a = {**ok, **kw}
        return lib.vk_gemm_f32_check(a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], a["transA"], a["transB"])
    assert check() == L.VK_OK
    assert check(transA=1, lda=5) == L.VK_OK and check(transB=0, ldb=7) == L.VK_OK
    for bad in (dict(M=0), dict(N=0), dict(K=-1), dict(lda=2), dict(ldb=2), dict(ldc=6), dict(transA=2), dict(transB=-1),
                dict(transA=1, lda=4), dict(transB=0, ldb=6)):
        assert check(**bad) == L.VK_EINVAL, bad
        assert b"gemm_f32" in lib.vk_last_error()
    with pytest.raises(ValueError, match="lda"):
        L.call("vk_gemm_f32_check", 5, 7, 3, 2, 3, 7, 0, 1)


def test_new_symbols_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(L.vk_adamw_tensor) == 48 and L.vk_adamw_tensor.n.offset == 32 and L.vk_adamw_tensor.decay.offset == 40
    import vltk_amd
    assert vltk_amd.HeadTrainer is T.HeadTrainer and vltk_amd.step_lr is T.step_lr and vltk_amd.linear_warmup is T.linear_warmup


def test_workspace_sizes(lib):
    assert lib.vk_col_sums_workspace_bytes(256, 100) == 0
    assert lib.vk_col_sums_workspace_bytes(257, 100) == 2 * 100 * 8
    assert lib.vk_layernorm_grad_workspace_bytes(7, 100) == 2 * 7 * 8
    assert lib.vk_layernorm_grad_workspace_bytes(300, 100) == 2 * 300 * 8 + 2 * 2 * 100 * 8


def test_launches_refuse_bad_arguments_before_the_device(lib):
    """Every check below fails before a launch, so no device is needed."""
    with pytest.raises(ValueError, match="activation"):
        L.call("vk_act_f32", 8, 8, 4, L.VK_ACT_RELU, None)
    with pytest.raises(ValueError, match="activation"):
        L.call("vk_act_grad_f32", 8, 8, 8, 4, 7, None)
    with pytest.raises(ValueError, match="ignore_index"):
        L.call("vk_cross_entropy_grad", 8, 4, 1, 4, 8, 0, 1.0, 8, 4, None)
    with pytest.raises(ValueError, match="workspace"):
        L.call("vk_col_sums", 8, 4, 300, 4, 8, None, 0, None)
    with pytest.raises(ValueError, match="betas"):
        L.call("vk_adamw_step", 8, 1, 1, 1e-3, 1.0, 0.999, 1e-8, 0.01, 0.1, 0.1, None)


def test_trainer_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a GPU: there is no CPU fallback"):
        T.HeadTrainer(object())


def test_torch_restatement_clears_the_loss_cap():
    """The fixture of test_gpu_head_train.py::test_loss_falls on the CPU: the yardstick itself reaches the cap the GPU test sets."""
    keys, sd, feats, labels = U.head_fixture()
    losses, _, _ = U.torch_run(sd, keys, feats, labels, 60, torch.float32)
    assert losses[-1] <= 0.5 * losses[0], losses[[0, -1]]
