"""CPU (-m "not gpu"): what the GPU tests of `EncoderTrainer` and `vk_attention_grad` stand on.  The float64 restatement of
tests/finetune_util.py reproduces transformers' own stored logits; the numpy attention-backward reference equals torch autograd;
the clip rule equals `clip_grad_norm_`; `vk_attention_grad_check` refuses what the launch refuses; and torch's own fp32 run on
the trajectory fixture clears every cap the GPU tests assert."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import finetune_util as U
from layoutlm_util import case_kwargs as llm_kwargs, golden_head
from visualbert_util import case_kwargs as vb_kwargs, golden_qa_state_dict
from vltk_amd import _lib as L


def _restate(sd, cfg, x0, mask01, kind, rows, enc_prefix):
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in sd.items()}
    layers = [f"{enc_prefix}encoder.layer.{i}" for i in range(cfg["num_hidden_layers"])]
    with torch.no_grad():
        return U.tail_logits(p, torch.tensor(np.asarray(x0, np.float64)), U.additive(mask01, torch.float64), layers,
                             cfg["num_attention_heads"], cfg["layer_norm_eps"], kind, rows, enc_prefix).numpy()


@pytest.mark.parametrize("geo", ["short", "long"])
def test_restatement_reproduces_visualbert_qa_logits(golden_dir, geo):
    """From the golden's `embedding_output` (the masked case, which the generator used for the QA head) to transformers' stored
    logits: measured 4.3e-7 (short) and 3.7e-7 (long) absolute on logits up to 2.3."""
    from vltk_amd.visualbert import visualbert_config
    g = np.load(os.path.join(golden_dir, "visualbert_small.npz"))
    cfg = visualbert_config(**{k[4:]: int(g[k]) for k in g.files if k.startswith("cfg/")})
    kw = vb_kwargs(g, geo, "masked")
    mask01 = np.concatenate((kw["attention_mask"], kw["visual_attention_mask"]), 1)
    rows = torch.as_tensor((kw["attention_mask"].sum(1) - 2).astype(np.int64))
    got = _restate(golden_qa_state_dict(g), cfg, g[f"{geo}/masked/embedding_output"], mask01, "cls", rows, "visual_bert.")
    err = np.abs(got - g[f"qa/{geo}/logits"]).max()
    print(f"visualbert {geo}: |restatement - transformers| = {err:.2e} on logits up to {np.abs(g[f'qa/{geo}/logits']).max():.2f}")
    assert err <= 2e-6


@pytest.mark.parametrize("geo,case", [("short", "plain"), ("short", "masked"), ("long", "masked")])
def test_restatement_reproduces_layoutlm_seq_logits(golden_dir, geo, case):
    """Measured 1.9e-7 .. 2.4e-7 absolute (printed)."""
    g = np.load(os.path.join(golden_dir, "layoutlm_small.npz"))
    cfg, n, sd = golden_head(g, "seq")
    mask01 = llm_kwargs(g, geo, case).get("attention_mask")
    got = _restate(sd, cfg, g[f"{geo}/{case}/embedding_output"], mask01, "classifier", None, "layoutlm.")
    err = np.abs(got - g[f"{geo}/{case}/seq_logits"]).max()
    print(f"layoutlm {geo}/{case}: |restatement - transformers| = {err:.2e} on logits up to {np.abs(g[f'{geo}/{case}/seq_logits']).max():.2f}")
    assert err <= 2e-6


@pytest.mark.parametrize("Lq,Lk,heads,d,masked", [(17, 35, 3, 8, True), (5, 70, 1, 24, False), (1, 3, 2, 4, True)])
def test_numpy_attention_backward_equals_autograd(Lq, Lk, heads, d, masked):
    r = np.random.Generator(np.random.PCG64([Lq, Lk, d]))
    q, dout = (r.standard_normal((2, Lq, heads * d)) for _ in range(2))
    k, v = (r.standard_normal((2, Lk, heads * d)) for _ in range(2))
    mask = None
    if masked:
        mask = np.zeros((2, Lk))
        mask[0, Lk // 2:] = U.FMIN
        mask[1, :] = U.FMIN                                # every key masked: the soft-max is uniform
    ref = U.attention_grad_reference(q, k, v, mask, dout, heads)
    for name, want in zip(("dq", "dk", "dv"), U.torch_attention_grads(q, k, v, mask, dout, heads, torch.float64)):
        assert U.maxnorm_rel(ref[name], want) <= 1e-12, name
        assert (ref["b_" + name] > 0).all() and np.isfinite(ref["b_" + name]).all()


def test_clip_rule_equals_clip_grad_norm():
    r = np.random.Generator(np.random.PCG64(5))
    for max_norm in (0.5, 1.0, 1e9):
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in ((7, 3), (5,), (1,))]
        gs = [r.standard_normal(p.shape) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g)
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        norm, coef = U.clip_rule(gs, max_norm)
        assert abs(norm - total) <= 1e-14 * total
        for p, g in zip(ps, gs):
            assert np.abs(p.grad.numpy() - g * coef).max() <= 1e-15 * np.abs(g).max()
        assert (coef == 1.0) == (max_norm == 1e9)


def test_attention_grad_check_refusals():
    """Host only: no pointer is read through, so made-up addresses stand in for device memory."""
    lib = L.load()
    B, heads, Lq, Lk, d = 2, 3, 5, 7, 8
    need = lib.vk_attention_grad_workspace_bytes(B, heads, Lq)
    assert need == 3 * B * heads * Lq * 4

    def check(ptrs=None, lds=None, mask=None, ws=4096, nbytes=need, **geo):
        g = dict(B=B, heads=heads, Lq=Lq, Lk=Lk, d=d)
        g.update(geo)
        ptrs = [4096] * 8 if ptrs is None else ptrs
        lds = [g["heads"] * g["d"]] * 8 if lds is None else lds
        a = [ptrs[0], lds[0], ptrs[1], lds[1], ptrs[2], lds[2], mask]
        for i in range(3, 8):
            a += [ptrs[i], lds[i]]
        return lib.vk_attention_grad_check(*a, g["B"], g["heads"], g["Lq"], g["Lk"], g["d"], ws, nbytes)

    assert check() == L.VK_OK and check(mask=4096) == L.VK_OK
    assert check(lds=[3 * heads * d] * 8) == L.VK_OK                      # a packed QKV projection
    assert check(d=128, lds=[3 * 128] * 8) == L.VK_OK and check(d=1, lds=[3] * 8) == L.VK_OK
    for bad in (0, 129, -1):
        assert check(d=bad, lds=[1024] * 8) == L.VK_EINVAL
        assert "head dim" in lib.vk_last_error().decode()
    for i in range(8):                                                    # every leading dimension, every pointer
        lds = [heads * d] * 8
        lds[i] -= 1
        assert check(lds=lds) == L.VK_EINVAL and "below heads * d" in lib.vk_last_error().decode()
        ptrs = [4096] * 8
        ptrs[i] = None
        assert check(ptrs=ptrs) == L.VK_EINVAL and "null" in lib.vk_last_error().decode()
    assert check(nbytes=need - 1) == L.VK_EINVAL and "workspace" in lib.vk_last_error().decode()
    assert check(ws=None) == L.VK_EINVAL
    for geo in (dict(B=0), dict(heads=0), dict(Lq=0), dict(Lk=0)):
        assert check(**geo) == L.VK_EINVAL
    assert lib.vk_attention_grad_workspace_bytes(0, 1, 1) == 0


@pytest.mark.parametrize("n", [1, 2])
def test_torch_clears_the_caps_of_the_gpu_tests(n):
    """Torch's own fp32 run on the trajectory fixture: the loss after 60 steps is at most half the first (measured 0.41 x for
    n = 1, 0.29 x for n = 2), and the step-1 gradient norm is above 1.0 (1.90, 1.92), so that `max_grad_norm = 1.0` engages."""
    cfg, sd, inputs, labels = U.trajectory_fixture()
    x0 = U.fixture_boundary_cpu(cfg, sd, inputs, cfg["num_hidden_layers"] - n)
    _, run = U.fixture_run(n, 60, torch.float32, x0)
    print(f"n={n}: loss {run['losses'][0]:.4f} -> {run['losses'][-1]:.4f} ({run['losses'][-1] / run['losses'][0]:.3f} x)")
    assert run["losses"][-1] <= 0.5 * run["losses"][0]
    _, clipped = U.fixture_run(n, 1, torch.float32, x0, max_norm=1.0)
    print(f"n={n}: step-1 gradient norm {clipped['norms'][0]:.3f}")
    assert clipped["norms"][0] > 1.0
    kb = [k for k in run["tensors"] if k.endswith("key.bias")]
    assert len(kb) == n
    for k in kb:                        # the key.bias gradient is rounding noise, far below AdamW's eps
        assert np.abs(run["first"][k]).max() < 1e-8, (k, np.abs(run["first"][k]).max())


def test_scatter_index_check():
    from vltk_amd.finetune import check_scatter_index
    assert check_scatter_index([3, 0, 5], 6).dtype == np.int32
    with pytest.raises(ValueError, match="distinct"):
        check_scatter_index([1, 1], 4)
    with pytest.raises(IndexError):
        check_scatter_index([4], 4)
