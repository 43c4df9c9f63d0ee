"""No GPU: the preconditions of every table of tests/extents_util.py, so that an exact GPU test can only fail for the kernel's
reasons: the GEMM sums stay below 2^24; the attention cases are exact in the 16-bit types (`exact_in_16`) and in fp32
(`exact_in_fp32`) with non-zero references where the GPU tests require them; the cross-entropy references agree with torch on rows
with infinite and NaN logits; the BASE fixture's yardstick runs are finite."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extents_util as E
import finetune_util as U
import mixed_util as X
import test_gpu_attention_grad as AG
import test_gpu_mixed_kernels as MK

DTYPES = [torch.bfloat16, torch.float16]


def test_gemm_tables_stay_exact_in_fp32():
    sizes = E.LONG_K + [E.LARGE_LONG_K] + [s for _, s, _ in E.TRAINER_CALLS]
    assert max(64 * K + 16 for _, _, K in sizes) == 64 * 4099 + 16 == 262352 < 2 ** 24
    for M, N, K in E.LONG_K:
        assert K % 16 and K % 32 and K % 64
        for one_hot in (False, True):
            a, b, bias, c0, want = E.gemm_case(M, N, K, 1, one_hot)
            assert E.gemm_sums_exact(a, b) and np.abs(want + bias + c0).max() < 2 ** 24
            assert (want == a.astype(np.int64) @ b.astype(np.int64)).all()                   # the BLAS product is the integer product
            for dtype in DTYPES:
                assert not one_hot or X.is16(want + bias, dtype)
    assert max(M for M, _ in E.COL_SUMS) * 8 < 2 ** 24


def test_gemm_tables_reach_both_tiles_on_the_devices_they_were_sized_for():
    """On 256 CUs (the GPU tests assert it from the device's own count)."""
    assert E.large_tile_rule(*E.LARGE_LONG_K[:2], 256) and not any(E.large_tile_rule(M, N, 256) for M, N, _ in E.LONG_K)
    assert {E.large_tile_rule(M, N, 256) for _, (M, N, _), _ in E.TRAINER_CALLS} == {False, True}


@pytest.mark.parametrize("kind,case", E.ATT16_EXACT, ids=str)
def test_attention_16_cases_are_exact(kind, case):
    q, k, v, mask, dout = MK.exact_data(kind, *case)
    for dtype in DTYPES:
        ref = X.attention_grad16_reference(q, k, v, mask, dout, case[1], dtype, scale=U.launcher_scale(case[4]))
        assert X.exact_in_16(ref, dtype, (q, k, v, dout))
        assert ref["dv"].any() and (kind != "d" or ref["dq"].any()) and (kind != "b" or ref["dk"].any())


@pytest.mark.parametrize("kind,case", E.ATT32_EXACT, ids=str)
def test_attention_fp32_cases_are_exact(kind, case):
    q, k, v, mask, dout = AG.exact_data(kind, *case)
    ref = U.attention_grad_reference(q, k, v, mask, dout, case[1], scale=U.launcher_scale(case[4]))
    assert U.exact_in_fp32(ref)
    assert ref["dv"].any() and (kind != "d" or ref["dq"].any()) and (kind != "b" or ref["dk"].any())


def test_a_uniform_p_over_512_keys_is_no_bf16_case():
    """Why the long key walks use the masked kinds."""
    case = (1, 1, 17, 512, 32, False)
    q, k, v, mask, dout = MK.exact_data("a", *case)
    ref = X.attention_grad16_reference(q, k, v, mask, dout, 1, torch.bfloat16, scale=U.launcher_scale(32))
    assert not X.exact_in_16(ref, torch.bfloat16, (q, k, v, dout))


@pytest.mark.parametrize("C,ld,form", E.CE_SHAPES, ids=str)
def test_cross_entropy_references_are_torchs(C, ld, form):
    for td in (torch.float32, torch.float16, torch.bfloat16):
        x, labels, kinds = E.ce_rows(C, td)
        assert kinds.count("finite") >= 3 and "label" in kinds and kinds.count("nan") == (6 if C >= 100 else 5)
        assert sum(bool(torch.isnan(r).any()) for r in x) == (3 if C >= 100 else 2)
        xt = x.double().requires_grad_(True)
        loss = F.cross_entropy(xt, torch.from_numpy(labels), reduction="none")
        loss.sum().backward()
        ref, bound = E.ce_loss_reference(x, labels, form, td)
        want = loss.detach().numpy()
        fin = np.isfinite(want)
        assert (np.isnan(ref) == np.isnan(want)).all() and (np.isposinf(ref) == np.isposinf(want)).all()
        assert [k == "finite" for k in kinds] == list(fin) and np.abs(ref[fin] - want[fin]).max() < 1e-12 and (bound[fin] > 0).all()
        if td == torch.float32:
            g, gb = E.ce_grad_reference(x.numpy(), labels, 1.0)
            tg = xt.grad.numpy()
            ok = ~np.isnan(tg)
            assert (np.isnan(g) == np.isnan(tg)).all() and np.abs(g[ok] - tg[ok]).max() < 1e-12
            assert (g[np.isneginf(x.numpy()) & ok & (g != -1.0)] == 0).all()


def test_base_fixture_yardsticks_are_finite():
    """One step of each yardstick of test_gpu_finetune_base.py from the CPU oracle's boundary state (the GPU tests take the
    model's own): 896 rows at hidden 768, finite losses and gradients, and the three runs agree on the loss to bf16's epsilon."""
    cfg, sd, inputs, labels = U.trajectory_fixture(base=True)
    assert (cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"], cfg["num_hidden_layers"]) == (768, 12, 3072, 2)
    x0 = U.fixture_boundary_cpu(cfg, sd, inputs, 1)
    assert x0.shape == (16, 56, 768) and np.isfinite(x0).all()
    assert not inputs["attention_mask"].all() and not inputs["visual_attention_mask"].all() and (labels == U.IGNORE_INDEX).sum() == 2
    keys, run32 = U.fixture_run(1, 1, torch.float32, x0, base=True)
    _, run64 = U.fixture_run(1, 1, torch.float64, x0, base=True)
    _, run16 = X.fixture_run(1, 1, x0, torch.bfloat16, base=True)
    for run in (run32, run64, run16):
        assert np.isfinite(run["losses"]).all() and all(np.isfinite(run["first"][k]).all() and run["first"][k].any() for k in keys
                                                        if not k.endswith("key.bias"))
        assert all(np.isfinite(v).all() for v in run["tensors"].values())
    assert abs(run32["losses"][0] - run64["losses"][0]) <= 1e-5 * run64["losses"][0]
    assert abs(run16["losses"][0] - run64["losses"][0]) <= 8 * X.EPS16[torch.bfloat16] * run64["losses"][0]
