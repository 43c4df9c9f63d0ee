"""CPU (-m "not gpu"): the host side of the mixed-precision fine-tuning mode.  `vk_gemm_16_check` and `vk_attention_grad_16_check`
refuse exactly what their contracts name (one case per rule; no pointer is read through, so the addresses are made up) and accept
the trainer's shapes; the workspace size is monotone; and the yardstick of the GPU tests (tests/mixed_util.py: the trained layers in
float64 with the mode's bf16 roundings) trains: its 60-step loss on the wide fixture falls below half the first, the cap the
trainer is held to."""
import numpy as np
import pytest
import torch

from vltk_amd import _lib as L

import finetune_util as U
import mixed_util as X

A, B_, C_ = 0x10000, 0x20000, 0x30000          # 16-byte aligned addresses, never read


@pytest.fixture(scope="module")
def lib():
    return L.load()


def gemm_args(**kw):
    a = dict(A=A, lda=128, transA=0, B=B_, ldb=128, transB=1, C=C_, ldc=384, M=256, N=384, K=128, dt=L.VK_BF16, out_dt=L.VK_BF16)
    a.update(kw)
    return tuple(a.values())


def test_gemm_16_check_accepts_the_trainers_calls(lib):
    """The wide fixture's QKV projection (hidden 128, 256 rows): Y = X W^T in bf16, dX = dY W and dW = dY^T X in fp32; and fp16."""
    assert lib.vk_gemm_16_check(*gemm_args()) == L.VK_OK
    assert lib.vk_gemm_16_check(*gemm_args(lda=384, ldb=128, transB=0, ldc=128, M=256, N=128, K=384, out_dt=L.VK_F32)) == L.VK_OK
    assert lib.vk_gemm_16_check(*gemm_args(lda=384, transA=1, ldb=128, transB=0, ldc=128, M=384, N=128, K=256, out_dt=L.VK_F32)) == L.VK_OK
    assert lib.vk_gemm_16_check(*gemm_args(dt=L.VK_F16, out_dt=L.VK_F16)) == L.VK_OK
    assert lib.vk_gemm_16_check(*gemm_args(M=1, N=1, K=1, lda=8, ldb=8, ldc=1, out_dt=L.VK_F32)) == L.VK_OK      # an fp32 C takes any ldc >= N


@pytest.mark.parametrize("change,text", [
    (dict(A=None), "null"), (dict(B=None), "null"), (dict(C=None), "null"),
    (dict(dt=L.VK_F32, out_dt=L.VK_F32), "f16 or bf16"), (dict(dt=L.VK_I32), "f16 or bf16"),
    (dict(out_dt=L.VK_F16), "out_dt"), (dict(out_dt=L.VK_I64), "out_dt"),
    (dict(M=0), "positive"), (dict(N=0), "positive"), (dict(K=-1), "positive"),
    (dict(transA=2), "0 or 1"), (dict(transB=-1), "0 or 1"),
    (dict(lda=120), "lda"), (dict(ldb=120), "ldb"), (dict(ldc=376), "ldc"),
    (dict(lda=132), "multiples of 8"), (dict(ldb=129), "multiples of 8"), (dict(ldc=388), "multiple of 8"),
    (dict(A=A + 8), "16-byte"), (dict(B=B_ + 2), "16-byte"), (dict(C=C_ + 4), "16-byte"),
    (dict(M=64 * 65535 + 1), "grid"),
], ids=str)
def test_gemm_16_check_refuses(lib, change, text):
    with pytest.raises(ValueError, match=text):
        L.call("vk_gemm_16_check", *gemm_args(**change))


def attn_args(**kw):
    """The wide fixture's backward: 16 sequences of 16 rows, 4 heads of d = 32, a packed [256, 384] projection, dense O and dO."""
    H = 128
    a = dict(q=A, ldq=3 * H, k=A + 2 * H, ldk=3 * H, v=A + 4 * H, ldv=3 * H, mask=None, o=B_, ldo=H, dout=C_, lddo=H, dq=0x40000, lddq=3 * H,
             dk=0x40000 + 4 * H, lddk=3 * H, dv=0x40000 + 8 * H, lddv=3 * H, B=16, heads=4, Lq=16, Lk=16, d=32, dt=L.VK_BF16, ws=0x50000,
             ws_bytes=3 * 16 * 4 * 16 * 4)
    a.update(kw)
    return tuple(a.values())


def test_attention_grad_16_check_accepts_the_trainers_calls(lib):
    assert lib.vk_attention_grad_16_workspace_bytes(16, 4, 16) == attn_args()[-1]
    assert lib.vk_attention_grad_16_check(*attn_args()) == L.VK_OK
    assert lib.vk_attention_grad_16_check(*attn_args(mask=0x60004)) == L.VK_OK                       # the mask is fp32: any 4-byte address
    assert lib.vk_attention_grad_16_check(*attn_args(dt=L.VK_F16)) == L.VK_OK
    # the long fixture: 2 sequences of 140 rows, 2 heads of d = 64; and a cross shape with matrices of their own
    assert lib.vk_attention_grad_16_check(*attn_args(B=2, heads=2, Lq=140, Lk=140, d=64, ws_bytes=3 * 2 * 2 * 140 * 4)) == L.VK_OK
    assert lib.vk_attention_grad_16_check(*attn_args(Lq=1, Lk=131, ldq=136, lddq=136)) == L.VK_OK


@pytest.mark.parametrize("change,text", [
    (dict(q=None), "null"), (dict(o=None), "null"), (dict(dout=None), "null"), (dict(dv=None), "null"),
    (dict(dt=L.VK_F32), "f16 or bf16"),
    (dict(B=0), "geometry"), (dict(heads=0), "geometry"), (dict(Lq=0), "geometry"), (dict(Lk=-3), "geometry"),
    (dict(d=16), "neither 32 nor 64"), (dict(d=128, heads=1), "neither 32 nor 64"),
    (dict(ldo=120), "of o is below"), (dict(lddv=120), "of dv is below"),
    (dict(ldq=388), "of q is no multiple of 8"), (dict(lddo=132), "of dout is no multiple of 8"), (dict(lddk=388), "of dk is no multiple of 8"),
    (dict(k=A + 2 * 128 + 8), "k is not 16-byte"), (dict(o=B_ + 2), "o is not 16-byte"), (dict(dq=0x40004), "dq is not 16-byte"),
    (dict(B=1 << 20, Lq=1 << 13, ws_bytes=1 << 62), "too many"),          # 2^20 * 4 heads * 2^9 query blocks = 2^31 items
    (dict(ws=None), "workspace"), (dict(ws_bytes=3 * 16 * 4 * 16 * 4 - 1), "workspace"), (dict(ws=0x50002), "4-byte"),
], ids=str)
def test_attention_grad_16_check_refuses(lib, change, text):
    with pytest.raises(ValueError, match=text):
        L.call("vk_attention_grad_16_check", *attn_args(**change))


def test_attention_grad_16_workspace_is_monotone(lib):
    f = lib.vk_attention_grad_16_workspace_bytes
    assert f(0, 1, 1) == f(1, 0, 1) == f(1, 1, 0) == 0
    sizes = (1, 2, 15, 16, 17, 140, 1024)
    for b in sizes:
        for h in (1, 3, 12):
            for lq in sizes:
                base = f(b, h, lq)
                assert base >= 12 * b * h * lq and base % 4 == 0
                assert f(b + 1, h, lq) >= base and f(b, h + 1, lq) >= base and f(b, h, lq + 1) >= base


def test_cast_16_refuses_on_the_host():
    with pytest.raises(ValueError, match="null"):
        L.call("vk_cast_16", None, A, 8, L.VK_BF16, None)
    with pytest.raises(ValueError, match="positive"):
        L.call("vk_cast_16", A, B_, 0, L.VK_BF16, None)
    with pytest.raises(ValueError, match="f16 or bf16"):
        L.call("vk_cast_16", A, B_, 8, L.VK_F32, None)


def test_trainer_refuses_a_dtype_before_it_asks_for_a_gpu():
    """The mode's own refusals are plain host checks (vltk_amd.finetune._check_compute_dtype)."""
    from vltk_amd.finetune import _check_compute_dtype
    ok = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4)
    assert _check_compute_dtype(None, dict(ok, hidden_size=32)) is None and _check_compute_dtype(torch.bfloat16, ok) is torch.bfloat16
    assert _check_compute_dtype(torch.bfloat16, dict(ok, num_attention_heads=2)) is torch.bfloat16
    with pytest.raises(ValueError, match="loss scaling"):
        _check_compute_dtype(torch.float16, ok)
    with pytest.raises(ValueError, match="torch.float64"):
        _check_compute_dtype(torch.float64, ok)
    with pytest.raises(ValueError, match="head dim is 8"):
        _check_compute_dtype(torch.bfloat16, dict(ok, hidden_size=32))
    with pytest.raises(ValueError, match="multiples of 8"):
        _check_compute_dtype(torch.bfloat16, dict(ok, intermediate_size=252))


def test_the_yardstick_trains():
    """60 steps of the bf16 yardstick on the wide fixture, one trained layer, from the CPU oracle's boundary state: the last loss
    is below half the first (the cap of the GPU test), and it stays near the pure-fp64 run."""
    cfg, sd, inputs, labels = U.trajectory_fixture(wide=True)
    x0 = U.fixture_boundary_cpu(cfg, sd, inputs, cfg["num_hidden_layers"] - 1)
    _, mixed = X.fixture_run(1, 60, x0, torch.bfloat16, wide=True)
    _, pure = X.fixture_run(1, 60, x0, None, wide=True)
    print(f"yardstick bf16: loss {mixed['losses'][0]:.4f} -> {mixed['losses'][-1]:.4f} ({mixed['losses'][-1] / mixed['losses'][0]:.3f} x); "
          f"fp64: {pure['losses'][0]:.4f} -> {pure['losses'][-1]:.4f}")
    assert mixed["losses"][-1] <= 0.5 * mixed["losses"][0]
    assert abs(mixed["losses"][0] - pure["losses"][0]) <= 8 * X.EPS16[torch.bfloat16] * pure["losses"][0]
    g, g64 = mixed["first"], pure["first"]
    for k in g:
        if not k.endswith("key.bias"):
            assert U.maxnorm_rel(g[k], g64[k]) <= 0.1, k                                  # a restatement of the same layer, 16-bit roundings apart


def test_rounding_helpers():
    for dtype in (torch.bfloat16, torch.float16):
        e = X.EPS16[dtype]
        assert e == torch.finfo(dtype).eps and X.U16[dtype] == e / 2
        assert X.round16(np.array([1 + e / 2, 1 + 3 * e / 2]), dtype).tolist() == [1.0, 1 + 2 * e]      # ties to even
        assert X.is16(np.array([1 + e, -3.0, 0.0]), dtype) and not X.is16(np.array([1 + e / 2]), dtype)
        b = X.bits16(np.array([1.0, -2.0]), dtype)
        assert X.from_bits16(b, dtype).tolist() == [1.0, -2.0]
