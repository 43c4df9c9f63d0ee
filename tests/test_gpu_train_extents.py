"""GPU (-m gpu): the training kernels at the extents the trainer runs them at, where tests/test_gpu_train_kernels.py,
test_gpu_mixed_kernels.py and test_gpu_attention_grad.py stop at tile edges and toy sizes.  The tables and their CPU halves are in
tests/extents_util.py; tests/test_train_extents_host.py asserts their exactness preconditions without a GPU.

GEMMs (`vk_gemm_f32`, `vk_gemm_16` in bf16 and fp16): whole-tensor equality with the float64 BLAS product of integers in [-8, 8]
at K = 4099 and 2051 (129 and 65 steps of the pipelined K loop, the last one partial at every step width) in every form, plain,
with bias and, in fp32, accumulated onto a non-zero C; on the 128 x 128 tile at K = 2051 in every form (`TT` included); and at
the nine (M, N, K) of a BERT-base layer's calls at 896 rows, where the launcher's rule (asserted from the CU count) picks both
tiles.  `vk_col_sums` at 17 slices and the two widths.

Attention backward (`vk_attention_grad`, `vk_attention_grad_16`) at 12 heads of d = 64: exact cases that walk 3 to 9 tiles of 64
(the masked kinds for the long key walks: a uniform P over more than 128 keys is no bf16 number), one bound case and one pair test
per kernel in the trainer's layout (a packed [B L, 2304] projection, dense O and dO)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import train as T                                                          # noqa: E402

import extents_util as E                                                                 # noqa: E402
import gpu_util as G                                                                     # noqa: E402
import mixed_util as X                                                                   # noqa: E402
import test_gpu_attention_grad as AG                                                     # noqa: E402
import test_gpu_mixed_kernels as MK                                                      # noqa: E402
import test_gpu_train_kernels as TK                                                      # noqa: E402

DTYPES = MK.DTYPES


def stored(op, trans):
    """op(A) or op(B) as the form stores it, fp32 and contiguous."""
    return np.ascontiguousarray((op.T if trans else op).astype(np.float32))


def gemm32(a, b, form, bias=None, C0=None):
    ta, tb = E.FORMS32[form]
    assert E.gemm_sums_exact(a, b)
    return TK.run_gemm(stored(a, ta), stored(b, tb), ta, tb, bias=None if bias is None else bias.astype(np.float32),
                       C0=None if C0 is None else C0.astype(np.float32))


def gemm16(a, b, bias, form, dtype, out16, pad=1):
    assert E.gemm_sums_exact(a, b)
    return MK.run_gemm16(np.array(a), np.array(b), bias, form, dtype, out16, pad)[0]                # copies: the case's arrays are read-only


# ---- A. GEMMs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(E.FORMS32))
@pytest.mark.parametrize("size", E.LONG_K, ids=str)
def test_gemm_f32_long_k(size, form):
    a, b, bias, c0, want = E.gemm_case(*size, 1)
    assert not MK.large_tile(size[0], size[1])
    np.testing.assert_array_equal(gemm32(a, b, form), want.astype(np.float32))
    np.testing.assert_array_equal(gemm32(a, b, form, bias=bias), (want + bias).astype(np.float32))
    np.testing.assert_array_equal(gemm32(a, b, form, bias=bias, C0=c0), (want + bias + c0).astype(np.float32))


@pytest.mark.parametrize("form", list(MK.FORMS))
@pytest.mark.parametrize("size", E.LONG_K, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_16_long_k(dtype, size, form):
    a, b, bias, _, want = E.gemm_case(*size, 1)
    assert np.array_equal(gemm16(a, b, None, form, dtype, False), want)
    assert np.array_equal(gemm16(a, b, bias, form, dtype, False), want + bias)
    a, b, bias, _, want = E.gemm_case(*size, 2, one_hot=True)
    assert X.is16(want + bias, dtype)
    assert np.array_equal(gemm16(a, b, bias, form, dtype, True), want + bias)


@pytest.mark.parametrize("form", list(E.FORMS32))
def test_gemm_f32_large_tile_long_k(form):
    M, N, K = E.LARGE_LONG_K
    assert MK.large_tile(M, N)
    a, b, bias, c0, want = E.gemm_case(M, N, K, 3)
    np.testing.assert_array_equal(gemm32(a, b, form, bias=bias, C0=c0), (want + bias + c0).astype(np.float32))


@pytest.mark.parametrize("form", list(MK.FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_16_large_tile_long_k(dtype, form):
    M, N, K = E.LARGE_LONG_K
    assert MK.large_tile(M, N)
    a, b, bias, _, want = E.gemm_case(M, N, K, 3)
    assert np.array_equal(gemm16(a, b, bias, form, dtype, False), want + bias)


def test_trainer_calls_cover_both_tiles():
    picks = {MK.large_tile(M, N) for _, (M, N, _), _ in E.TRAINER_CALLS}
    assert picks == {False, True}, picks


@pytest.mark.parametrize("form,size,use_bias", E.TRAINER_CALLS, ids=[f"{f}-{s}" for f, s, _ in E.TRAINER_CALLS])
def test_gemm_f32_trainer_calls(form, size, use_bias):
    """Dense leading dimensions, as the trainer's activations and weights have them."""
    ta, tb = E.FORMS32[form]
    M, N, K = size
    a, b, bias, _, want = E.gemm_case(M, N, K, 4)
    assert E.gemm_sums_exact(a, b)
    print(f"gemm_f32 {form} {size}: {'128 x 128' if MK.large_tile(M, N) else '64 x 64'} tile")
    A, B = (torch.from_numpy(stored(a, ta)).to(G.DEV), torch.from_numpy(stored(b, tb)).to(G.DEV))
    cbuf = torch.full((M * N + 64,), TK.POISON, dtype=torch.float32, device=G.DEV)
    T.gemm_f32(A, B, bias=torch.from_numpy(bias.astype(np.float32)).to(G.DEV) if use_bias else None, out=cbuf[:M * N].view(M, N),
               trans_a=bool(ta), trans_b=bool(tb), accumulate=False)
    torch.cuda.synchronize()
    host = cbuf.cpu().numpy()
    assert (host[M * N:] == np.float32(TK.POISON)).all(), "the guard was written"
    np.testing.assert_array_equal(host[:M * N].reshape(M, N), (want + (bias if use_bias else 0)).astype(np.float32))


@pytest.mark.parametrize("form,size,use_bias", E.TRAINER_CALLS, ids=[f"{f}-{s}" for f, s, _ in E.TRAINER_CALLS])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_16_trainer_calls(dtype, form, size, use_bias):
    """The QKV projection (NT, N = 2304) writes 16 bits, as the mode does; everything else fp32."""
    M, N, K = size
    out16 = form == "NT" and N == 2304
    a, b, bias, _, want = E.gemm_case(M, N, K, 5, one_hot=out16)
    want = want + (bias if use_bias else 0)
    assert not out16 or X.is16(want, dtype)
    assert np.array_equal(gemm16(a, b, bias if use_bias else None, form, dtype, out16, pad=0), want)


@pytest.mark.parametrize("M,N", E.COL_SUMS)
def test_col_sums_exact_at_17_slices(M, N):
    r = np.random.Generator(np.random.PCG64([M, N]))
    x = r.integers(-8, 9, (M, N)).astype(np.float32)
    assert 8 * M < 2 ** 24 and -(-M // 256) == 17
    _, xv = TK.padded(x, 3)
    obuf = torch.full((N + 1,), TK.POISON, dtype=torch.float32, device=G.DEV)
    T.col_sums(xv, out=obuf[:N])
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    np.testing.assert_array_equal(got[:N], x.astype(np.int64).sum(0).astype(np.float32))
    assert got[N] == np.float32(TK.POISON)


# ---- B. attention backward at 12 heads of d = 64 ---------------------------------------------------------------------------------------
def assert_exact(kind, ref, got, same_bits):
    """What the exact tests of the two kernels' own files ask of each kind."""
    assert same_bits(got["dv"], ref["dv"]) and ref["dv"].any()
    if kind in "ad":
        assert same_bits(got["dq"], ref["dq"]) and not got["dk"].any() and not ref["dk"].any()
        assert kind == "a" or ref["dq"].any()
    if kind == "b":
        assert same_bits(got["dk"], ref["dk"]) and ref["dk"].any() and not got["dq"].any() and not ref["dq"].any()
    if kind == "c":
        assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.parametrize("kind,case", E.ATT16_EXACT, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_grad_16_exact_at_12_heads(dtype, kind, case):
    """`exact_in_16` is asserted of the case's data in front of the launch (MK.exact_case)."""
    ref, got = MK.exact_case(kind, dtype, *case, dense=case[5])
    assert_exact(kind, ref, got, MK.same_bits)


@pytest.mark.parametrize("kind,case", E.ATT32_EXACT, ids=str)
def test_attention_grad_exact_at_12_heads(kind, case):
    """`exact_in_fp32` is asserted of the case's data in front of the launch (AG.exact_case)."""
    ref, got = AG.exact_case(kind, *case, dense=case[5])
    assert_exact(kind, ref, got, AG.same_bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_grad_16_bounds_at_12_heads(dtype):
    heads, packed = E.ATT_BOUND[0], E.ATT_BOUND[4]
    q, k, v, mask, dout, ref, g16 = MK.bound_case(dtype, *E.ATT_BOUND)
    got = dict(zip(("dq", "dk", "dv"), MK.run_attention_grad16(q, k, v, mask, ref["o_given"], dout, heads, dtype, packed, dense=True)))
    MK.held(f"{dtype} {E.ATT_BOUND} trainer layout", got, ref, g16, dtype)


def test_attention_grad_bounds_at_12_heads():
    AG.test_bounds(E.ATT_BOUND, True)


def test_attention_grad_16_of_the_tiled_forward_at_12_heads():
    """O from `vk_attention_tiled` in bf16; the route is asked of `vk_attention_route` in front of the launch."""
    heads, Lx, _, d, _ = E.ATT_BOUND
    MK.test_attention_backward_of_the_tiled_forward(heads, Lx, d)


def test_attention_grad_of_the_fp32_forward_at_12_heads():
    """O from `vk_attention` in fp32, which streams at this length: the route is asked of the dispatcher in front of the launch."""
    heads, Lx, _, d, _ = E.ATT_BOUND
    AG.test_backward_of_the_librarys_own_forward(heads, Lx, d, "vk_attention", "stream")
