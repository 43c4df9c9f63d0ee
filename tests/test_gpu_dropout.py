"""GPU (-m gpu): dropout in fine-tuning.  The mask is csrc/philox.h's pure function, restated in numpy in tests/dropout_util.py (pinned
here to Random123's known answers): `vk_dropout_add_f32` bit for bit, `vk_attention_tiled_dropout` and `vk_attention_grad_16_dropout`
against the float64 reference under the numpy mask (test_gpu_mixed_kernels.py's relative rule at its floor; exact on integer data at
p = 0.5, where rs = 2), and `EncoderTrainer(hidden_dropout=, attention_dropout=, seed=)` against the mask-taking yardstick."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                           # noqa: E402

import dropout_util as D                                                                 # noqa: E402
import finetune_util as U                                                                # noqa: E402
import mixed_util as X                                                                   # noqa: E402
import test_gpu_finetune as TF                                                           # noqa: E402
import test_gpu_mixed_finetune as TM                                                     # noqa: E402
from test_gpu_mixed_kernels import MASKED, VK, exact_data, same_bits                     # noqa: E402

SEED, STREAM = 0x9E3779B97F4A7C15, (5 << 16) + 3


def test_philox_known_answers():
    for ctr, key, want in D.KAT:
        got = D.philox(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, [ctr[0] | ctr[1] << 32])
        assert tuple(int(w) for w in got[0]) == want


# ---- vk_dropout_add_f32 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 255 / 256])
@pytest.mark.parametrize("form", ["plain", "residual", "in_place", "offset"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_dropout_add_bits(n, form, p):
    r = np.random.Generator(np.random.PCG64([n, 11]))
    o = int(form == "offset")                                         # the call's element 0 is 4 bytes past a 16-byte boundary
    x, res = (r.standard_normal(n + 1).astype(np.float32) for _ in range(2))
    xd, rd, od = (torch.from_numpy(a).cuda() for a in (x, res, np.full(n + 1, 7.0, np.float32)))
    with_res, out = form in ("residual", "offset"), xd if form == "in_place" else od

    def run(stream):
        xd.copy_(torch.from_numpy(x))
        L.call("vk_dropout_add_f32", xd.data_ptr() + 4 * o, rd.data_ptr() + 4 * o if with_res else None, out.data_ptr() + 4 * o, n, p, SEED, stream, None)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = run(STREAM)
    want = D.dropout_add(x[o:o + n], res[o:o + n] if with_res else None, p, SEED, STREAM)
    assert got[o:o + n].tobytes() == want.tobytes(), np.flatnonzero(got[o:o + n] != want)[:8]
    if p == 0 and not with_res:
        assert got[:n].tobytes() == x[:n].tobytes()
    assert run(STREAM).tobytes() == got.tobytes()
    if n >= 15 and 0 < p < 0.9:
        assert run(STREAM + 1).tobytes() != got.tobytes()              # another stream, another mask


# ---- the attention pair -------------------------------------------------------------------------------------------------------------------
def run_pair(q, k, v, mask, dout, heads, dtype, p, entry="_dropout"):
    """-> dict(o, dq, dk, dv) float64 [B, L, H]: the forward, then the backward on the forward's own O."""
    B, Lq, H = q.shape
    Lk, d = k.shape[1], H // heads
    dev = [torch.from_numpy(np.ascontiguousarray(a.reshape(-1, H))).to(dtype).cuda() for a in (q, k, v, dout)]
    mk = torch.from_numpy(np.asarray(mask, np.float32)).cuda()
    o = torch.empty((B * Lq, H), dtype=dtype, device="cuda")
    g = [torch.full((B * n, H), 7.0, dtype=torch.float32, device="cuda") for n in (Lq, Lk, Lk)]
    drop = (p, SEED, STREAM) if entry else ()
    L.call("vk_attention_tiled" + entry, dev[0].data_ptr(), H, dev[1].data_ptr(), H, dev[2].data_ptr(), H, mk.data_ptr(), o.data_ptr(), H, B, heads,
           Lq, Lk, d, VK[dtype], None, *drop)
    need = L.load().vk_attention_grad_16_dropout_workspace_bytes(B, heads, Lq)
    ws = torch.empty((need // 4,), dtype=torch.float32, device="cuda")
    call = [dev[0].data_ptr(), H, dev[1].data_ptr(), H, dev[2].data_ptr(), H, mk.data_ptr(), o.data_ptr(), H, dev[3].data_ptr(), H,
            g[0].data_ptr(), H, g[1].data_ptr(), H, g[2].data_ptr(), H, B, heads, Lq, Lk, d, VK[dtype], ws.data_ptr(), need]
    if entry:
        assert L.load().vk_attention_grad_16_dropout_check(*call, p) == L.VK_OK
    L.call("vk_attention_grad_16" + entry, *call, None, *drop)
    torch.cuda.synchronize()
    return dict(o=o.double().cpu().numpy().reshape(B, Lq, H), **{n: t.double().cpu().numpy().reshape(B, -1, H) for n, t in zip(("dq", "dk", "dv"), g)})


SHAPES = [(1, 1), (15, 15), (16, 17), (17, 16), (63, 65), (64, 64), (80, 80), (20, 36), (33, 130)]


@functools.lru_cache(maxsize=None)
def bound_case(dtype, Lq, Lk, d):
    r = np.random.Generator(np.random.PCG64([Lq, Lk, d]))
    q, k, v, dout = (X.round16(r.standard_normal((2, n, 2 * d)), dtype) for n in (Lq, Lk, Lk, Lq))
    mask = np.zeros((2, Lk))
    mask[0, r.choice(Lk, Lk // 3, replace=False)] = MASKED
    return q, k, v, mask, dout


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_attention_against_float64(dtype, d, shape, p):
    """B = 2, heads = 2, a key mask.  O within 4 eps of float64 (the pair test's rule of test_gpu_mixed_kernels.py); dQ, dK, dV on
    that O within 8 eps in the max norm: the floor of that file's relative rule, so never wider than it.  With one key P = 1 and
    dS = dP~ - D is zero but for the rounding of O: there dQ and dK are held to 8 eps of what each of the two terms can reach."""
    q, k, v, mask, dout = bound_case(dtype, *shape, d)
    keep, rs = D.keep_attention(2, 2, *shape, p, SEED, STREAM), D.rule(p)[1]
    got = run_pair(q, k, v, mask, dout, 2, dtype, p)
    ref = D.attention_reference(q, k, v, mask, dout, 2, dtype, keep, rs, o_given=got["o"])
    dist = {n: U.maxnorm_rel(got[n], ref[n]) / X.EPS16[dtype] for n in ("o", "dv") + (("dq", "dk") if shape[1] > 1 else ())}
    print(f"{dtype} d {d} {shape} p {p}: distance to float64 in eps: " + " ".join(f"{n} {x:.3f}" for n, x in dist.items()))
    assert dist.pop("o") <= 4 and all(x <= 8 for x in dist.values()), dist
    if shape[1] == 1:
        term = rs * d * np.abs(dout).max() * np.abs(v).max() / np.sqrt(d)
        assert np.abs(got["dq"]).max() <= 8 * X.EPS16[dtype] * term * np.abs(k).max() and np.abs(got["dk"]).max() <= 8 * X.EPS16[dtype] * term * np.abs(q).max()
    again = run_pair(q, k, v, mask, dout, 2, dtype, p)
    assert all(again[n].tobytes() == got[n].tobytes() for n in got)


# (kind of test_gpu_mixed_kernels.exact_data, B, heads, Lq, Lk, d, keys left): uniform P over a power-of-two count of keys
EXACT = [("b", 2, 2, 17, 16, 32, None), ("b", 1, 2, 80, 64, 64, None), ("a", 2, 2, 17, 64, 32, None), ("a", 1, 2, 33, 16, 64, None), ("d", 2, 2, 20, 36, 32, 16), ("d", 1, 1, 63, 130, 64, 64), ("d", 1, 2, 80, 80, 64, 32)]


@pytest.mark.parametrize("case", EXACT, ids=str)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_attention_exact(dtype, case):
    """p = 0.5, rs = 2: every P~, dS and O is a number of the type and every sum is exact, so one misplaced byte of the mask fails."""
    kind, B, heads, Lq, Lk, d, left = case
    q, k, v, mask, dout = exact_data(kind, B, heads, Lq, Lk, d, False, left)
    mask = np.zeros((B, Lk)) if mask is None else mask
    keep = D.keep_attention(B, heads, Lq, Lk, 0.5, SEED, STREAM)
    ref = D.attention_reference(q, k, v, mask, dout, heads, dtype, keep, 2.0, scale=U.launcher_scale(d))
    assert X.exact_in_16(ref, dtype, (q, k, v, dout)) and X.is16(ref["terms"]["p_undropped"], dtype), "the case's own data is not exact"
    assert not keep.all() and keep.any() and X.is16(ref["o"], dtype)
    got = run_pair(q, k, v, mask, dout, heads, dtype, 0.5)
    assert np.array_equal(got["o"], ref["o"]) and ref["o"].any() and ref["dk" if kind == "b" else "dq"].any()
    assert all(same_bits(got[n], ref[n]) for n in ("dq", "dk", "dv"))      # kind b: K = 0, an exact dK and a zero dQ; a, d: Q = 0, the reverse


@pytest.mark.parametrize("shape", [(16, 17), (33, 130)], ids=str)
def test_rate_zero_is_the_plain_entries(shape):
    q, k, v, mask, dout = bound_case(torch.bfloat16, *shape, 64)
    a, b = run_pair(q, k, v, mask, dout, 2, torch.bfloat16, 0.0), run_pair(q, k, v, mask, dout, 2, torch.bfloat16, 0.0, entry="")
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)


# ---- the trainer, on the wide fixture: two trained layers ------------------------------------------------------------------------------
RATES = dict(hidden_dropout=0.1, attention_dropout=0.1, seed=SEED)


@functools.lru_cache(maxsize=None)
def yardstick(mode, hidden, attention, max_norm):
    """-> (keys, the mode's yardstick with the masks, the pure-float64 run with the masks), 3 steps, shared."""
    runs = [D.trainer_run(2, 3, TM.boundary(2, TF.FX), m, hidden, attention, SEED, max_norm) for m in (mode, None)]
    return runs[0][0], runs[0][1], runs[1][1]


def test_trainer_mixed():
    """First-step gradients and a 3-step clipped trajectory under test_gpu_mixed_finetune.py's rule (cap 8 x, floor 2^-7); the same
    seed twice: the same bits; both rates 0.0: the trainer without the arguments."""
    tr = TM.trainer(2, **RATES)
    assert (tr.hidden_dropout, tr.attention_dropout) == (26 / 256, 26 / 256)
    TF.run_gpu(tr, 1)
    keys, yard, run64 = yardstick(TM.BF16, 0.1, 0.1, None)
    TM.hold_gradients("dropout n=2", keys, tr.grads(), yard, run64)
    a, b = TM.trainer(2, max_grad_norm=1.0, **RATES), TM.trainer(2, max_grad_norm=1.0, **RATES)
    la, lb = TF.run_gpu(a, 3), TF.run_gpu(b, 3)
    assert la.tobytes() == lb.tobytes()
    TM.same_bits(a, b)
    keys, yard, run64 = yardstick(TM.BF16, 0.1, 0.1, 1.0)
    TM.hold_trajectory("dropout n=2 clipped", keys, la, a.state_dict(), yard, run64, lambda s: TM.step_lr(*U.FIXTURE_STEP_LR)(U.FIXTURE_LR, s))
    a, b = TM.trainer(2, max_grad_norm=1.0), TM.trainer(2, max_grad_norm=1.0, hidden_dropout=0.0, attention_dropout=0.0, seed=5)
    assert TF.run_gpu(a, 2).tobytes() == TF.run_gpu(b, 2).tobytes()
    TM.same_bits(a, b)


def test_trainer_fp32_mode():
    """Hidden dropout in the fp32 mode against the pure-float64 run under test_gpu_finetune.py's rule (8 x torch's fp32 distance);
    attention dropout there, and rates outside [0, 1), are refused."""
    tr = TM.trainer(2, compute_dtype=None, hidden_dropout=0.1, seed=SEED)
    losses = TF.run_gpu(tr, 3)
    keys, run32, run64 = yardstick(torch.float32, 0.1, 0.0, None)
    TF.hold("fp32 hidden dropout n=2", keys, losses, tr.state_dict(), run32, run64)
    with pytest.raises(ValueError, match="compute_dtype=torch.bfloat16"):
        TM.trainer(2, compute_dtype=None, attention_dropout=0.1)
    for kw in (dict(hidden_dropout=1.0), dict(attention_dropout=-0.1), dict(hidden_dropout=float("nan"))):
        with pytest.raises(ValueError, match="dropout"):
            TM.trainer(2, **kw)
