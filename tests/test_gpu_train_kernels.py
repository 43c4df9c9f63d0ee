"""GPU (-m gpu): the kernels of csrc/train.hip, one by one: the GEMM bit-exact on integer data in its transposition forms and both
tile sizes, and within the fmaf chain's bound on real data; the column sums exact on integers; the backward kernels and the
optimiser step against float64 under the bounds tests/train_util.py derives from their rounding points.  Every launch writes into
a buffer with poisoned padding and a guard behind it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L             # noqa: E402
from vltk_amd import train as T            # noqa: E402

import gpu_util as G                       # noqa: E402
import train_util as U                     # noqa: E402

POISON = 1e30
FORMS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}


def padded(a, extra, guard=0):
    """A host matrix on the device with `extra` poisoned columns per row (and `guard` poisoned elements behind the last row).
    -> (the flat buffer, the [rows, cols] view whose row stride is cols + extra)."""
    a = np.asarray(a, np.float32)
    rows, cols = a.shape
    ld = cols + extra
    buf = torch.full((rows * ld + guard,), POISON, dtype=torch.float32, device=G.DEV)
    view = buf[:rows * ld].view(rows, ld)[:, :cols]
    view.copy_(torch.from_numpy(a))
    return buf, view


def assert_padding_untouched(buf, rows, cols, ld, guard):
    host = buf.cpu().numpy()
    assert (host[:rows * ld].reshape(rows, ld)[:, cols:] == np.float32(POISON)).all(), "padding columns were written"
    assert (host[rows * ld:] == np.float32(POISON)).all() and len(host) == rows * ld + guard, "the guard was written"


def operands(r, M, N, K, ta, tb, integer):
    draw = (lambda *s: r.integers(-8, 9, s).astype(np.float32)) if integer else (lambda *s: r.standard_normal(s).astype(np.float32))
    return draw(*((K, M) if ta else (M, K))), draw(*((N, K) if tb else (K, N))), draw(N), draw(M, N)


def run_gemm(A, B, ta, tb, bias=None, C0=None):
    """-> C as numpy; padding and guard asserted."""
    _, a = padded(A, 3)
    _, b = padded(B, 2)
    M, N = (A.shape[1] if ta else A.shape[0]), (B.shape[0] if tb else B.shape[1])
    cbuf, c = padded(np.zeros((M, N), np.float32) if C0 is None else C0, 5, guard=1)
    if C0 is None:
        c.fill_(POISON)                        # without accumulate the old C is not read: poison proves it
    bt = None if bias is None else torch.from_numpy(bias).to(G.DEV)
    T.gemm_f32(a, b, bias=bt, out=c, trans_a=bool(ta), trans_b=bool(tb), accumulate=C0 is not None)
    torch.cuda.synchronize()
    assert_padding_untouched(cbuf, M, N, N + 5, 1)
    return c.cpu().numpy()


# ---- vk_gemm_f32 ---------------------------------------------------------------------------------------------------------------------
GEMM_EXACT = [(1, 1, 1), (33, 65, 3), (31, 130, 34), (130, 33, 65), (64, 259, 7)]           # the exact sizes (M, N, K); other files run them too
GEMM_EXACT_LARGE = (1400, 1500, 40)                                                         # the 128 x 128 tile


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("M,N,K", GEMM_EXACT)
def test_gemm_exact_on_integers(M, N, K, form):
    """Integers in [-8, 8]: every partial sum is an integer below 2^24, so the fmaf chain is exact and the result is numpy's integer
    product bit for bit: plain, with bias, and accumulated onto a non-zero C with bias."""
    ta, tb = FORMS[form]
    r = np.random.Generator(np.random.PCG64([M, N, K, ta, tb]))
    A, B, bias, C0 = operands(r, M, N, K, ta, tb, integer=True)
    ai = (A.T if ta else A).astype(np.int64)
    bi = (B.T if tb else B).astype(np.int64)
    want = ai @ bi
    assert np.abs(ai).__matmul__(np.abs(bi)).max() + 16 < 2 ** 24
    np.testing.assert_array_equal(run_gemm(A, B, ta, tb), want.astype(np.float32))
    np.testing.assert_array_equal(run_gemm(A, B, ta, tb, bias=bias), (want + bias.astype(np.int64)[None]).astype(np.float32))
    np.testing.assert_array_equal(run_gemm(A, B, ta, tb, bias=bias, C0=C0),
                                  (want + bias.astype(np.int64)[None] + C0.astype(np.int64)).astype(np.float32))


@pytest.mark.parametrize("form", ["NT", "NN", "TN"])
def test_gemm_exact_on_integers_large_tile(form):
    """A shape whose 128 x 128 tiles fill half the CUs and so runs the large-tile kernel, ragged in M, N and K (two K steps)."""
    M, N, K = GEMM_EXACT_LARGE
    assert 2 * (-(-M // 128)) * (-(-N // 128)) >= torch.cuda.get_device_properties(0).multi_processor_count
    ta, tb = FORMS[form]
    r = np.random.Generator(np.random.PCG64([7, ta, tb]))
    A, B, bias, C0 = operands(r, M, N, K, ta, tb, integer=True)
    want = (A.T if ta else A).astype(np.int64) @ (B.T if tb else B).astype(np.int64) + bias.astype(np.int64)[None] + C0.astype(np.int64)
    np.testing.assert_array_equal(run_gemm(A, B, ta, tb, bias=bias, C0=C0), want.astype(np.float32))


@pytest.mark.parametrize("form", list(FORMS))
def test_gemm_real_data_within_chain_bound(form):
    M, N, K = 130, 259, 200
    ta, tb = FORMS[form]
    r = np.random.Generator(np.random.PCG64([11, ta, tb]))
    A, B, _, _ = operands(r, M, N, K, ta, tb, integer=False)
    ref, mag = U.gemm_reference(A, B, ta, tb)
    got = run_gemm(A, B, ta, tb).astype(np.float64)
    ratio = (np.abs(got - ref) / (K * U.U32 * mag)).max()
    print(f"gemm {form}: worst |err| / (K u sum|ab|) = {ratio:.3e}")
    assert ratio <= 1.0


def test_gemm_refuses_bad_arguments():
    a = torch.zeros((4, 4), dtype=torch.float32, device=G.DEV)
    with pytest.raises(ValueError, match="ldc"):
        L.call("vk_gemm_f32", a.data_ptr(), 4, 0, a.data_ptr(), 4, 0, None, a.data_ptr(), 3, 4, 4, 4, 0, G.stream())
    with pytest.raises(ValueError, match="accumulate"):
        L.call("vk_gemm_f32", a.data_ptr(), 4, 0, a.data_ptr(), 4, 0, None, a.data_ptr(), 4, 4, 4, 4, 2, G.stream())


# ---- vk_col_sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 130])
@pytest.mark.parametrize("M", [1, 63, 65, 1000])
def test_col_sums_exact_on_integers(M, N):
    r = np.random.Generator(np.random.PCG64([M, N]))
    x = r.integers(-8, 9, (M, N)).astype(np.float32)
    _, xv = padded(x, 3)
    obuf = torch.full((N + 1,), POISON, dtype=torch.float32, device=G.DEV)
    T.col_sums(xv, out=obuf[:N])
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    np.testing.assert_array_equal(got[:N], x.astype(np.int64).sum(0).astype(np.float32))
    assert got[N] == np.float32(POISON)


# ---- vk_cross_entropy_grad ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(2, 2), (100, 104), (3129, 3131)])
def test_cross_entropy_grad(C, ld):
    r = np.random.Generator(np.random.PCG64([C]))
    kinds = [r.standard_normal(C) * 3, np.where(r.integers(0, 2, C) > 0, 90.0, -90.0) + r.standard_normal(C) * 0.01, np.full(C, 1.25),
             np.concatenate([[40.0], r.standard_normal(C - 1)])]
    rows, labels = [], []
    for x in kinds:
        for lab in (0, C - 1, -100):
            rows.append(x)
            labels.append(lab)
    x = np.array(rows, np.float32)
    labels = np.array(labels, np.int64)
    M = len(x)
    counted = int((labels != -100).sum())
    scale = np.float32(1.0 / counted)
    _, xv = padded(x, ld - C)
    obuf, ov = padded(np.zeros((M, C), np.float32), 1, guard=C + 1)          # a guard row behind the last
    ov.fill_(POISON)
    T.cross_entropy_grad(xv, torch.from_numpy(labels).to(G.DEV), scale, out=ov)
    torch.cuda.synchronize()
    assert_padding_untouched(obuf, M, C, C + 1, C + 1)
    got = ov.cpu().numpy().astype(np.float64)
    ref, bound = U.ce_grad_reference(x, labels, float(scale))
    assert (got[labels == -100] == 0).all()
    ratio = (np.abs(got - ref)[labels != -100] / bound[labels != -100]).max()
    print(f"ce_grad C={C}: worst |err| / bound = {ratio:.3e}")
    assert (np.abs(got - ref) <= bound).all()
    assert (np.abs(got.sum(1)) <= bound.sum(1)).all()


# ---- vk_act_f32 / vk_act_grad_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,code", [("gelu", L.VK_ACT_GELU), ("tanh", L.VK_ACT_TANH)])
def test_act_and_its_grad(act, code):
    r = np.random.Generator(np.random.PCG64(5))
    x = np.concatenate([np.linspace(-12, 12, 2049), [0.0, -0.0, 1e-30, -1e-30], r.uniform(-12, 12, 1000)]).astype(np.float32)
    assert (x == 0).sum() >= 2
    dy = r.standard_normal(len(x)).astype(np.float32)
    xt, dyt = torch.from_numpy(x).to(G.DEV), torch.from_numpy(dy).to(G.DEV)
    y = T.act_f32(xt, code).cpu().numpy().astype(np.float64)
    dx = T.act_grad_f32(xt, dyt, code).cpu().numpy().astype(np.float64)
    yref = U.act_reference(x, act)
    assert (np.abs(y - yref) <= U.U32 * np.abs(yref) + U.W64 * (np.abs(x) + 1) + 2.0 ** -149).all()
    ref, bound = U.act_grad_reference(x, dy, act)
    print(f"act_grad {act}: worst |err| / bound = {(np.abs(dx - ref) / bound).max():.3e}")
    assert (np.abs(dx - ref) <= bound).all()
    for name, args in (("vk_act_f32", (xt.data_ptr(), xt.data_ptr())), ("vk_act_grad_f32", (xt.data_ptr(), xt.data_ptr(), xt.data_ptr()))):
        with pytest.raises(ValueError, match="activation"):
            L.call(name, *args, 4, L.VK_ACT_RELU, G.stream())


# ---- vk_layernorm_grad ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 7, 300])
@pytest.mark.parametrize("C", [8, 100, 1536])
def test_layernorm_grad(M, C):
    """Against float64 autograd, eps = 1e-12; row 3 (where there is one) is constant: torch's backward gives
    (g - mean(g)) / sqrt(eps) there (train_util's docstring), and so does the kernel."""
    eps = 1e-12
    r = np.random.Generator(np.random.PCG64([M, C]))
    x = (r.standard_normal((M, C)) * 2 + 0.5).astype(np.float32)
    if M > 3:
        x[3] = np.float32(0.3)
    gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
    dy = r.standard_normal((M, C)).astype(np.float32)
    _, xv = padded(x, 3)
    _, dyv = padded(dy, 1)
    gt = torch.from_numpy(gamma).to(G.DEV)
    runs = []
    for _ in range(2):
        dx, dg, db = T.layernorm_grad(xv, gt, dyv, eps)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (dx, dg, db)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "two runs differ"
    ref = U.layernorm_grad_reference(x, gamma, dy, eps)
    for name, got in zip(("dx", "dgamma", "dbeta"), runs[0]):
        err = np.abs(got.astype(np.float64) - ref[name])
        print(f"layernorm_grad M={M} C={C} {name}: worst |err| / bound = {(err / ref['b_' + name]).max():.3e}")
        assert (err <= ref["b_" + name]).all(), name
    if M > 3:
        g = dy[3].astype(np.float64) * gamma
        want = (g - g.mean()) / np.sqrt(eps)
        assert np.abs(runs[0][0][3] - want).max() <= 2 * U.U32 * np.abs(want).max()


# ---- vk_adamw_step ---------------------------------------------------------------------------------------------------------------------
def test_adamw_step():
    """Tensors of 1, 7, 1536 and 1536 * 8 + 3 elements in one buffer per kind with a guard element between neighbours (so their
    starts are not 16-byte aligned), mixed decay flags, three steps, one gradient exactly zero; p, m, v against the float64 rule
    taken from the same fp32 inputs each step."""
    sizes, decay = [1, 7, 1536, 1536 * 8 + 3], [True, False, False, True]
    offs = np.cumsum([1] + [n + 1 for n in sizes])[:-1]               # a guard in front of each tensor, one behind the last
    total = int(offs[-1] + sizes[-1] + 1)
    assert any(int(o) % 4 for o in offs)
    r = np.random.Generator(np.random.PCG64(9))
    hp = {k: np.full(total, POISON, np.float32) for k in "pgmv"}
    for o, n in zip(offs, sizes):
        hp["p"][o:o + n] = r.standard_normal(n)
        hp["m"][o:o + n] = 0
        hp["v"][o:o + n] = 0
    bufs = {k: torch.from_numpy(v.copy()).to(G.DEV) for k, v in hp.items()}
    table, max_n = T.adamw_table([tuple(bufs[k][o:o + n] for k in "pgmv") + (d,) for o, n, d in zip(offs, sizes, decay)], G.DEV)
    assert max_n == sizes[-1]
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 0.01
    guard = np.ones(total, bool)
    for o, n in zip(offs, sizes):
        guard[o:o + n] = False
    worst = 0.0
    for step in (1, 2, 3):
        g = np.full(total, POISON, np.float32)
        for i, (o, n) in enumerate(zip(offs, sizes)):
            g[o:o + n] = 0.0 if (step == 2 and i == 2) else r.standard_normal(n) * 10.0 ** r.integers(-4, 1)
        g[offs[3]:offs[3] + 5] = 0.0
        bufs["g"].copy_(torch.from_numpy(g))
        before = {k: bufs[k].cpu().numpy() for k in "pmv"}
        T.adamw_step(table, len(sizes), max_n, lr, betas, eps, wd, step, G.DEV)
        torch.cuda.synchronize()
        after = {k: bufs[k].cpu().numpy() for k in "pgmv"}
        for k in "pgmv":
            assert (after[k][guard] == np.float32(POISON)).all(), f"a guard of {k} was written"
        for o, n, d in zip(offs, sizes, decay):
            s = slice(o, o + n)
            p, m, v, upd = U.adamw_f64(before["p"][s], g[s], before["m"][s], before["v"][s], lr, *betas, eps, wd, step, decay=d)
            for k, ref, b in zip("pmv", (p, m, v), U.adamw_bounds(before["p"][s], p, m, v, upd)):
                err = np.abs(after[k][s].astype(np.float64) - ref)
                worst = max(worst, (err / b).max())
                assert (err <= b).all(), (step, n, k)
    print(f"adamw: worst |err| / bound = {worst:.3e}")
