"""GPU (-m gpu): `vk_attention_grad`, `vk_scatter_rows_f32` and `vk_grad_clip` (csrc/attention_grad.hip, csrc/train.hip) against
the float64 references of tests/finetune_util.py.

The attention backward owns Tq = Tk = 16 rows per workgroup and walks the other side 64 rows at a time, so the lengths come from
{1, 15, 16, 17, 35} and {63, 64, 65, 131}; leading dimensions are heads * d + 3 .. 7, the packed 3 * heads * d, and heads * d itself.  Exact cases (integers in [-4, 4], d a power of four so that scale is a power of two)
ask for the reference's bits (the sign of a zero aside: an exact 0 is +0 or -0 by the order of the sum); each asserts first
that its own data is exact in fp32 whatever the order (`exact_in_fp32`).  Bound cases hold every element under the bound derived
in finetune_util's docstring and every tensor within 8 x torch's own fp32 distance to float64.  Every matrix lies in a buffer
with poisoned padding columns (1e30 in the inputs) and a guard behind it; the outputs' padding and guards must come back
untouched.  Head dims 1 and 128 (AG_MAXD) run in exact cases of every kind and in bound cases, 96 in bound cases; at d = 128 the scale is
no power of two and dQ, dK are asked as the one rounding of S * scale.  The pair tests put the library's own fp32 forward
(vk_attention, vk_attention_tiled: the LDS and the streaming kernel) in front of the backward, where every other test passes
O = fp32(reference O)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                           # noqa: E402
from vltk_amd.finetune import scatter_rows_f32                                           # noqa: E402
from vltk_amd.train import adamw_table                                                   # noqa: E402

import finetune_util as U                                                                # noqa: E402

GUARD, POISON, SENT = 64, np.float32(1e30), np.float32(-7.5e29)
FLOOR = 2.0 ** -23


class Buf:
    """One [rows, ld] fp32 matrix buffer with a guard behind it; `cols` are the columns that count, the rest is padding."""

    def __init__(self, rows, ld, fill):
        self.rows, self.ld = rows, ld
        self.host = np.full(rows * ld + GUARD, fill, np.float32)

    def put(self, a, col0):
        a = np.asarray(a, np.float32).reshape(self.rows, -1)
        self.host[:self.rows * self.ld].reshape(self.rows, self.ld)[:, col0:col0 + a.shape[1]] = a

    def upload(self):
        self.dev = torch.from_numpy(self.host).cuda()
        return self

    def ptr(self, col0=0):
        return self.dev.data_ptr() + 4 * col0

    def fetch(self, written):
        """-> the buffer after the call; asserts that nothing outside the column ranges `written` changed."""
        got = self.dev.cpu().numpy()
        keep = np.ones(got.shape, bool)
        body = keep[:self.rows * self.ld].reshape(self.rows, self.ld)
        for c0, c1 in written:
            body[:, c0:c1] = False
        assert (got[keep].view(np.uint32) == self.host[keep].view(np.uint32)).all(), "padding or guard overwritten"
        return got[:self.rows * self.ld].reshape(self.rows, self.ld)


def run_attention_grad(q, k, v, mask, o, dout, heads, packed=False, pad=3, dense=False):
    """-> (dq, dk, dv) as [B, L, H] fp32 numpy.  packed: q | k | v are the column blocks of one [B * L, 3H] buffer (leading
    dimension 3H), and so are the outputs; else each matrix has a leading dimension of H + pad (+ 0 .. 4) of its own.  dense:
    every matrix that is not packed has the leading dimension H = heads * d exactly (with packed: the trainer's layout, a
    packed projection beside dense O and dO); only the guards behind the buffers remain."""
    B, Lq, H = q.shape
    pad = -100 if dense else pad

    def ld(extra):
        return H + max(pad + extra, 0)
    Lk, d = k.shape[1], H // heads
    if packed:
        assert Lq == Lk
        qkv = Buf(B * Lq, 3 * H, POISON)
        for i, a in enumerate((q, k, v)):
            qkv.put(a, i * H)
        qkv.upload()
        ins = [(qkv, 0), (qkv, H), (qkv, 2 * H)]
        dqkv = Buf(B * Lq, 3 * H, SENT).upload()
        outs = [(dqkv, 0), (dqkv, H), (dqkv, 2 * H)]
    else:
        ins = []
        for a, extra in ((q, 0), (k, 1), (v, 2)):
            b = Buf(a.shape[0] * a.shape[1], ld(extra), POISON)
            b.put(a, 0)
            ins.append((b.upload(), 0))
        outs = [(Buf(B * L_, ld(extra), SENT).upload(), 0) for L_, extra in ((Lq, 1), (Lk, 0), (Lk, 4))]
    ob, dob = Buf(B * Lq, ld(0), POISON), Buf(B * Lq, ld(2), POISON)
    ob.put(o, 0)
    dob.put(dout, 0)
    ob.upload(), dob.upload()
    need = L.load().vk_attention_grad_workspace_bytes(B, heads, Lq)
    ws = Buf(1, need // 4, SENT).upload()
    mk = None if mask is None else torch.from_numpy(np.asarray(mask, np.float32)).cuda().contiguous()
    args = []
    for b, c in ins:
        args += [b.ptr(c), b.ld]
    args += [None if mk is None else mk.data_ptr(), ob.ptr(), ob.ld, dob.ptr(), dob.ld]
    for b, c in outs:
        args += [b.ptr(c), b.ld]
    L.call("vk_attention_grad", *args, B, heads, Lq, Lk, d, ws.ptr(), need, None)
    torch.cuda.synchronize()
    ws.fetch([(0, need // 4)])
    if packed:
        full = outs[0][0].fetch([(0, 3 * H)])
        res = [full[:, i * H:(i + 1) * H] for i in range(3)]
    else:
        res = [b.fetch([(0, H)])[:, :H] for b, _ in outs]
    return tuple(r.reshape(B, -1, H).copy() for r in res)


def ints(r, *shape):
    return r.integers(-4, 5, shape).astype(np.float64)


def keep_mask(r, B, Lk, count):
    """An additive mask [B, Lk] that leaves `count` scattered keys per batch item."""
    m = np.full((B, Lk), U.FMIN)
    for b in range(B):
        m[b, r.choice(Lk, count, replace=False)] = 0.0
    return m


# (B, heads, Lq, Lk, d, packed[, keys left])
CASE_A = [(1, 1, 1, 1, 4, False), (2, 3, 15, 16, 16, False), (1, 3, 17, 64, 64, False), (2, 1, 35, 128, 16, False),
          (1, 1, 131, 16, 4, False), (1, 3, 16, 16, 16, True), (2, 1, 64, 64, 4, True), (1, 1, 65, 128, 64, False)]
CASE_B = [(2, 3, 17, 16, 16, False), (1, 1, 131, 64, 4, False), (1, 3, 64, 64, 64, True), (2, 1, 63, 1, 16, False)]
CASE_C = [(2, 3, 17, 35, 16, False), (1, 1, 1, 131, 4, False), (2, 1, 65, 17, 64, False), (1, 3, 15, 15, 16, True),
          (2, 1, 131, 131, 4, True)]
CASE_D = [(2, 3, 16, 17, 16, False, 8), (1, 1, 35, 35, 4, False, 32), (1, 3, 1, 63, 16, False, 32), (2, 1, 17, 65, 64, False, 64),
          (1, 1, 15, 131, 16, False, 128), (1, 3, 35, 35, 16, True, 16), (2, 1, 131, 131, 4, True, 64)]


def exact_data(kind, B, heads, Lq, Lk, d, packed, left=None):
    """-> (q, k, v, mask, dout) of an exact case, float64."""
    r = np.random.Generator(np.random.PCG64([ord(kind), B, heads, Lq, Lk, d]))
    H = heads * d
    q, k, v, dout = ints(r, B, Lq, H), ints(r, B, Lk, H), ints(r, B, Lk, H), ints(r, B, Lq, H)
    mask = None
    if kind in "ad":
        q[:] = 0
    if kind == "b":
        k[:] = 0
    if kind == "c":
        mask = keep_mask(r, B, Lk, 1)
    if kind == "d":
        mask = keep_mask(r, B, Lk, left)
    return q, k, v, mask, dout


def exact_case(kind, B, heads, Lq, Lk, d, packed, left=None, dense=False):
    q, k, v, mask, dout = exact_data(kind, B, heads, Lq, Lk, d, packed, left)
    ref = U.attention_grad_reference(q, k, v, mask, dout, heads, scale=U.launcher_scale(d))      # d a power of four: 1 / sqrt(d) itself
    assert U.exact_in_fp32(ref), "the case's own data is not exact in fp32"
    got = run_attention_grad(*(t.astype(np.float32) for t in (q, k, v)), mask, ref["o"].astype(np.float32), dout.astype(np.float32), heads, packed, dense=dense)
    return ref, dict(zip(("dq", "dk", "dv"), got))


def same_bits(got, ref, rounded=False):
    """Equal values everywhere and equal bits wherever the reference is not zero.  `rounded`: the reference is an exact float64
    product with a scale that is no power of two, and its one rounding to fp32 is what is asked (else it is an fp32 number)."""
    want = ref.astype(np.float32)
    assert rounded or (want.astype(np.float64) == ref).all()
    nz = want != 0
    return np.array_equal(got, want) and (got[nz].view(np.uint32) == want[nz].view(np.uint32)).all()


@pytest.mark.parametrize("case", CASE_A, ids=str)
def test_exact_uniform(case):
    """Q = 0, no mask, Lk a power of two: P is exactly 1 / Lk.  Exact dV and dQ; dK exactly 0."""
    ref, got = exact_case("a", *case)
    assert same_bits(got["dv"], ref["dv"]) and same_bits(got["dq"], ref["dq"])
    assert not got["dk"].any() and not ref["dk"].any()


@pytest.mark.parametrize("case", CASE_B, ids=str)
def test_exact_zero_keys(case):
    """K = 0, Q integers: exact dK (and dV); dQ exactly 0."""
    ref, got = exact_case("b", *case)
    assert same_bits(got["dk"], ref["dk"]) and same_bits(got["dv"], ref["dv"])
    assert not got["dq"].any() and not ref["dq"].any()
    assert ref["dk"].any() or case[3] == 1


@pytest.mark.parametrize("case", CASE_C, ids=str)
def test_exact_one_hot(case):
    """A mask that leaves one key per batch item: P is one-hot.  Exact dV; dQ and dK exactly 0."""
    ref, got = exact_case("c", *case)
    assert same_bits(got["dv"], ref["dv"]) and ref["dv"].any()
    assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.parametrize("case", CASE_D, ids=str)
def test_exact_uniform_under_mask(case):
    """Case a under a mask that leaves a power-of-two count of scattered keys."""
    ref, got = exact_case("d", *case)
    assert same_bits(got["dv"], ref["dv"]) and same_bits(got["dq"], ref["dq"]) and ref["dq"].any()
    assert not got["dk"].any()


# the leading dimension heads * d itself: each kind once unpacked and once as the trainer lays it out (packed QKV, dense O and dO)
DENSE = [("a", (2, 3, 17, 64, 16, False)), ("a", (1, 3, 16, 16, 16, True)), ("b", (2, 1, 65, 16, 4, False)), ("b", (1, 3, 64, 64, 64, True)),
         ("c", (2, 3, 17, 35, 16, False)), ("c", (2, 1, 131, 131, 4, True)), ("d", (1, 1, 15, 131, 16, False, 128)), ("d", (1, 3, 35, 35, 16, True, 16))]


@pytest.mark.parametrize("kind,case", DENSE, ids=str)
def test_exact_dense_leading_dimensions(kind, case):
    """Leading dimensions equal to heads * d (and 3 * heads * d for the packed matrices): the same exact cases, no padding columns."""
    ref, got = exact_case(kind, *case, dense=True)
    for name in ("dq", "dk", "dv"):
        assert same_bits(got[name], ref[name]), name
    assert ref["dv"].any()


# ---- head dims 128 (AG_MAXD: every one of a thread's 8 accumulators live, 87 and 91 KiB of LDS in the dQ and dK/dV kernels) and 1 ------
# One case of each kind at each.  At d = 128 scale = fp32(1 / sqrt(128)) is no power of two: dV and the exact zeros as above; dQ and
# dK are asked as float32(S * float64(scale)) with S the exact sum (exact_in_fp32 is asserted of the data first, as everywhere):
# the kernel's last operation is that one product.
WIDE = [("a", (1, 2, 17, 64, 128, False)), ("b", (1, 1, 64, 64, 128, True)), ("c", (2, 1, 35, 70, 128, False)), ("d", (1, 2, 17, 65, 128, False, 32)),
        ("a", (2, 3, 17, 16, 1, False)), ("b", (1, 3, 16, 16, 1, True)), ("c", (1, 1, 35, 131, 1, False)), ("d", (2, 1, 65, 65, 1, True, 16))]


@pytest.mark.parametrize("kind,case", WIDE, ids=str)
def test_exact_head_dims_128_and_1(kind, case):
    ref, got = exact_case(kind, *case)
    assert case[4] in (1, 128) and np.float32(U.launcher_scale(case[4])) == np.float32(1.0) / np.sqrt(np.float32(case[4]))
    zero = {"a": ("dk",), "b": ("dq",), "c": ("dq", "dk"), "d": ("dk",)}[kind]
    assert same_bits(got["dv"], ref["dv"]) and ref["dv"].any()
    for name in ("dq", "dk"):
        if name in zero:
            assert not got[name].any() and not ref[name].any(), name
        else:
            assert same_bits(got[name], ref[name], rounded=True) and ref[name].any(), name


def test_backward_at_its_largest_head_dim_is_covered():
    """d = 128 = AG_MAXD runs in every exact kind and in bound cases that are padded, dense and packed."""
    assert {kind for kind, case in WIDE if case[4] == 128} == set("abcd")
    assert {case[4] for case in BOUND if case[3] == 128} == {False, True}


# ---- bound cases: (heads, Lq, Lk, d, packed); B = 3: a partial mask, every key masked, no key masked ---------------------------------
# d = 96 and 128: accumulator slots 5 .. 7, and more than 64 KiB of LDS in the dQ and dK/dV kernels; d = 1: one column.  A packed
# projection has as many queries as keys, so d = 96 runs (35, 70) with matrices of their own and (70, 70) packed.
BOUND = [(2, 35, 70, 8, False), (1, 17, 131, 24, False), (3, 65, 65, 64, True), (1, 20, 17, 80, False),
         (2, 17, 65, 128, False), (1, 35, 70, 96, False), (1, 70, 70, 96, True), (1, 33, 33, 128, True), (3, 20, 17, 1, False)]


@functools.lru_cache(maxsize=None)
def bound_case(heads, Lq, Lk, d, packed):
    r = np.random.Generator(np.random.PCG64([heads, Lq, Lk, d]))
    H = heads * d
    q, k, v, dout = (r.standard_normal((3, L_, H)).astype(np.float32) for L_ in (Lq, Lk, Lk, Lq))
    mask = np.zeros((3, Lk), np.float32)
    mask[0, r.choice(Lk, Lk // 3, replace=False)] = U.FMIN
    mask[1, :] = U.FMIN
    ref = U.attention_grad_reference(q, k, v, mask, dout, heads)
    g32 = U.torch_attention_grads(q, k, v, mask, dout, heads, torch.float32)
    return q, k, v, mask, dout, ref, dict(zip(("dq", "dk", "dv"), g32))


@pytest.mark.parametrize("case", BOUND, ids=str)
@pytest.mark.parametrize("dense", [False, True], ids=["padded", "dense"])
def test_bounds(case, dense):
    heads, packed = case[0], case[4]
    q, k, v, mask, dout, ref, g32 = bound_case(*case)
    got = dict(zip(("dq", "dk", "dv"), run_attention_grad(q, k, v, mask, ref["o"].astype(np.float32), dout, heads, packed, dense=dense)))
    for name in ("dq", "dk", "dv"):
        ratio = np.abs(got[name].astype(np.float64) - ref[name]) / ref["b_" + name]
        d_cpu, d_gpu = U.maxnorm_rel(g32[name], ref[name]), U.maxnorm_rel(got[name], ref[name])
        print(f"{case} dense={dense} {name}: worst error / bound {ratio.max():.3f}; d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, FLOOR):.2f}")
        assert ratio.max() <= 1.0, (name, ratio.max())
        assert d_gpu <= 8 * max(d_cpu, FLOOR), (name, d_cpu, d_gpu)


def test_same_input_same_bits():
    case = BOUND[2]
    q, k, v, mask, dout, ref, _ = bound_case(*case)
    runs = [run_attention_grad(q, k, v, mask, ref["o"].astype(np.float32), dout, case[0], case[4]) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


# ---- the pair: the library's own fp32 forward in front of the backward ------------------------------------------------------------------
# (heads, L, d, entry, route): q, k, v, the masks and dO of a packed bound case, in the trainer's layout (a packed projection
# [B * L, 3H], dense O and dO).  O comes from vk_attention / vk_attention_tiled, not from the reference: the LDS kernel forms
# P = e * (1 / l) as the backward does, the streaming kernel divides O by l where the backward multiplies by 1 / l.
PAIR = [(2, 35, 16, "vk_attention", "lds"), (2, 35, 16, "vk_attention_tiled", "stream"), (2, 140, 64, "vk_attention", "stream")]


@pytest.mark.parametrize("heads,Lx,d,entry,route", PAIR, ids=[f"{c[1]}-{c[2]}-{c[4]}" for c in PAIR])
def test_backward_of_the_librarys_own_forward(heads, Lx, d, entry, route):
    """O per element within transformer_check.attention_bound; dQ, dK, dV within the bounds with `o_given` = that O (the term
    |sum_c dO_c (O_given - O_ref)_c| of D is computed from it) and within 8 x torch's fp32 distance to float64."""
    import gpu_util as G
    import transformer_check as T
    from test_gpu_attention_long import attention
    q, k, v, mask, dout, _, g32 = bound_case(heads, Lx, Lx, d, True)
    B, H = 3, heads * d
    qkv = torch.from_numpy(np.concatenate((q, k, v), 2).reshape(B * Lx, 3 * H)).to(G.DEV)
    add = torch.from_numpy(mask)
    o = attention(entry, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], add.to(G.DEV), B, heads, Lx, Lx, d, L.VK_F32, route)
    t = [torch.from_numpy(a.reshape(B * Lx, H)) for a in (q, k, v)]
    r = T.attention_reference(*t, add, B, heads, Lx, Lx, d)
    T.assert_within(o, r["ref"], T.attention_bound(r, torch.float32, route), f"forward {entry} -> {route} L {Lx} d {d}")
    o = o.cpu().numpy().reshape(B, Lx, H)
    ref = U.attention_grad_reference(q, k, v, mask, dout, heads, o_given=o)
    got = dict(zip(("dq", "dk", "dv"), run_attention_grad(q, k, v, mask, o, dout, heads, packed=True, dense=True)))
    for name in ("dq", "dk", "dv"):
        ratio = np.abs(got[name].astype(np.float64) - ref[name]) / ref["b_" + name]
        d_cpu, d_gpu = U.maxnorm_rel(g32[name], ref[name]), U.maxnorm_rel(got[name], ref[name])
        print(f"pair {route} L {Lx} d {d} {name}: worst error / bound {ratio.max():.3f}; d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, FLOOR):.2f}")
        assert ratio.max() <= 1.0, (name, ratio.max())
        assert d_gpu <= 8 * max(d_cpu, FLOOR), (name, d_cpu, d_gpu)


# ---- the two small kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M,C", [(5, 19, 33), (16, 256, 32), (1, 1, 1)])
def test_scatter_rows(n, M, C):
    r = np.random.Generator(np.random.PCG64([n, M, C]))
    src = r.standard_normal((n, C)).astype(np.float32)
    idx = r.choice(M, n, replace=False).astype(np.int32)
    dst = Buf(M, C, SENT).upload()
    src_dev, idx_dev = torch.from_numpy(src).cuda(), torch.from_numpy(idx).cuda()
    L.call("vk_scatter_rows_f32", src_dev.data_ptr(), C, idx_dev.data_ptr(), n, dst.ptr(), C, M, C, None)
    torch.cuda.synchronize()
    got = dst.fetch([(0, C)])
    want = np.zeros((M, C), np.float32)
    want[idx] = src
    assert got.tobytes() == want.tobytes()
    again = scatter_rows_f32(src_dev, idx_dev, M)
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == want.tobytes()


def _clip(grads, max_norm):
    """-> (norm, coef, the gradients after the call) of vk_grad_clip over a table of these gradients."""
    g = [torch.from_numpy(a.copy()).cuda() for a in grads]
    table, max_n = adamw_table([(t, t, t, t, True) for t in g], g[0].device)
    nbytes = L.load().vk_grad_clip_workspace_bytes(len(g))
    work = Buf(1, nbytes // 4, SENT).upload()
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    L.call("vk_grad_clip", table.data_ptr(), len(g), max_n, float(max_norm), out.data_ptr(), work.ptr(), nbytes, None)
    torch.cuda.synchronize()
    work.fetch([(0, nbytes // 4)])
    norm, coef = (float(x) for x in out.cpu().numpy())
    return norm, coef, [t.cpu().numpy() for t in g]


def test_grad_clip():
    r = np.random.Generator(np.random.PCG64(11))
    grads = [r.standard_normal(n).astype(np.float32) * s for n, s in ((1, 1.0), (1000, 0.1), (70001, 0.01), (8192, 1e-3))]
    total = sum(g.size for g in grads)
    w = total * 2.0 ** -52                                   # the fp64 sums' own error, relative
    for max_norm in (1.0, 0.05):
        norm64, coef64 = U.clip_rule(grads, max_norm)
        norm, coef, got = _clip(grads, max_norm)
        print(f"max_norm {max_norm}: norm {norm:.6f} (fp64 {norm64:.6f}) coef {coef:.6f} (fp64 {coef64:.6f})")
        assert coef64 < 1.0
        assert abs(norm - norm64) <= (U.U32 + w) * norm64                  # one rounding of the fp64 norm
        assert abs(coef - coef64) <= (U.U32 + w) * coef64
        for a, b in zip(got, grads):                                       # coef's rounding and the product's
            want = b.astype(np.float64) * coef64
            assert (np.abs(a - want) <= np.abs(want) * (2 * U.U32 + w) * (1 + 2.0 ** -20) + 2.0 ** -149).all()
    norm, coef, got = _clip(grads, 1e9)
    assert coef == 1.0
    for a, b in zip(got, grads):
        assert a.tobytes() == b.tobytes()


def test_grad_clip_nonfinite_propagates():
    grads = [np.ones(10, np.float32), np.array([1.0, np.nan, 2.0], np.float32)]
    norm, coef, got = _clip(grads, 1.0)
    assert np.isnan(norm) and np.isnan(coef) and all(np.isnan(a).all() for a in got)
    grads[1][1] = np.inf
    norm, coef, got = _clip(grads, 1.0)
    assert np.isinf(norm) and coef == 0.0 and (got[0] == 0).all() and np.isnan(got[1][1])
