"""GPU (-m gpu): the three kernels of the mixed-precision fine-tuning mode, `vk_cast_16`, `vk_gemm_16` (csrc/gemm16.hip) and
`vk_attention_grad_16` (csrc/attention_grad16.hip), in bf16 and fp16, against float64 references on the rounded inputs.

Every matrix lies in a buffer with poisoned padding columns (a large finite value of its type) and a guard behind it; the
outputs' padding and guards must come back untouched.  Leading dimensions of 16-bit matrices are multiples of 8.

`vk_gemm_16` runs 64 x 64 tiles where 128 x 128 tiles would fill less than half the CUs and 128 x 128 tiles elsewhere, K in steps of
64 made of two 32-wide slices and 8-element chunks: the exact cases take M, N, K from {1, 63, 64, 65, 127, 128, 129} in all three
forms, and M, N one below, at and one above a multiple of 128 at sizes where the large tile runs (asserted from the CU count).
Integer data in [-8, 8]: the products' sums stay below 2^24, so fp32 accumulation is exact in any order.

`vk_attention_grad_16` owns 16 rows per wave and walks the other side 64 at a time in two 32-row slices: lengths from
{1, 15, 16, 17, 63, 64, 65, 131}.  Its exact cases use data for which P, dS and the O it is given are numbers of the 16-bit type
(asserted first, `exact_in_16`): uniform P over a power-of-two count of keys, V in {-1, 0, 1} and one +-1 per (row, head) of dO, so
that dP - D is a multiple of 1 / Lk below 256 / Lk; under a one-hot mask any integers."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                           # noqa: E402

import finetune_util as U                                                                # noqa: E402
import mixed_util as X                                                                   # noqa: E402

GUARD = 64
DTYPES = [torch.bfloat16, torch.float16]
VK = {torch.bfloat16: L.VK_BF16, torch.float16: L.VK_F16}
POISON = {torch.bfloat16: 1e30, torch.float16: 6e4, torch.float32: 1e30}
SENT = {torch.bfloat16: -7.5e29, torch.float16: -5e4, torch.float32: -7.5e29}


class Buf:
    """One [rows, ld] matrix buffer of `dtype` (a torch dtype) with a guard behind it, filled with `fill`."""

    def __init__(self, rows, ld, dtype, fill):
        self.rows, self.ld, self.dtype = rows, ld, dtype
        self.host = torch.full((rows * ld + GUARD,), float(fill), dtype=dtype)

    def put(self, a, col0=0):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(self.rows, -1))).to(self.dtype)
        self.host[:self.rows * self.ld].view(self.rows, self.ld)[:, col0:col0 + a.shape[1]] = a
        return self

    def upload(self):
        self.dev = self.host.cuda()
        return self

    def ptr(self, col0=0):
        return self.dev.data_ptr() + self.host.element_size() * col0

    def _bits(self, t):
        return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()

    def fetch(self, written):
        """-> the body after the call as float64 [rows, ld] and its bits; asserts nothing outside the column ranges changed."""
        got = self.dev.cpu()
        keep = np.ones(got.shape, bool)
        body = keep[:self.rows * self.ld].reshape(self.rows, self.ld)
        for c0, c1 in written:
            body[:, c0:c1] = False
        assert (self._bits(got)[keep] == self._bits(self.host)[keep]).all(), "padding or guard overwritten"
        return got[:self.rows * self.ld].view(self.rows, self.ld).double().numpy(), self._bits(got)[:self.rows * self.ld].reshape(self.rows, self.ld)


def up8(n):
    return (n + 7) // 8 * 8


# ---- vk_cast_16 ---------------------------------------------------------------------------------------------------------------------------
def cast_pool(dtype):
    """fp32 values: zeros, infinities, NaN, ties of the target (to even both ways), its subnormals and their ties, overflow, and
    normals at several scales."""
    e = X.EPS16[dtype]
    sub = 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -24                       # the target's smallest subnormal
    big = 3.4e38 if dtype == torch.bfloat16 else 65520.0                                # rounds to Inf
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 1 + e / 2, 1 + 3 * e / 2, -(1 + e / 2), 1 + e / 2 + e / 2 ** 10, 1 + e / 2 - e / 2 ** 10,
               sub, -sub, 3 * sub, sub / 2, 3 * sub / 2, sub * 0.75, 5 * sub / 2, sub * 1000.5, big, -big, big / 2, 1e-30, 1e-7, 123456.7]
    r = np.random.Generator(np.random.PCG64(16))
    rnd = np.concatenate([r.standard_normal(2048) * s for s in (1.0, 1e-3, 1e3 if dtype == torch.float16 else 1e20, 2.0 ** -16)])
    return np.concatenate((np.array(special), rnd)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4097])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_cast_is_torchs_cpu_cast(dtype, n):
    pool = cast_pool(dtype)
    start = {1: 4, 7: 5, 8: 2}.get(n, 0)                                                 # n = 1 is the NaN; 7 the ties and subnormals; 8 the infinities
    x = np.resize(np.roll(pool, -start), n).astype(np.float32)
    if n >= 8:
        assert np.isnan(x).any() and np.isinf(x).any()
    want = torch.from_numpy(x).to(dtype)
    xd = torch.from_numpy(x).cuda()
    out = Buf(1, n, dtype, SENT[dtype]).upload()
    L.call("vk_cast_16", xd.data_ptr(), out.ptr(), n, VK[dtype], None)
    torch.cuda.synchronize()
    vals, bits = out.fetch([(0, n)])
    wbits = want.view(torch.int16).numpy()
    nan = np.isnan(want.double().numpy())
    assert (np.isnan(vals[0]) == nan).all(), "NaN must stay NaN, and nothing else may become one"
    assert (bits[0][~nan] == wbits[~nan]).all(), np.flatnonzero(bits[0][~nan] != wbits[~nan])[:8]


def test_cast_unaligned_pointers_take_the_element_path():
    """A source that is only 4-byte aligned and a destination that is only 2-byte aligned: the same bits."""
    r = np.random.Generator(np.random.PCG64(17))
    x = r.standard_normal(1001).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = Buf(1, 1008, torch.bfloat16, SENT[torch.bfloat16]).upload()
    L.call("vk_cast_16", xd.data_ptr() + 4, out.ptr(3), 1000, L.VK_BF16, None)
    torch.cuda.synchronize()
    _, bits = out.fetch([(3, 1003)])
    assert (bits[0][3:1003] == torch.from_numpy(x[1:]).to(torch.bfloat16).view(torch.int16).numpy()).all()


# ---- vk_gemm_16 ---------------------------------------------------------------------------------------------------------------------------
FORMS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0)}


def large_tile(M, N):
    """Whether the launcher picks the 128 x 128 tile (csrc/gemm16.hip: where such tiles fill at least half the CUs)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * (-(-M // 128)) * (-(-N // 128)) >= cus


def run_gemm16(a, b, bias, form, dtype, out16, pad=1):
    """a = op(A) [M, K] and b = op(B) [K, N] as float64 arrays of `dtype` numbers -> (C float64 [M, N], its bits).  The operands are
    stored as the form says (A as [K, M] where transA; B as [N, K] where transB) with leading dimensions of the width rounded up to 8
    plus 8 * pad poisoned columns; C has N + 3 columns of fp32 or up8(N) + 8 of `dtype`."""
    ta, tb = FORMS[form]
    M, K = a.shape
    N = b.shape[1]
    sa, sb = (a.T if ta else a), (b.T if tb else b)
    A = Buf(sa.shape[0], up8(sa.shape[1]) + 8 * pad, dtype, POISON[dtype]).put(sa).upload()
    B = Buf(sb.shape[0], up8(sb.shape[1]) + 8 * pad, dtype, POISON[dtype]).put(sb).upload()
    cdt = dtype if out16 else torch.float32
    C = Buf(M, up8(N) + 8 * pad if out16 else N + 3 * pad, cdt, SENT[cdt]).upload()
    bd = None if bias is None else torch.from_numpy(np.asarray(bias, np.float32)).cuda()
    call = (A.ptr(), A.ld, ta, B.ptr(), B.ld, tb, C.ptr(), C.ld, M, N, K, VK[dtype], VK[dtype] if out16 else L.VK_F32)
    assert L.load().vk_gemm_16_check(*call) == L.VK_OK
    L.call("vk_gemm_16", *call[:6], None if bd is None else bd.data_ptr(), *call[6:], None)
    torch.cuda.synchronize()
    vals, bits = C.fetch([(0, N)])
    return vals[:, :N], bits[:, :N]


def int_operands(M, N, K, seed, one_hot=False):
    """Integers in [-8, 8] (both extremes present where the size allows); one_hot: op(A) has one +-1 per row, so that C is a row
    of B plus the bias, a number of either 16-bit type."""
    r = np.random.Generator(np.random.PCG64([M, N, K, seed]))
    b = r.integers(-8, 9, (K, N)).astype(np.float64)
    if one_hot:
        a = np.zeros((M, K))
        a[np.arange(M), r.integers(0, K, M)] = r.choice([-1.0, 1.0], M)
    else:
        a = r.integers(-8, 9, (M, K)).astype(np.float64)
    return a, b, r.integers(-8, 9, N).astype(np.float64)


EDGES = [(1, 1, 1), (63, 65, 64), (64, 63, 65), (65, 64, 63), (127, 129, 128), (128, 127, 129), (129, 128, 127), (1, 129, 65), (65, 1, 129),
         (129, 65, 1), (8, 8, 33), (17, 9, 31)]
# sizes at which the 128 x 128 tile runs on a 256-CU device (9 x 15 tiles and more), one below, at and one above its edge
EDGES_LARGE = [(1151, 1921, 65), (1152, 1919, 127), (1153, 1920, 64)]


@pytest.mark.parametrize("size", EDGES + EDGES_LARGE, ids=str)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_exact_fp32_out(dtype, form, size):
    M, N, K = size
    assert large_tile(M, N) == (size in EDGES_LARGE)
    a, b, bias = int_operands(M, N, K, 1)
    use_bias = (M + N + K) % 2 == 0
    want = (a.astype(np.int64) @ b.astype(np.int64) if M * N * K < 1 << 22 else a @ b) + (bias.astype(np.int64) if use_bias else 0)
    assert np.abs(a).max() <= 8 and (np.abs(a) @ np.abs(b)).max() + 8 < 2 ** 24
    got, _ = run_gemm16(a, b, bias if use_bias else None, form, dtype, out16=False)
    assert np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("size", EDGES + EDGES_LARGE[:1], ids=str)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_exact_16bit_out(dtype, form, size):
    M, N, K = size
    a, b, bias = int_operands(M, N, K, 2, one_hot=True)
    want = a @ b + bias
    assert X.is16(want, dtype)                                                           # the result is representable: one rounding changes nothing
    got, _ = run_gemm16(a, b, bias, form, dtype, out16=True)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# the three GEMMs of the trainer's QKV projection on the wide fixture (hidden 128, 16 x 16 rows): Y = X W^T + b written in 16 bits,
# dX = dY W and dW = dY^T X in fp32, dense leading dimensions
@pytest.mark.parametrize("form,size,out16", [("NT", (256, 384, 128), True), ("NN", (256, 128, 384), False), ("TN", (384, 128, 256), False)])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_exact_trainer_calls(dtype, form, size, out16):
    M, N, K = size
    a, b, bias = int_operands(M, N, K, 3, one_hot=out16)
    bias = bias if form == "NT" else None
    want = a @ b + (bias if bias is not None else 0)
    assert (np.abs(a) @ np.abs(b)).max() + 8 < 2 ** 24 and (not out16 or X.is16(want, dtype))
    got, _ = run_gemm16(a, b, bias, form, dtype, out16, pad=0)
    assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def gemm_bound_case(dtype, M, N, K):
    r = np.random.Generator(np.random.PCG64([M, N, K]))
    a, b = X.round16(r.standard_normal((M, K)), dtype), X.round16(r.standard_normal((K, N)), dtype)
    bias = r.standard_normal(N).astype(np.float32).astype(np.float64)
    return a, b, bias, a @ b + bias, np.abs(a) @ np.abs(b) + np.abs(bias)


@pytest.mark.parametrize("out16", [False, True], ids=["f32out", "16out"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gemm_bounds(dtype, form, out16):
    """Standard-normal data rounded to the type against float64 on the rounded inputs: |C - ref| <= (K + 1) 2^-24 (|A| |B| + |bias|),
    the fp32 accumulation of K exact products and the bias in any order, plus one rounding of the result to the output type."""
    M, N, K = 129, 65, 200
    a, b, bias, ref, mag = gemm_bound_case(dtype, M, N, K)
    got, _ = run_gemm16(a, b, bias, form, dtype, out16)
    bound = (K + 1) * 2.0 ** -24 * mag + (X.U16[dtype] if out16 else 2.0 ** -24) * np.abs(ref) * (1 + 2.0 ** -10) + X.T16[dtype if out16 else torch.bfloat16]
    ratio = np.abs(got - ref) / bound
    print(f"gemm_16 {dtype} {form} {'16-bit' if out16 else 'fp32'} out: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
def test_gemm_same_input_same_bits(form):
    a, b, bias, _, _ = gemm_bound_case(torch.bfloat16, 129, 65, 200)
    runs = [run_gemm16(a, b, bias, form, torch.bfloat16, False)[1] for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()


# ---- vk_attention_grad_16 ---------------------------------------------------------------------------------------------------------------
def run_attention_grad16(q, k, v, mask, o, dout, heads, dtype, packed=False, dense=False):
    """-> (dq, dk, dv) as float64 [B, L, H].  The inputs are float64 arrays of `dtype` numbers.  packed: q | k | v are the column
    blocks of one [B * L, 3H] buffer, and so are the fp32 outputs; else each matrix has a leading dimension of H + 8, 16, ..  of
    its own.  dense: every matrix that is not packed has the leading dimension H (with packed: the trainer's layout)."""
    B, Lq, H = q.shape
    Lk, d = k.shape[1], H // heads
    f32 = torch.float32

    def ld(extra):
        return H if dense else H + 8 * (1 + extra)
    if packed:
        assert Lq == Lk
        qkv = Buf(B * Lq, 3 * H, dtype, POISON[dtype])
        for i, a in enumerate((q, k, v)):
            qkv.put(a, i * H)
        qkv.upload()
        ins = [(qkv, 0), (qkv, H), (qkv, 2 * H)]
        dqkv = Buf(B * Lq, 3 * H, f32, SENT[f32]).upload()
        outs = [(dqkv, 0), (dqkv, H), (dqkv, 2 * H)]
    else:
        ins = [(Buf(a.shape[0] * a.shape[1], ld(extra), dtype, POISON[dtype]).put(a).upload(), 0) for a, extra in ((q, 0), (k, 1), (v, 2))]
        outs = [(Buf(B * L_, ld(extra), f32, SENT[f32]).upload(), 0) for L_, extra in ((Lq, 1), (Lk, 0), (Lk, 3))]
    ob = Buf(B * Lq, ld(0), dtype, POISON[dtype]).put(o).upload()
    dob = Buf(B * Lq, ld(2), dtype, POISON[dtype]).put(dout).upload()
    need = L.load().vk_attention_grad_16_workspace_bytes(B, heads, Lq)
    ws = Buf(1, need // 4, f32, SENT[f32]).upload()
    mk = None if mask is None else torch.from_numpy(np.asarray(mask, np.float32)).cuda().contiguous()
    call = []
    for b, c in ins:
        call += [b.ptr(c), b.ld]
    call += [None if mk is None else mk.data_ptr(), ob.ptr(), ob.ld, dob.ptr(), dob.ld]
    for b, c in outs:
        call += [b.ptr(c), b.ld]
    call += [B, heads, Lq, Lk, d, VK[dtype], ws.ptr(), need]
    assert L.load().vk_attention_grad_16_check(*call) == L.VK_OK
    L.call("vk_attention_grad_16", *call, None)
    torch.cuda.synchronize()
    ws.fetch([(0, need // 4)])
    if packed:
        full, _ = outs[0][0].fetch([(0, 3 * H)])
        res = [full[:, i * H:(i + 1) * H] for i in range(3)]
    else:
        res = [b.fetch([(0, H)])[0][:, :H] for b, _ in outs]
    return tuple(r.reshape(B, -1, H).copy() for r in res)


def keep_mask(r, B, Lk, count, value=U.FMIN):
    """An additive mask [B, Lk] that leaves `count` scattered keys per batch item."""
    m = np.full((B, Lk), value)
    for b in range(B):
        m[b, r.choice(Lk, count, replace=False)] = 0.0
    return m


# (B, heads, Lq, Lk, d, packed[, keys left])
CASE_A = [(1, 1, 1, 1, 32, False), (2, 3, 15, 16, 32, False), (1, 3, 17, 64, 64, False), (1, 1, 131, 16, 32, False), (1, 3, 16, 16, 64, True),
          (2, 1, 64, 64, 32, True), (2, 1, 65, 64, 64, False), (1, 1, 63, 1, 32, False)]
CASE_B = [(2, 3, 17, 16, 32, False), (1, 1, 131, 64, 64, False), (1, 3, 64, 64, 64, True), (2, 1, 63, 1, 32, False)]
CASE_C = [(2, 3, 17, 63, 32, False), (1, 1, 1, 131, 64, False), (2, 1, 65, 17, 64, False), (1, 3, 15, 15, 32, True), (2, 1, 131, 131, 32, True)]
CASE_D = [(2, 3, 16, 17, 32, False, 8), (1, 1, 63, 65, 64, False, 32), (2, 1, 17, 65, 64, False, 64), (1, 1, 15, 131, 32, False, 128),
          (1, 3, 17, 17, 32, True, 16), (2, 1, 131, 131, 64, True, 64)]


def exact_data(kind, B, heads, Lq, Lk, d, packed, left=None):
    """-> (q, k, v, mask, dout, reference): see the module docstring for why P, dS and O are numbers of bf16 and fp16 alike."""
    r = np.random.Generator(np.random.PCG64([ord(kind), B, heads, Lq, Lk, d]))
    H = heads * d
    ints = lambda *shape: r.integers(-4, 5, shape).astype(np.float64)
    q, k = ints(B, Lq, H), ints(B, Lk, H)
    mask = None
    if kind == "c":
        v, dout, mask = ints(B, Lk, H), ints(B, Lq, H), keep_mask(r, B, Lk, 1)
    else:
        v = r.integers(-1, 2, (B, Lk, H)).astype(np.float64)
        dout = np.zeros((B, Lq, heads, d))
        hot = r.integers(0, d, (B, Lq, heads))
        np.put_along_axis(dout, hot[..., None], r.choice([-1.0, 1.0], (B, Lq, heads, 1)), -1)
        dout = dout.reshape(B, Lq, H)
        if kind in "ad":
            q[:] = 0
        if kind == "b":
            k[:] = 0
        if kind == "d":
            mask = keep_mask(r, B, Lk, left)
    return q, k, v, mask, dout


def exact_case(kind, dtype, B, heads, Lq, Lk, d, packed, left=None, dense=False):
    q, k, v, mask, dout = exact_data(kind, B, heads, Lq, Lk, d, packed, left)
    ref = X.attention_grad16_reference(q, k, v, mask, dout, heads, dtype, scale=U.launcher_scale(d))
    assert X.exact_in_16(ref, dtype, (q, k, v, dout)), "the case's own data is not exact in the 16-bit type"
    got = run_attention_grad16(q, k, v, mask, ref["o_given"], dout, heads, dtype, packed, dense)
    return ref, dict(zip(("dq", "dk", "dv"), got))


def same_bits(got, ref):
    """The reference is an exact sum (dV) or an exact sum times the fp32 scale (dQ, dK: exact in float64, one rounding in the
    kernel): equal values everywhere, and equal bits wherever the reference is not zero (an exact 0 is +0 or -0 by the order)."""
    want = ref.astype(np.float32)
    g = got.astype(np.float32)
    nz = want != 0
    return np.array_equal(g, want) and (g[nz].view(np.uint32) == want[nz].view(np.uint32)).all()


@pytest.mark.parametrize("case", CASE_A, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_exact_uniform(dtype, case):
    """Q = 0, no mask, Lk a power of two: P is exactly 1 / Lk.  Exact dV and dQ; dK exactly 0."""
    ref, got = exact_case("a", dtype, *case)
    assert same_bits(got["dv"], ref["dv"]) and same_bits(got["dq"], ref["dq"]) and ref["dv"].any()
    assert not got["dk"].any() and not ref["dk"].any()


@pytest.mark.parametrize("case", CASE_B, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_exact_zero_keys(dtype, case):
    """K = 0, Q integers: exact dK and dV; dQ exactly 0."""
    ref, got = exact_case("b", dtype, *case)
    assert same_bits(got["dk"], ref["dk"]) and same_bits(got["dv"], ref["dv"])
    assert not got["dq"].any() and not ref["dq"].any()
    assert ref["dk"].any() or case[3] == 1


@pytest.mark.parametrize("case", CASE_C, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_exact_one_hot(dtype, case):
    """A mask that leaves one key per batch item: P is one-hot.  Exact dV; dQ and dK exactly 0."""
    ref, got = exact_case("c", dtype, *case)
    assert same_bits(got["dv"], ref["dv"]) and ref["dv"].any()
    assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.parametrize("case", CASE_D, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_exact_uniform_under_mask(dtype, case):
    """Case a under a mask that leaves a power-of-two count of scattered keys."""
    ref, got = exact_case("d", dtype, *case)
    assert same_bits(got["dv"], ref["dv"]) and same_bits(got["dq"], ref["dq"]) and ref["dq"].any()
    assert not got["dk"].any()


# the leading dimension heads * d itself: each kind unpacked, and as the trainer lays it out (packed QKV, dense O and dO)
DENSE = [("a", (2, 3, 17, 64, 32, False)), ("a", (1, 3, 16, 16, 64, True)), ("b", (2, 1, 65, 16, 32, False)), ("b", (1, 3, 64, 64, 64, True)),
         ("c", (2, 3, 17, 63, 32, False)), ("c", (2, 1, 131, 131, 32, True)), ("d", (1, 1, 15, 131, 32, False, 128)), ("d", (1, 3, 17, 17, 32, True, 16))]


@pytest.mark.parametrize("kind,case", DENSE, ids=str)
def test_attention_exact_dense_leading_dimensions(kind, case):
    ref, got = exact_case(kind, torch.bfloat16, *case, dense=True)
    for name in ("dq", "dk", "dv"):
        assert same_bits(got[name], ref[name]), name
    assert ref["dv"].any()


# ---- bound cases: (heads, Lq, Lk, d, packed); B = 3: a partial mask, every key masked, no key masked -----------------------------------
BOUND = [(2, 35, 70, 32, False), (1, 17, 131, 64, False), (3, 65, 65, 64, True), (1, 63, 17, 32, False), (2, 16, 16, 32, True)]
MASKED = -2.0 ** 120         # below -1e30, so it absorbs q . k in fp32, and a finite number of bf16


def torch_grads16(q, k, v, mask, dout, heads, dtype):
    """`torch_attention_grads` in `dtype` with the mask clamped to the type's finite range: -2^120 is -Inf in fp16, where a row
    with every key masked would be NaN in torch; at the type's most negative finite number the scores of such a row are absorbed
    there too (its spacing is 32 in fp16), which is the uniform P the kernels and the float64 reference give."""
    lo = float(torch.finfo(dtype).min)
    return U.torch_attention_grads(q, k, v, np.maximum(mask, lo), dout, heads, dtype)


@functools.lru_cache(maxsize=None)
def bound_case(dtype, heads, Lq, Lk, d, packed):
    r = np.random.Generator(np.random.PCG64([heads, Lq, Lk, d]))
    H = heads * d
    q, k, v, dout = (X.round16(r.standard_normal((3, L_, H)), dtype) for L_ in (Lq, Lk, Lk, Lq))
    mask = np.zeros((3, Lk))
    mask[0, r.choice(Lk, Lk // 3, replace=False)] = MASKED
    mask[1, :] = MASKED
    ref = X.attention_grad16_reference(q, k, v, mask, dout, heads, dtype)
    g16 = torch_grads16(q, k, v, mask, dout, heads, dtype)
    return q, k, v, mask, dout, ref, dict(zip(("dq", "dk", "dv"), g16))


def held(tag, got, ref, g16, dtype):
    for name in ("dq", "dk", "dv"):
        ratio = np.abs(got[name] - ref[name]) / ref["b_" + name]
        d_cpu, d_gpu = U.maxnorm_rel(g16[name], ref[name]), U.maxnorm_rel(got[name], ref[name])
        print(f"{tag} {name}: worst error / bound {ratio.max():.3f}; d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, X.EPS16[dtype]):.3f}")
        assert ratio.max() <= 1.0, (name, ratio.max())
        assert d_gpu <= 8 * max(d_cpu, X.EPS16[dtype]), (name, d_cpu, d_gpu)


@pytest.mark.parametrize("case", BOUND, ids=str)
@pytest.mark.parametrize("dense", [False, True], ids=["padded", "dense"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_attention_bounds(dtype, dense, case):
    heads, packed = case[0], case[4]
    q, k, v, mask, dout, ref, g16 = bound_case(dtype, *case)
    got = dict(zip(("dq", "dk", "dv"), run_attention_grad16(q, k, v, mask, ref["o_given"], dout, heads, dtype, packed, dense)))
    held(f"{dtype} {case} dense={dense}", got, ref, g16, dtype)


def test_attention_same_input_same_bits():
    case = BOUND[2]
    q, k, v, mask, dout, ref, _ = bound_case(torch.bfloat16, *case)
    runs = [run_attention_grad16(q, k, v, mask, ref["o_given"], dout, case[0], torch.bfloat16, case[4]) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


# ---- the pair: vk_attention_tiled in bf16 in front of the backward, on the trainer's packed layout -------------------------------------
@pytest.mark.parametrize("heads,Lx,d", [(4, 16, 32), (2, 140, 64)])
def test_attention_backward_of_the_tiled_forward(heads, Lx, d):
    """O comes from attention_tiled_kernel (route asserted), not from the reference: dQ, dK, dV within the bounds with `o_given` =
    that O, and within 8 x torch's bf16 distance to float64."""
    dtype = torch.bfloat16
    q, k, v, mask, dout, _, g16 = bound_case(dtype, heads, Lx, Lx, d, True)
    B, H = 3, heads * d
    assert L.load().vk_attention_route(Lx, Lx, d, L.VK_BF16, 3 * H, 3 * H, 3 * H, 1, 1) == L.VK_ATT_ROUTE_TILED
    qkv = torch.from_numpy(np.concatenate((q, k, v), 2).reshape(B * Lx, 3 * H)).to(dtype).cuda()
    mk = torch.from_numpy(mask.astype(np.float32)).cuda()
    o = torch.empty((B * Lx, H), dtype=dtype, device="cuda")
    L.call("vk_attention_tiled", qkv.data_ptr(), 3 * H, qkv.data_ptr() + 2 * H, 3 * H, qkv.data_ptr() + 4 * H, 3 * H, mk.data_ptr(), o.data_ptr(), H,
           B, heads, Lx, Lx, d, L.VK_BF16, None)
    torch.cuda.synchronize()
    o = o.double().cpu().numpy().reshape(B, Lx, H)
    ref = X.attention_grad16_reference(q, k, v, mask, dout, heads, dtype, o_given=o)
    assert U.maxnorm_rel(o, ref["o"]) <= 4 * X.EPS16[dtype]                              # the forward's own O is the reference's to a few roundings
    got = dict(zip(("dq", "dk", "dv"), run_attention_grad16(q, k, v, mask, o, dout, heads, dtype, packed=True, dense=True)))
    held(f"pair L {Lx} d {d}", got, ref, g16, dtype)
