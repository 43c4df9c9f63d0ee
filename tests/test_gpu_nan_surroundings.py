"""GPU (-m gpu): the kernels that handle an edge by zero-filling or masking an operand (`vk_gemm_f32`, `vk_gemm_16`,
`vk_attention_grad`, `vk_attention_grad_16`, `vk_attention`, `vk_attention_tiled`) must not READ the bytes around their operands.

The other tests fill padding columns and guards with a large finite number.  That is blind to a one-sided leak: if one operand's
edge path read the padding where the other operand's path gave its zero, the product 1e30 x 0 = 0 would pass.  Stale memory of a
caching allocator can hold NaN, and 0 x NaN = NaN.  So every ragged case here runs twice in the same layout: once with the finite
poison, once with a quiet NaN of the buffer's type in every padding column of every INPUT and in a guard of 64 elements in front
of and behind it: the matrices, and the GEMMs' bias and the attention masks, which have no padding but guards (`Vector`).  Outputs
keep their finite sentinel in both runs.  The two results must be the same bits, and the outputs'
padding and guards must come back untouched (a bit compare) in both.  No reference is needed, and no byte outside the test's own
allocations is touched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                           # noqa: E402

import extents_util as E                                                                 # noqa: E402
import finetune_util as U                                                                # noqa: E402
import gpu_util as G                                                                     # noqa: E402
import mixed_util as X                                                                   # noqa: E402
import test_gpu_attention_grad as AG                                                     # noqa: E402
import test_gpu_attention_long as AL                                                     # noqa: E402
import test_gpu_mixed_kernels as MK                                                      # noqa: E402
import test_gpu_train_kernels as TK                                                      # noqa: E402

GUARD = 64
NAN = float("nan")


class Guarded:
    """One [rows, ld] matrix of a torch dtype with GUARD elements in front of and behind it.  Whoever constructs it with the
    module's input poison gets NaN in its place where `nan` is set: padding columns and both guards; an output's sentinel stays."""
    nan, poison = False, {}

    def __init__(self, rows, ld, dtype, fill):
        self.rows, self.ld, self.dtype = rows, ld, dtype
        if self.nan and float(fill) == float(self.poison[dtype]):
            fill = NAN
        self.host = torch.full((GUARD + rows * ld + GUARD,), float(fill), dtype=dtype)

    def _body(self, t):
        return t[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)

    def put(self, a, col0=0):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(self.rows, -1))).to(self.dtype)
        self._body(self.host)[:, col0:col0 + a.shape[1]] = a
        return self

    def upload(self):
        self.dev = self.host.cuda()
        return self

    def ptr(self, col0=0):
        return self.dev.data_ptr() + self.host.element_size() * (GUARD + col0)

    def view(self, cols):
        """The device matrix [rows, cols] with row stride ld."""
        return self._body(self.dev)[:, :cols]

    def _fetch(self, written):
        bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
        got = self.dev.cpu()
        keep = torch.ones(got.shape, dtype=torch.bool)
        for c0, c1 in written:
            self._body(keep)[:, c0:c1] = False
        assert (bits(got)[keep] == bits(self.host)[keep]).all(), "padding or guard overwritten"
        return self._body(got), self._body(bits(got)).numpy()


def buf16(nan_):
    class Buf(Guarded):
        nan, poison = nan_, MK.POISON

        def fetch(self, written):
            vals, bits = self._fetch(written)
            return vals.double().numpy(), bits
    return Buf


def buf32(nan_):
    class Buf(Guarded):
        nan, poison = nan_, {torch.float32: AG.POISON}

        def __init__(self, rows, ld, fill):
            Guarded.__init__(self, rows, ld, torch.float32, fill)

        def put(self, a, col0):
            Guarded.put(self, a, col0)

        def fetch(self, written):
            return self._fetch(written)[0].numpy()
    return Buf


class Vector:
    """An fp32 input that is no matrix (a GEMM's bias, an attention mask) with guards of GUARD elements on both sides."""

    def __init__(self, a, nan):
        a = np.asarray(a, np.float32).reshape(-1)
        host = np.full(a.size + 2 * GUARD, NAN if nan else 1e30, np.float32)
        host[GUARD:GUARD + a.size] = a
        self.n, self.dev = a.size, torch.from_numpy(host).cuda()

    def ptr(self):
        return self.dev.data_ptr() + 4 * GUARD


def twice(monkeypatch, module, factory, run, entry=None, index=None, vector=None):
    """run() under the finite poison and under NaN -> the two results.  `module`'s runners build their matrices through its `Buf`,
    which is replaced; their bias or mask is a plain tensor, so argument `index` of every call of `entry` is pointed at a guarded
    copy of `vector` (the array the caller hands the runner) on its way into the library."""
    outs = []
    for nan in (False, True):
        with monkeypatch.context() as m:
            m.setattr(module, "Buf", factory(nan))
            if vector is not None:
                real, held = L.call, []

                def call(name, *args, nan=nan, real=real, held=held):
                    if name == entry:
                        assert args[index] is not None
                        held.append(Vector(vector, nan))
                        args = args[:index] + (held[-1].ptr(),) + args[index + 1:]
                    return real(name, *args)
                m.setattr(L, "call", call)
            outs.append(run())
            assert vector is None or len(held) == 1, "the entry was not called"
    return outs


def same_bytes(a, b):
    a, b = (np.ascontiguousarray(t) for t in (a, b))
    return not np.isnan(a).any() and a.tobytes() == b.tobytes()


# ---- the GEMMs: every exact size whose K is no multiple of the K step -----------------------------------------------------------------
GEMM32 = [s for s in TK.GEMM_EXACT + [TK.GEMM_EXACT_LARGE] + E.LONG_K + [E.LARGE_LONG_K] if s[2] % 16]
GEMM16 = [s for s in MK.EDGES + MK.EDGES_LARGE + E.LONG_K + [E.LARGE_LONG_K] if s[2] % 64]


def run_gemm32(Buf, a, b, bias, ta, tb):
    """`vk_gemm_f32` with every operand in a `Buf`: A and B with 3 and 2 padding columns, C with 5; the bias in a `Vector`."""
    M, K = a.shape
    N = b.shape[1]
    sa, sb = (a.T if ta else a), (b.T if tb else b)
    A = Buf(sa.shape[0], sa.shape[1] + 3, AG.POISON)
    A.put(sa, 0)
    B = Buf(sb.shape[0], sb.shape[1] + 2, AG.POISON)
    B.put(sb, 0)
    C = Buf(M, N + 5, AG.SENT)
    A.upload(), B.upload(), C.upload()
    bd = Vector(bias, Buf.nan)
    L.call("vk_gemm_f32", A.ptr(), A.ld, ta, B.ptr(), B.ld, tb, bd.ptr(), C.ptr(), C.ld, M, N, K, 0, None)
    torch.cuda.synchronize()
    return C.fetch([(0, N)])[:, :N]


@pytest.mark.parametrize("size", GEMM32, ids=str)
def test_gemm_f32_ignores_its_surroundings(size):
    assert len(GEMM32) >= 9
    a, b, bias = (np.array(t) for t in E.gemm_case(*size, 6)[:3])
    for form, (ta, tb) in E.FORMS32.items():
        fin, nan = (run_gemm32(buf32(n), a, b, bias, ta, tb) for n in (False, True))
        assert same_bytes(fin, nan), (form, np.argwhere(fin != nan)[:8])


@pytest.mark.parametrize("size", GEMM16, ids=str)
@pytest.mark.parametrize("dtype", MK.DTYPES, ids=str)
def test_gemm_16_ignores_its_surroundings(monkeypatch, dtype, size):
    assert len(GEMM16) == 15
    a, b, bias = (np.array(t) for t in E.gemm_case(*size, 6)[:3])
    for form in MK.FORMS:
        fin, nan = twice(monkeypatch, MK, buf16, lambda: MK.run_gemm16(a, b, bias, form, dtype, out16=False)[1], "vk_gemm_16", 6, bias)
        assert same_bytes(fin.view(np.float32), nan.view(np.float32)), (form, np.argwhere(fin != nan)[:8])
    a, b, bias = (np.array(t) for t in E.gemm_case(*size, 7, one_hot=True)[:3])
    for form in MK.FORMS:
        fin, nan = twice(monkeypatch, MK, buf16, lambda: MK.run_gemm16(a, b, bias, form, dtype, out16=True)[1], "vk_gemm_16", 6, bias)
        assert (fin == nan).all() and not np.isnan(X.from_bits16(fin.view(np.uint16), dtype)).any(), form


# ---- the attention backward: every exact case with a length that is no multiple of 16 -----------------------------------------------
def ragged(cases):
    return [(kind, c) for kind, c in cases if c[2] % 16 or c[3] % 16]


ATT16 = ragged([(k, c) for k, cs in zip("abcd", (MK.CASE_A, MK.CASE_B, MK.CASE_C, MK.CASE_D)) for c in cs] + E.ATT16_EXACT)
ATT32 = ragged([(k, c) for k, cs in zip("abcd", (AG.CASE_A, AG.CASE_B, AG.CASE_C, AG.CASE_D)) for c in cs] + AG.WIDE + E.ATT32_EXACT)


@pytest.mark.parametrize("kind,case", ATT16, ids=str)
@pytest.mark.parametrize("dtype", MK.DTYPES, ids=str)
def test_attention_grad_16_ignores_its_surroundings(monkeypatch, dtype, kind, case):
    q, k, v, mask, dout = MK.exact_data(kind, *case)
    heads, packed = case[1], case[5]
    o = X.round16(U.attention_grad_reference(q, k, v, mask, dout, heads, scale=U.launcher_scale(case[4]))["o"], dtype)
    fin, nan = twice(monkeypatch, MK, buf16, lambda: MK.run_attention_grad16(q, k, v, mask, o, dout, heads, dtype, packed),
                     "vk_attention_grad_16", 6, mask)
    for name, f, n in zip(("dq", "dk", "dv"), fin, nan):
        assert same_bytes(f, n), name


@pytest.mark.parametrize("kind,case", ATT32, ids=str)
def test_attention_grad_ignores_its_surroundings(monkeypatch, kind, case):
    q, k, v, mask, dout = AG.exact_data(kind, *case)
    heads, packed = case[1], case[5]
    o = U.attention_grad_reference(q, k, v, mask, dout, heads, scale=U.launcher_scale(case[4]))["o"].astype(np.float32)
    f32 = lambda t: t.astype(np.float32)
    fin, nan = twice(monkeypatch, AG, buf32, lambda: AG.run_attention_grad(f32(q), f32(k), f32(v), mask, o, f32(dout), heads, packed),
                     "vk_attention_grad", 6, mask)
    for name, f, n in zip(("dq", "dk", "dv"), fin, nan):
        assert same_bytes(f, n), name


# ---- the forwards: q, k, v with a leading dimension of H + 8, every route ---------------------------------------------------------------
# (entry, dt, B, heads, Lq, Lk, d, route): the route is asked of the dispatcher in front of the launch
FORWARD = [("vk_attention", L.VK_BF16, 2, 3, 17, 63, 32, "mfma"), ("vk_attention", L.VK_F16, 2, 3, 33, 49, 64, "mfma"),
           ("vk_attention", L.VK_F32, 2, 3, 17, 63, 32, "lds"), ("vk_attention", L.VK_BF16, 3, 2, 65, 100, 64, "lds"),
           ("vk_attention", L.VK_BF16, 3, 2, 131, 131, 64, "tiled"), ("vk_attention", L.VK_F32, 3, 2, 131, 131, 64, "stream"),
           ("vk_attention_tiled", L.VK_BF16, 2, 3, 17, 63, 32, "tiled"), ("vk_attention_tiled", L.VK_F16, 3, 1, 65, 129, 64, "tiled"),
           ("vk_attention_tiled", L.VK_F32, 2, 3, 17, 63, 32, "stream"), ("vk_attention_tiled", L.VK_BF16, 3, 1, 35, 70, 48, "stream")]


def test_forward_cases_reach_every_route():
    assert {c[-1] for c in FORWARD} == set(AL.ROUTES)


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: f"{c[0]}-{AL.IDS[c[1]]}-{c[4]}x{c[5]}-d{c[6]}-{c[7]}")
def test_attention_forward_ignores_its_surroundings(case):
    """q, k, v and the output on a leading dimension of H + 8, the mask in a `Vector`; the output's 8 extra columns and its guards
    keep their sentinel in both runs."""
    entry, dt, B, heads, Lq, Lk, d, route = case
    assert Lq % 16 or Lk % 16
    td, H = G.TDT[dt], heads * d
    r = np.random.Generator(np.random.PCG64([B, heads, Lq, Lk, d]))
    q, k, v = (r.standard_normal((B * L_, H)) for L_ in (Lq, Lk, Lk))
    mask = AL.mixed_mask(B, Lk).numpy()
    outs = []
    for nan in (False, True):
        qb, kb, vb = (Guarded(len(a), H + 8, td, NAN if nan else MK.POISON[td]).put(a).upload() for a in (q, k, v))
        mk, out = Vector(mask, nan), Guarded(B * Lq, H + 8, td, MK.SENT[td]).upload()
        aligned = int((qb.ptr() | kb.ptr() | vb.ptr()) % 16 == 0)
        got = L.load().vk_attention_route(Lq, Lk, d, dt, H + 8, H + 8, H + 8, aligned, int(entry == "vk_attention_tiled"))
        assert got >= 0 and AL.ROUTES[got] == route, f"{entry}: route {got}, the test expects {route}"
        L.call(entry, qb.ptr(), H + 8, kb.ptr(), H + 8, vb.ptr(), H + 8, mk.ptr(), out.ptr(), H + 8, B, heads, Lq, Lk, d, dt, G.stream())
        torch.cuda.synchronize()
        vals, bits = out._fetch([(0, H)])
        assert not torch.isnan(vals[:, :H].float()).any()
        outs.append(bits[:, :H])
    assert (outs[0] == outs[1]).all()
