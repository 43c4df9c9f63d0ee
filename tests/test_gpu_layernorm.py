"""-m gpu: vk_layernorm and vk_embed_layernorm (csrc/layernorm.hip, the row body of csrc/row_norm.h) per element against float64
and bit-exact.  The row strides are walked as the encoders pass them: ld == C, the padded strides vk_linear
leaves behind (layernorm_kernel<T, 16 / sizeof(T)>, the 16-byte-chunk form, where C and the bases allow it) and odd strides
(layernorm_kernel<T, 1>, one element per lane and step, at every C); the columns of y past C must stay untouched and the columns
of x past C unread.  The entries that share the row body (vk_layoutlm_embed among them) are bit-equal on equal rows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
import transformer_check as T                          # noqa: E402
from test_gpu_lxmert import TDT                        # noqa: E402

ALL = [L.VK_F32, L.VK_F16, L.VK_BF16]
IDS = {L.VK_F32: "fp32", L.VK_F16: "fp16", L.VK_BF16: "bf16"}
CS = [8, 63, 64, 65, 100, 768, 2040, 2047, 2048]
LDS = ["tight", "padded", "odd"]                        # (ldx, ldy) = (C, C), (C + 8, C + 16), (C + 1, C + 3)
EPS = 1e-12
SENTINEL = -77.0


def strides(C, ld):
    return {"tight": (C, C), "padded": (C + 8, C + 16), "odd": (C + 1, C + 3)}[ld]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def layernorm(x, gm, bt, dt, ldx, ldy, scale, y_old=None, offset=0):
    """x [M, C] (storage type, CPU) -> y [M, C] (CPU).  x lies in a [M, ldx] buffer whose other columns hold 1e4 (a kernel that
    reads them lands far off); y in a [M, ldy] buffer prefilled with the sentinel (y_old in the first C columns when accumulating),
    whose columns past C are asserted untouched.  Both buffers start `offset` elements into their allocations (1e4 / the sentinel
    in front), and the elements in front of y must keep their bytes too."""
    M, C = x.shape
    td = TDT[dt]
    xf = torch.full((offset + M * ldx,), 1e4, dtype=td)
    xf[offset:].view(M, ldx)[:, :C] = x
    yf = torch.full((offset + M * ldy,), SENTINEL, dtype=td)
    if y_old is not None:
        yf[offset:].view(M, ldy)[:, :C] = y_old
    xd, yd, gd, bd = xf.to(G.DEV), yf.to(G.DEV), gm.to(G.DEV), bt.to(G.DEV)
    L.call("vk_layernorm", G.P(xd[offset:]), ldx, G.P(gd), G.P(bd), G.P(yd[offset:]), ldy, M, C, EPS, scale, int(y_old is not None), dt,
           G.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(yd[:offset]), bits(yf[:offset])), "elements in front of y were written"
    y, yb = yd.cpu()[offset:].view(M, ldy), yf[offset:].view(M, ldy)
    assert torch.equal(bits(y[:, C:]), bits(yb[:, C:])), "columns of y past C were written"
    return y[:, :C]


# ---- 1. per element against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("ld", LDS)
def test_layernorm_per_element(dt, C, ld):
    """Rows N(1, 3) and 1000 + N(0, 1) (the mean's rounding against a small spread), scale 1 and 0.5, with and without the old y."""
    td = TDT[dt]
    ldx, ldy = strides(C, ld)
    gen = np.random.Generator(np.random.PCG64([C, LDS.index(ld)]))
    for M in [1, 5] + ([130] if C in (100, 2048) else []):
        gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
        bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
        y_old = torch.from_numpy(gen.standard_normal((M, C)).astype(np.float32)).to(td)
        for kind in ("wide", "offset"):
            z = gen.standard_normal((M, C))
            x = torch.from_numpy((z * 3 + 1 if kind == "wide" else 1000 + z).astype(np.float32)).to(td)
            for scale in (1.0, 0.5):
                for acc in (None, y_old):
                    y = layernorm(x, gm, bt, dt, ldx, ldy, scale, acc)
                    r = T.layernorm_reference(x, gm, bt, EPS, scale, acc)
                    T.assert_within(y, r["ref"], T.layernorm_bound(r, td),
                                    f"layernorm {IDS[dt]} {ld} M {M} C {C} {kind} scale {scale} acc {int(acc is not None)}")


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
def test_layernorm_misaligned_bases(dt):
    """Strides that are multiples of the 16-byte chunk under bases that are not 16-byte aligned (x and y start one element into
    their allocations): the one-element form has to take the launch."""
    td = TDT[dt]
    M, C = 5, 128
    ldx, ldy = strides(C, "padded")
    gen = np.random.Generator(np.random.PCG64([C, 77]))
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
    y_old = torch.from_numpy(gen.standard_normal((M, C)).astype(np.float32)).to(td)
    x = torch.from_numpy((gen.standard_normal((M, C)) * 3 + 1).astype(np.float32)).to(td)
    for scale in (1.0, 0.5):
        for acc in (None, y_old):
            y = layernorm(x, gm, bt, dt, ldx, ldy, scale, acc, offset=1)
            r = T.layernorm_reference(x, gm, bt, EPS, scale, acc)
            T.assert_within(y, r["ref"], T.layernorm_bound(r, td), f"layernorm {IDS[dt]} misaligned scale {scale} acc {int(acc is not None)}")


# ---- 2. exact --------------------------------------------------------------------------------------------------------------
def dyadic(gen, n, lo, hi, step):
    return torch.from_numpy((gen.integers(int(lo / step), int(hi / step) + 1, n) * step).astype(np.float32))


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("C", [1] + CS)
def test_exact_constant_rows(dt, C):
    """x = k (an integer, |k| <= 64): the fp32 sum k C and the mean k are exact, every x - mean is 0 and the output is beta * scale
    rounded once, whatever gamma is."""
    td = TDT[dt]
    gen = np.random.Generator(np.random.PCG64(C))
    ks = torch.tensor([-64.0, -3.0, 0.0, 1.0, 7.0, 64.0])
    x = ks[:, None].expand(len(ks), C).to(td)
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = dyadic(gen, C, -4, 4, 0.125)
    for ld in ("tight", "odd"):
        for scale in (1.0, 0.5):
            y = layernorm(x, gm, bt, dt, *strides(C, ld), scale)
            want = (bt * np.float32(scale)).to(td)[None].expand(len(ks), C)
            assert torch.equal(bits(y), bits(want)), (ld, scale)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("C", [8, 64, 100, 768, 2040, 2048])
def test_exact_balanced_signs(dt, C):
    """Rows of as many +1 as -1 (alternating, in halves, shuffled): mean 0 and variance 1 exactly, and 1 + 1e-12 is 1 in fp32, so
    the output is (+-gamma + beta) * scale rounded once (gamma, beta small dyadic values: the fp32 value is exact)."""
    td = TDT[dt]
    gen = np.random.Generator(np.random.PCG64(C))
    alt = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    halves = np.where(np.arange(C) < C // 2, 1.0, -1.0)
    xs = torch.from_numpy(np.stack([alt, -alt, halves, gen.permutation(alt), gen.permutation(alt)]).astype(np.float32))
    gm = dyadic(gen, C, 0.5, 1.5, 0.125)
    bt = dyadic(gen, C, -2, 2, 0.125)
    for ld in ("tight", "odd"):
        for scale in (1.0, 0.5):
            y = layernorm(xs.to(td), gm, bt, dt, *strides(C, ld), scale)
            want = ((xs * gm + bt) * np.float32(scale)).to(td)
            assert torch.equal(bits(y), bits(want)), (ld, scale)


# ---- 3. the embedding stage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("C", [100, 128, 768, 2048])
@pytest.mark.parametrize("Lt", [1, 9])
def test_embed_layernorm_per_element(dt, C, Lt):
    """LayerNorm(word[id] + position[row % L] + token_type[tt]) against the float64 LayerNorm of the float64 sum of the three
    stored rows; the ids include 0 and V - 1, both token types appear, and with B = 3 the position index wraps."""
    td = TDT[dt]
    B, V = 3, 50
    gen = np.random.Generator(np.random.PCG64([C, Lt]))
    word, pos, typ = (torch.from_numpy(gen.standard_normal(s).astype(np.float32)).to(td) for s in ((V, C), (16, C), (2, C)))
    ids = torch.from_numpy(gen.integers(0, V, (B, Lt)))
    tts = torch.from_numpy(gen.integers(0, 2, (B, Lt)))
    ids[0, 0], ids[1, -1], ids[2, 0] = 0, V - 1, V - 1
    tts[0, 0], tts[1, 0], tts[2, -1] = 0, 1, 1
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
    dev = [t.to(G.DEV) for t in (ids, tts, word, pos, typ, gm, bt)]
    y = torch.empty((B * Lt, C), dtype=td, device=G.DEV)
    L.call("vk_embed_layernorm", G.P(dev[0]), G.P(dev[1]), B, Lt, G.P(dev[2]), G.P(dev[3]), G.P(dev[4]), G.P(dev[5]), G.P(dev[6]), G.P(y),
           C, EPS, dt, G.stream())
    torch.cuda.synchronize()
    e = (word.double()[ids] + pos.double()[torch.arange(Lt)][None] + typ.double()[tts]).view(B * Lt, C)
    r = T.layernorm_reference(e, gm, bt, EPS, 1.0)
    T.assert_within(y, r["ref"], T.layernorm_bound(r, td), f"embed layernorm {IDS[dt]} C {C} L {Lt}")


@functools.lru_cache(maxsize=None)
def shared_rows(dt, C):
    """One set of word / position / token-type tables, ids and gamma / beta through vk_embed_layernorm and through
    vk_layoutlm_embed with all-zero x, y, h and w tables (B = 3, L = 9).  Adding a +0 row is exact and leaves
    (word + position) + token_type, vk_embed_layernorm's order, unless a sum is -0: the host asserts that none is.  Returns both
    outputs and that sum in fp32 (CPU)."""
    td = TDT[dt]
    B, Lt, V, P, M2 = 3, 9, 50, 16, 8
    gen = np.random.Generator(np.random.PCG64([C, 9]))
    word, pos, typ = (torch.from_numpy(gen.standard_normal(s).astype(np.float32)).to(td) for s in ((V, C), (P, C), (2, C)))
    ids = torch.from_numpy(gen.integers(0, V, (B, Lt)))
    tts = torch.from_numpy(gen.integers(0, 2, (B, Lt)))
    box = torch.from_numpy(np.sort(gen.integers(0, M2, (B, Lt, 2, 2)), -2).reshape(B, Lt, 4).astype(np.int32))   # x0 y0 x1 y1
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
    part = word.float()[ids] + pos.float()[:Lt][None]
    total = (part + typ.float()[tts]).view(B * Lt, C)
    for t in (part, total):
        assert not ((t == 0) & torch.signbit(t)).any(), "a -0 sum: adding the +0 rows would change it"
    zero = torch.zeros((M2, C), dtype=td, device=G.DEV)
    d = [t.to(G.DEV) for t in (ids, tts, word, pos, typ, gm, bt, box)]
    ye, yl = (torch.full((B * Lt, C), SENTINEL, dtype=td, device=G.DEV) for _ in range(2))
    L.call("vk_embed_layernorm", G.P(d[0]), G.P(d[1]), B, Lt, G.P(d[2]), G.P(d[3]), G.P(d[4]), G.P(d[5]), G.P(d[6]), G.P(ye), C, EPS, dt,
           G.stream())
    L.call("vk_layoutlm_embed", G.P(d[0]), G.P(d[1]), G.P(d[7]), B, Lt, G.P(d[2]), V, G.P(d[3]), P, G.P(zero), G.P(zero), G.P(zero),
           G.P(zero), M2, G.P(d[4]), 2, G.P(d[5]), G.P(d[6]), G.P(yl), C, EPS, dt, G.stream())
    torch.cuda.synchronize()
    return dict(embed=ye.cpu(), layoutlm=yl.cpu(), total=total, gm=gm, bt=bt)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("C", [63, 65, 2047])
def test_layoutlm_embed_bit_equals_embed_layernorm(dt, C):
    """Odd C: both entries take the one-element form, and the shared row body makes equal rows equal bits."""
    r = shared_rows(dt, C)
    assert torch.equal(bits(r["layoutlm"]), bits(r["embed"]))


@pytest.mark.parametrize("C", [63, 65, 128])
def test_embed_entries_bit_equal_layernorm_of_the_host_sum(C):
    """fp32: vk_layernorm (tight strides, scale 1, no accumulate) on (word[ids] + position) + token_type summed on the host gives
    the bits of vk_embed_layernorm at odd C (both on the one-element form) and of vk_layoutlm_embed at C = 128 (both on the
    16-byte-chunk form; vk_embed_layernorm stays on the one-element form there)."""
    r = shared_rows(L.VK_F32, C)
    y = layernorm(r["total"], r["gm"], r["bt"], L.VK_F32, C, C, 1.0)
    assert torch.equal(bits(y), bits(r["embed" if C % 4 else "layoutlm"]))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_sizes():
    """C beyond 2048 and an empty batch are refused by the host check, before any launch: y keeps its bytes."""
    lib = L.load()
    x = torch.zeros((4, 2056), device=G.DEV)
    y = torch.full((4, 2056), SENTINEL, device=G.DEV)
    gm, bt = torch.ones(2056, device=G.DEV), torch.zeros(2056, device=G.DEV)
    ok = dict(M=4, C=2048)
    for patch in (dict(C=2049), dict(M=0), dict(C=0), dict(M=-1)):
        a = dict(ok, **patch)
        args = (G.P(x), 2056, G.P(gm), G.P(bt), G.P(y), 2056, a["M"], a["C"], EPS, 1.0, 0, L.VK_F32, G.stream())
        assert lib.vk_layernorm(*args) == L.VK_EINVAL
        with pytest.raises(ValueError):
            L.call("vk_layernorm", *args)
    assert lib.vk_layernorm(G.P(x), 2056, G.P(gm), G.P(bt), G.P(y), 2056, 4, 2048, EPS, 1.0, 0, L.VK_I32, G.stream()) == L.VK_EINVAL
    ids = torch.zeros((4,), dtype=torch.int64, device=G.DEV)
    for B, Lt, C in ((4, 1, 2049), (0, 1, 128), (4, 0, 128)):
        with pytest.raises(ValueError):
            L.call("vk_embed_layernorm", G.P(ids), G.P(ids), B, Lt, G.P(x), G.P(x), G.P(x), G.P(gm), G.P(bt), G.P(y), C, EPS, L.VK_F32,
                   G.stream())
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL))
    L.call("vk_layernorm", G.P(x), 2056, G.P(gm), G.P(bt), G.P(y), 2056, 4, 2048, EPS, 1.0, 0, L.VK_F32, G.stream())
    torch.cuda.synchronize()
    assert torch.equal(y[:, :2048], torch.zeros((4, 2048), device=G.DEV)) and torch.equal(y[:, 2048:], torch.full((4, 8), SENTINEL, device=G.DEV))
