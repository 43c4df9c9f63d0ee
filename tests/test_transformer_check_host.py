"""CPU only: the per-element bounds of tests/transformer_check.py hold for correct arithmetic and fail for wrong arithmetic.

The emulations below restate, with torch in fp32, the rounding points of the attention kernels (csrc/attention.hip) and of the
LayerNorm kernels (csrc/layernorm.hip): operands read from the storage type, everything in fp32, P rounded to the storage type
where the matrix-core kernels round it, the output rounded once.  Each must sit below 1 on |out - ref| / bound against the float64
reference; each mutation (one live key dropped, two V rows swapped, LayerNorm dividing by the padded row length) must exceed 1."""
import numpy as np
import pytest
import torch

import transformer_check as T
from test_gpu_attention_long import mixed_mask

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
FMIN = float(np.finfo(np.float32).min)
ATT_CASES = [("mfma", 32, 1, 1), ("mfma", 64, 15, 17), ("mfma", 32, 20, 36), ("mfma", 64, 36, 20), ("mfma", 64, 48, 64), ("mfma", 32, 47, 49),
             ("lds", 16, 33, 31), ("lds", 64, 50, 100), ("lds", 20, 20, 36), ("lds", 64, 1, 64),
             ("tiled", 64, 17, 65), ("tiled", 64, 33, 129), ("stream", 64, 17, 65), ("stream", 64, 33, 129),
             # the D = 32 builds and three key tiles; then the head dims up to the contracts' limits (test_gpu_attention_builds.py)
             ("tiled", 32, 13, 150), ("tiled", 32, 50, 129), ("stream", 32, 13, 150),
             ("stream", 128, 17, 65), ("stream", 128, 33, 129), ("stream", 256, 17, 65), ("stream", 256, 33, 129), ("stream", 1, 17, 65),
             ("lds", 128, 20, 36), ("lds", 256, 20, 36), ("lds", 64, 127, 127)]


def draw(seed, B, heads, Lq, Lk, d, td):
    gen = np.random.Generator(np.random.PCG64(seed))
    H = heads * d
    q, k, v = (torch.from_numpy(gen.standard_normal((B * n, H)).astype(np.float32)).to(td) for n in (Lq, Lk, Lk))
    return q, k, v


def emulate_attention(q, k, v, add, B, heads, Lq, Lk, d, td, route):
    """The route's kernel in torch fp32.  mfma / lds: the whole score row, p = exp(s - max) * (1 / sum); tiled / stream: 64-key
    tiles with the running maximum and sum, p = exp(s - max so far) unnormalised, O / l at the end.  mfma and tiled round p to the
    storage type for the second product (the sum l takes the unrounded p)."""
    H = heads * d
    qh, kh, vh = (t.float().view(B, n, heads, d).transpose(1, 2) for t, n in ((q, Lq), (k, Lk), (v, Lk)))
    s = (qh @ kh.transpose(-1, -2)) * np.float32(1.0 / np.sqrt(np.float32(d)))
    if add is not None:
        s = s + add[:, None, None, :]
    rp = (lambda p: p.to(td).float()) if T.ROUNDS_P[route] else (lambda p: p)
    if route in ("mfma", "lds"):
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = rp(e * (1.0 / e.sum(-1, keepdim=True))) @ vh
    else:
        m = torch.full((B, heads, Lq, 1), -np.inf)
        l = torch.zeros((B, heads, Lq, 1))
        o = torch.zeros((B, heads, Lq, d))
        for k0 in range(0, Lk, 64):
            st = s[..., k0:k0 + 64]
            mn = torch.maximum(m, st.amax(-1, keepdim=True))
            alpha, p = torch.exp(m - mn), torch.exp(st - mn)
            l = alpha * l + p.sum(-1, keepdim=True)
            o = alpha * o + rp(p) @ vh[:, :, k0:k0 + 64]
            m = mn
        o = o / l
    return o.permute(0, 2, 1, 3).reshape(B * Lq, H).to(td)


# the matrix-core kernels take the 16-bit types only
ATT_PARAMS = [(td, *c) for c in ATT_CASES for td in DTYPES if not (td == torch.float32 and T.ROUNDS_P[c[0]])]


@pytest.mark.parametrize("td,route,d,Lq,Lk", ATT_PARAMS, ids=["-".join([T.NAMES[p[0]]] + [str(x) for x in p[1:]]) for p in ATT_PARAMS])
def test_attention_emulation_fits_and_mutations_do_not(td, route, d, Lq, Lk):
    B, heads = 3, 3
    q, k, v = draw(Lq * Lk + d, B, heads, Lq, Lk, d, td)
    for add in (mixed_mask(B, Lk), None):
        r = T.attention_reference(q, k, v, add, B, heads, Lq, Lk, d)
        bound = T.attention_bound(r, td, route)
        w = T.assert_within(emulate_attention(q, k, v, add, B, heads, Lq, Lk, d, td, route), r["ref"], bound,
                            f"emulated attention {route} {T.NAMES[td]} d {d} Lq {Lq} Lk {Lk} {'masked' if add is not None else 'plain'}")
        assert w < 1
    if Lk < 2:
        return
    # mutations, on the unmasked case (every key live): the emulation sees other inputs than the reference
    drop = torch.zeros((B, Lk))
    drop[:, Lk // 2] = FMIN
    vs = v.view(B, Lk, -1).clone()
    vs[:, [0, Lk - 1]] = vs[:, [Lk - 1, 0]]
    for name, out in (("one key dropped", emulate_attention(q, k, v, drop, B, heads, Lq, Lk, d, td, route)),
                      ("two V rows swapped", emulate_attention(q, k, vs.view(B * Lk, -1), None, B, heads, Lq, Lk, d, td, route))):
        w, _ = T.worst_ratio(out, r["ref"], bound)
        print(f"\n[{name}: {route} {T.NAMES[td]} d {d} Lq {Lq} Lk {Lk}] worst ratio {w:.1f}", end="")
        assert w > 1, name


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """With 2^-9 (half of bf16's unit roundoff) correct arithmetic does not fit: the constant is not a matter of taste."""
    td, route, d, Lq, Lk, B, heads = torch.bfloat16, "lds", 16, 33, 31, 3, 3
    q, k, v = draw(Lq * Lk + d, B, heads, Lq, Lk, d, td)
    add = mixed_mask(B, Lk)
    r = T.attention_reference(q, k, v, add, B, heads, Lq, Lk, d)
    out = emulate_attention(q, k, v, add, B, heads, Lq, Lk, d, td, route)
    assert T.worst_ratio(out, r["ref"], T.attention_bound(r, td, route))[0] < 1
    saved = T.U[td]
    try:
        T.U[td] = 2.0 ** -9
        assert T.worst_ratio(out, r["ref"], T.attention_bound(r, td, route))[0] > 1
    finally:
        T.U[td] = saved


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
def emulate_layernorm(x32, gamma, beta, eps, scale, y_old, td, divisor=None):
    """fp32 mean and two-pass population variance over the values as read (x32: fp32), 1 / sqrt(var + eps), the affine map, the scale,
    the old y added, one rounding."""
    C = x32.shape[1] if divisor is None else divisor
    mean = x32.sum(1, keepdim=True) / np.float32(C)
    dd = x32 - mean
    rstd = 1.0 / torch.sqrt((dd * dd).sum(1, keepdim=True) / np.float32(C) + np.float32(eps))
    o = (dd * rstd * gamma + beta) * np.float32(scale)
    if y_old is not None:
        o = o + y_old.float()
    return o.to(td)


def ln_inputs(seed, M, C, td, kind):
    gen = np.random.Generator(np.random.PCG64(seed))
    z = gen.standard_normal((M, C))
    x = torch.from_numpy((z * 3 + 1 if kind == "wide" else 1000 + z).astype(np.float32)).to(td)
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
    y_old = torch.from_numpy(gen.standard_normal((M, C)).astype(np.float32)).to(td)
    return x, gm, bt, y_old


@pytest.mark.parametrize("td", DTYPES, ids=[T.NAMES[t] for t in DTYPES])
@pytest.mark.parametrize("C", [8, 63, 100, 768, 2047, 2048])
@pytest.mark.parametrize("kind", ["wide", "offset"])
def test_layernorm_emulation_fits_and_wrong_divisor_does_not(td, C, kind):
    M = 5
    x, gm, bt, y_old = ln_inputs(C, M, C, td, kind)
    for scale, acc in ((1.0, None), (0.5, y_old)):
        r = T.layernorm_reference(x, gm, bt, 1e-12, scale, acc)
        bound = T.layernorm_bound(r, td)
        w = T.assert_within(emulate_layernorm(x.float(), gm, bt, 1e-12, scale, acc, td), r["ref"], bound,
                            f"emulated layernorm {T.NAMES[td]} C {C} {kind} scale {scale} acc {int(acc is not None)}")
        assert w < 1
        padded = C + 8 if C % 8 == 0 else (C + 7) // 8 * 8             # the row stride _linear leaves behind
        w, _ = T.worst_ratio(emulate_layernorm(x.float(), gm, bt, 1e-12, scale, acc, td, divisor=padded), r["ref"], bound)
        print(f"\n[divided by the padded length {padded}: {T.NAMES[td]} C {C} {kind}] worst ratio {w:.1f}", end="")
        assert w > 1


@pytest.mark.parametrize("td", DTYPES, ids=[T.NAMES[t] for t in DTYPES])
def test_embedding_emulation_fits(td):
    """The embedding kernel adds the three table rows in fp32 (two roundings); the reference LayerNorms their float64 sum."""
    gen = np.random.Generator(np.random.PCG64(2))
    M, C = 27, 768
    w, p, t = (torch.from_numpy(gen.standard_normal((M, C)).astype(np.float32)).to(td) for _ in range(3))
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(C).astype(np.float32))
    r = T.layernorm_reference(w.double() + p.double() + t.double(), gm, bt, 1e-12, 1.0)
    out = emulate_layernorm(w.float() + p.float() + t.float(), gm, bt, 1e-12, 1.0, None, td)
    assert T.assert_within(out, r["ref"], T.layernorm_bound(r, td), f"emulated embedding {T.NAMES[td]}") < 1


def test_assert_within_checks_every_element_and_names_the_worst():
    ref = torch.zeros((3, 4), dtype=torch.float64)
    bound = torch.full((3, 4), 1e-3, dtype=torch.float64)
    out = torch.zeros((3, 4))
    assert T.assert_within(out, ref, bound, "zeros") == 0.0
    out[2, 1] = 5e-3
    with pytest.raises(AssertionError, match=r"\(2, 1\)"):
        T.assert_within(out, ref, bound, "one element off")
    out[2, 1] = float("nan")
    with pytest.raises(AssertionError):
        T.assert_within(out, ref, bound, "not finite")
    bound[0, 0] = 0.0                                        # a zero bound asks for the exact value
    out[2, 1] = 0.0
    assert T.assert_within(out, ref, bound, "zero bound, exact") == 0.0
    out[0, 0] = 1e-30
    with pytest.raises(AssertionError, match=r"\(0, 0\)"):
        T.assert_within(out, ref, bound, "zero bound, off")
