"""-m gpu: vk_attention_relpos against float64, per element, with the form it must run on.

The reference is transformer_check.attention_reference with the bias added to the scores before the soft-max: every (batch, head,
query) is handed to it as a batch entry of its own, one head and one query, whose additive row is mask[b] + bias[b, h, i] / sqrt(d).

The bound is derived, not measured.  The kernel's score is (dot + (t1 + (tx + ty))) * scale + mask in fp32.  attention_bound's
fp32 term 2 (d + 2) 2^-24 S_r covers a score that is a rounded sum of magnitude at most S_r times the scale; the bias joins that
sum as one more term (the addition dot + bias, then the scale), so S_r grows by the row's max_j (|t1| + |tx| + |ty|) / sqrt(d) =: Bs_r.
The two additions that form the bias itself (tx + ty, then t1 + that) each round once, at most 2^-24 (|t1| + |tx| + |ty|) apiece, which
reaches a score as 2 2^-24 Bs_r and the difference of two scores as twice that:

    bound = attention_bound(S_r + Bs_r)  +  4 2^-24 Bs_r A

The table lookups are exact (integers), and P is rounded to the storage type on the matrix-core form only (u_P as for "tiled")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                          # noqa: E402
from vltk_amd.layoutlmv3 import attention_relpos, attention_relpos_form   # noqa: E402

import gpu_util as G                                                    # noqa: E402
from transformer_check import U32, assert_within, attention_bound, attention_reference   # noqa: E402

FMIN = float(np.finfo(np.float32).min)
TDS = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]
# (B, heads, Lq, Lk, d): one token; a key tile + 1, a query block + 1 and 6 (batch, head) pairs; past 128 queries and two key tiles; exact tiles
SHAPES = [(1, 1, 1, 1, 32), (2, 3, 17, 65, 64), (1, 3, 130, 129, 32), (2, 2, 64, 64, 64)]
QUERIES = {1: 16, 17: 32, 130: 128, 64: 64}          # the matrix-core form's queries per workgroup


def make_case(td, B, heads, Lq, Lk, d, r1, r2, coords):
    """Stored operands on the CPU.  Positions run 0 .. L - 1 (differences up to 16 at L = 17 against r1 = 8); x and y are drawn from
    `coords` (0 .. 39 against r2 = 16, or the two ends 0 and 1000 against 256): saturated and unsaturated differences of both signs.
    The mask is ragged: batch b loses its last (5 b + 3) % Lk keys."""
    gen = np.random.Generator(np.random.PCG64(1000 * Lq + Lk + d))
    H = heads * d

    def normal(*shape):
        return torch.from_numpy(gen.standard_normal(shape).astype(np.float32))

    def triples(Lx):
        pos = np.broadcast_to(np.arange(Lx), (B, Lx))
        return torch.from_numpy(np.stack([pos, gen.choice(coords, (B, Lx)), gen.choice(coords, (B, Lx))], -1).astype(np.int32))
    add = torch.zeros((B, Lk))
    for b in range(B):
        cut = (5 * b + 3) % Lk
        add[b, Lk - cut:] = FMIN
    return dict(q=normal(B * Lq, H).to(td), k=normal(B * Lk, H).to(td), v=normal(B * Lk, H).to(td), rq=triples(Lq), rk=triples(Lk),
                lut=normal(heads, (2 * r1 + 1) + 2 * (2 * r2 + 1)), add=add)


def reference(c, B, heads, Lq, Lk, d, r1, r2):
    """-> (ref, bound inputs) as [B * Lq, heads * d]; the bias in float64 from the stored table and triples."""
    n1, n2 = 2 * r1 + 1, 2 * r2 + 1
    lut = c["lut"].double()
    dl = c["rk"].long()[:, None, :, :] - c["rq"].long()[:, :, None, :]                     # [B, Lq, Lk, 3]
    hd = torch.arange(heads)[None, :, None, None]

    def look(col, r, off):
        return lut[hd, dl[..., col].clamp(-r, r)[:, None] + r + off]                         # [B, heads, Lq, Lk]
    t1, tx, ty = look(0, r1, 0), look(1, r2, n1), look(2, r2, n1 + n2)
    scale = 1.0 / np.sqrt(float(d))
    N = B * heads * Lq

    def per_query(t):                                                 # k or v [B * Lk, H] -> the head's keys again for each (b, h, i)
        return t.reshape(B, Lk, heads, d).transpose(1, 2)[:, :, None].expand(B, heads, Lq, Lk, d).reshape(N * Lk, d)
    add = (c["add"].double()[:, None, None, :] + (t1 + tx + ty) * scale).reshape(N, Lk)
    q1 = c["q"].reshape(B, Lq, heads, d).transpose(1, 2).reshape(N, d)
    r = attention_reference(q1, per_query(c["k"]), per_query(c["v"]), add, N, 1, 1, Lk, d)
    Bs = ((t1.abs() + tx.abs() + ty.abs()).amax(-1) * scale).reshape(N, 1)

    def rows(t):
        return t.reshape(B, heads, Lq, d).permute(0, 2, 1, 3).reshape(B * Lq, heads * d)
    out = {key: rows(r[key]) for key in ("ref", "A", "sumv")}
    out.update(S=rows(r["S"] + Bs), Bs=rows(Bs.expand(N, d)), Lk=Lk, d=d)
    return out


def run(td, B, heads, Lq, Lk, d, r1=8, r2=16, coords=np.arange(40), form="mfma"):
    c = make_case(td, B, heads, Lq, Lk, d, r1, r2, coords)
    dev = {key: t.to(G.DEV) for key, t in c.items()}
    got = attention_relpos_form(Lq, Lk, d, td, heads * d, heads * d, heads * d)
    assert got == (form, QUERIES[Lq] if form == "mfma" else 16), got
    out = attention_relpos(dev["q"], dev["k"], dev["v"], dev["rq"], dev["rk"], dev["lut"], r1, r2, heads, mask=dev["add"])
    again = attention_relpos(dev["q"], dev["k"], dev["v"], dev["rq"], dev["rk"], dev["lut"], r1, r2, heads, mask=dev["add"])
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    r = reference(c, B, heads, Lq, Lk, d, r1, r2)
    bound = attention_bound(r, td, "tiled" if form == "mfma" else "stream") + 4 * U32 * r["Bs"] * r["A"]
    return assert_within(out, r["ref"], bound, f"relpos {form} {td} B{B} h{heads} Lq{Lq} Lk{Lk} d{d} r{r1}/{r2}")


@pytest.mark.parametrize("td", TDS, ids=IDS)
@pytest.mark.parametrize("B,heads,Lq,Lk,d", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_vs_float64(td, B, heads, Lq, Lk, d):
    run(td, B, heads, Lq, Lk, d, form="strict" if td == torch.float32 else "mfma")


def test_fp32_head_dim_48():
    run(torch.float32, 2, 3, 17, 65, 48, form="strict")


def test_sixteen_bit_on_the_strict_form(monkeypatch):
    """The matrix cores switched off: bf16 through the fp32 kernel, P not rounded."""
    monkeypatch.setenv("VK_ATTENTION_MFMA", "0")
    run(torch.bfloat16, 2, 3, 17, 65, 64, form="strict")


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_default_radii_page_corners(td):
    """LayoutLMv3's radii 128 / 256 (a table of 1283 floats a head) with every coordinate at 0 or 1000: each 2-D difference is 0
    or saturated, of either sign."""
    run(td, 2, 3, 17, 65, 64, r1=128, r2=256, coords=np.array([0, 1000]), form="strict" if td == torch.float32 else "mfma")
