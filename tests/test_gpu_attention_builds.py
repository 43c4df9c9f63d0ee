"""-m gpu: every build of the two long-sequence attention kernels, and every kernel's head dims up to its contract's limit
(DESIGN.md section 20a), with the tools of test_gpu_attention_small.py: every output element against float64 within
transformer_check.attention_bound, and data on which the output is exact.

attention_tiled_kernel<T, D, QB> has eight builds: T in {f16, bf16} x D in {32, 64} x QB in {1, 2}; the launcher takes QB = 1 (16
queries to a wave) for Lq <= 16 and QB = 2 otherwise (`tiled_launch` of csrc/attention.hip; `tiled_build` below restates it, the
dispatcher reports the route only).  attention_stream_kernel<T> has three, one per type; a thread of it owns the outputs
tid + 256 n, n < 16 d / 256, so head dims past 64 are what reaches n >= 4, and from d = 106 on it asks for more than 64 KiB of LDS.
attention_kernel takes whatever fits 160 KiB: (127, 127, 64) in fp32 is the largest image the rule admits, 163 576 bytes.

Every launch goes through vk_attention / vk_attention_tiled, with the route asked of vk_attention_route immediately before it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
from test_gpu_attention_long import ALL, IDS, attention                                 # noqa: E402
from test_gpu_attention_small import LONG_CASES, SIXTEEN, on_route, per_element, same_bits       # noqa: E402
from test_gpu_lxmert import TDT                        # noqa: E402

LONG_IDS = [f"{IDS[dt]}-{r}" for dt, r in LONG_CASES]

# ---- 1. per element, every build ---------------------------------------------------------------------------------------------
# Lq <= 16: QB = 1; Lq = 17 / 33 / 50: a second item of 1 / 1 / 18 rows; Lk = 32 | 33 and 96 | 97: the second product's nk2 switch
# (Lk - k0 > 32) in the first and in a later tile; Lk = 65 / 129: a last tile of one key; Lk = 1: a single key.
BUILD_PAIRS = [(1, 1), (1, 65), (13, 150), (16, 16), (16, 64), (17, 32), (17, 33), (32, 96), (33, 97), (50, 129)]
OTHER_BH = [(16, 64), (50, 129)]                       # also at (B, heads) = (1, 1), (2, 2): no idle wave in the last workgroup of four
HEAD_DIMS = [32, 64]


def tiled_build(dt, d, Lq):
    """(T, D, QB) of the attention_tiled_kernel instantiation a launch runs."""
    return IDS[dt], d, 1 if Lq <= 16 else 2


def test_the_pairs_cover_every_build():
    """The eight tiled builds and the three streaming builds each run under the per-element tests below, and both sides of the
    nk2 switch are crossed in a first and in a later tile by each."""
    tiled = {tiled_build(dt, d, Lq) for dt in SIXTEEN for d in HEAD_DIMS for Lq, _ in BUILD_PAIRS}
    assert tiled == {(t, D, QB) for t in ("fp16", "bf16") for D in (32, 64) for QB in (1, 2)}
    assert {IDS[dt] for dt, r in LONG_CASES if r == "stream"} == {"fp32", "fp16", "bf16"}
    for QB in (1, 2):
        lks = {Lk for Lq, Lk in BUILD_PAIRS if (Lq <= 16) == (QB == 1)}
        last = {(Lk - 1) % 64 + 1 for Lk in lks}                           # keys in the last tile
        assert any(n <= 32 for n in last) and any(n > 32 for n in last) and any(Lk > 64 for Lk in lks), QB
    assert {32, 33, 96, 97} <= {Lk for _, Lk in BUILD_PAIRS}
    for pair in OTHER_BH:
        assert pair in BUILD_PAIRS


def run_pair(dt, route, d, Lq, Lk):
    worst = 0.0
    for B, heads in [(3, 3)] + ([(1, 1), (2, 2)] if (Lq, Lk) in OTHER_BH else []):
        for masked in (True, False):
            worst = max(worst, per_element(dt, route, B, heads, Lq, Lk, d, masked))
    return worst


@pytest.mark.parametrize("dt", SIXTEEN, ids=[IDS[d] for d in SIXTEEN])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", BUILD_PAIRS)
def test_tiled_per_element_every_build(dt, d, Lq, Lk, monkeypatch):
    on_route("tiled", dt, monkeypatch)
    T_, D, QB = tiled_build(dt, d, Lq)
    w = run_pair(dt, "tiled", d, Lq, Lk)
    print(f"\n[attention_tiled_kernel<{T_}, {D}, {QB}> Lq {Lq} Lk {Lk}] worst ratio {w:.3f}", end="")


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", BUILD_PAIRS)
def test_stream_per_element_every_build(dt, d, Lq, Lk, monkeypatch):
    """fp32 as it routes, the 16-bit types with the matrix cores switched off."""
    on_route("stream", dt, monkeypatch)
    w = run_pair(dt, "stream", d, Lq, Lk)
    print(f"\n[attention_stream_kernel<{IDS[dt]}> d {d} Lq {Lq} Lk {Lk}] worst ratio {w:.3f}", end="")


# ---- 2. exact: row and head permutation across three key tiles ---------------------------------------------------------------
def permutation_three_tiles(dt, route, B, heads, Lq, d, a):
    """Lk = 150 and n = min(d, Lk) live columns: the key for column c < n sits at row pos(c) = 37 c mod 150 (37 and 150 are
    coprime: n different rows, spread over the three 64-key tiles) and equals a e_c; every other key is zero.  Query row r of head
    h is a e_c with c = (7 r + 3 h) mod n, v is random, there is no mask.  The matching key scores a^2 / sqrt(d) >= 128 and every
    other key 0, so the other weights are exactly 0 in expf and in the tiled kernel's exp2 form, whichever tile comes first (a
    tile before the matching one leaves a finite O that the rescale factor exp(-gap) = 0 clears), and l = 1:
    out[b, r, head h] is v[b, pos(c), head h] bit for bit."""
    Lk, td, H = 150, TDT[dt], heads * d
    n = min(d, Lk)
    assert a * a / np.sqrt(d) >= 128 and float(torch.tensor(float(a)).to(td)) == a
    pos = 37 * np.arange(n) % Lk
    assert len(set(pos.tolist())) == n and {int(p) // 64 for p in pos} == {0, 1, 2}
    col = (7 * np.arange(Lq)[:, None] + 3 * np.arange(heads)[None]) % n                       # [Lq, heads]
    gen = np.random.Generator(np.random.PCG64([d, Lq]))
    q = torch.zeros((B, Lq, heads, d), dtype=td)
    k = torch.zeros((B, Lk, heads, d), dtype=td)
    for h in range(heads):
        q[:, torch.arange(Lq), h, torch.from_numpy(col[:, h])] = a
        k[:, torch.from_numpy(pos), h, torch.arange(n)] = a
    v = torch.from_numpy(gen.standard_normal((B, Lk, heads, d)).astype(np.float32)).to(td)
    out = attention("vk_attention_tiled", q.view(B * Lq, H).to(G.DEV), k.view(B * Lk, H).to(G.DEV), v.view(B * Lk, H).to(G.DEV), None, B,
                    heads, Lq, Lk, d, dt, route)
    want = torch.stack([v[:, torch.from_numpy(pos[col[:, h]]), h] for h in range(heads)], 2)   # [B, Lq, heads, d]
    got = out.view(B, Lq, heads, d).cpu()
    wrong = [(b, r, h) for b in range(B) for r in range(Lq) for h in range(heads) if not same_bits(got[b, r, h], want[b, r, h])]
    assert not wrong, f"(batch, row, head) that do not return v[batch, pos, head]: {wrong[:8]}"


@pytest.mark.parametrize("dt,route", LONG_CASES, ids=LONG_IDS)
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("B,Lq", [(2, 50), (1, 13)])
def test_exact_permutation_three_key_tiles(dt, route, d, B, Lq, monkeypatch):
    """(2, 50): QB = 2, a last item of 18 rows; (1, 13): QB = 1, three items in a workgroup of four waves (one idle)."""
    on_route(route, dt, monkeypatch)
    permutation_three_tiles(dt, route, B, 3, Lq, d, 32)


# ---- 4. head dims to the contract's limits -----------------------------------------------------------------------------------
STREAM_DIMS = [(L.VK_F32, d) for d in (1, 3, 65, 100, 128, 255, 256)] + [(dt, d) for dt in SIXTEEN for d in (8, 72, 128, 256)]


@pytest.mark.parametrize("dt,d", STREAM_DIMS, ids=[f"{IDS[dt]}-{d}" for dt, d in STREAM_DIMS])
@pytest.mark.parametrize("Lq,Lk", [(17, 65), (33, 129)])
def test_stream_head_dims_per_element(dt, d, Lq, Lk, monkeypatch):
    """d = 256 is STR_MAXD: every one of a thread's 16 accumulators is live and the launch asks for 152 128 bytes of LDS."""
    on_route("stream", dt, monkeypatch)
    w = max(per_element(dt, "stream", 3, 2, Lq, Lk, d, masked) for masked in (True, False))
    print(f"\n[attention_stream_kernel<{IDS[dt]}> d {d} Lq {Lq} Lk {Lk}] worst ratio {w:.3f}", end="")


def test_stream_kernel_at_its_largest_head_dim_is_covered():
    assert {IDS[dt] for dt, d in STREAM_DIMS if d == 256} == {"fp32", "fp16", "bf16"}


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("d", [128, 256])
def test_stream_exact_permutation_wide_heads(dt, d, monkeypatch):
    """The three-tile permutation at d = 128 and 256, a = 64 (the gap a^2 / sqrt(d) is 362 and 256)."""
    on_route("stream", dt, monkeypatch)
    permutation_three_tiles(dt, "stream", 2, 3, 50, d, 64)


def test_lds_kernel_at_its_largest_image_127_127_64():
    """fp32 at (127, 127, 64): 163 576 of the 163 840 bytes the rule admits, on vk_attention."""
    lib = L.load()
    assert lib.vk_attention_route(127, 127, 64, L.VK_F32, 384, 384, 384, 1, 0) == L.VK_ATT_ROUTE_LDS
    for masked in (True, False):
        per_element(L.VK_F32, "lds", 3, 3, 127, 127, 64, masked)


def test_first_shape_past_the_lds_kernel_128_128_64():
    """One more token and vk_attention itself streams."""
    for masked in (True, False):
        per_element(L.VK_F32, "stream", 3, 3, 128, 128, 64, masked, entry="vk_attention")


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("d", [128, 256])
def test_lds_wide_heads_per_element(dt, d, monkeypatch):
    on_route("lds", dt, monkeypatch)
    for masked in (True, False):
        per_element(dt, "lds", 3, 3, 20, 36, d, masked)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
def test_lds_exact_permutation_d128(dt, monkeypatch):
    """test_gpu_attention_small's row / head permutation at Lk = d = 128 with a = 64 (at a = 32 the gap would be 90.5, where expf
    is not yet 0).  Lq = 31 is the longest the LDS kernel holds beside 128 keys of 128: 163 576 bytes again."""
    on_route("lds", dt, monkeypatch)
    B, heads, Lq, Lk, d, a, td = 2, 3, 31, 128, 128, 64, TDT[dt]
    H = heads * d
    assert a * a / np.sqrt(d) >= 128
    gen = np.random.Generator(np.random.PCG64(d))
    pi = (7 * np.arange(Lq)[:, None] + 3 * np.arange(heads)[None]) % Lk                        # [Lq, heads]
    q = torch.zeros((B, Lq, heads, d), dtype=td)
    k = torch.zeros((B, Lk, heads, d), dtype=td)
    for h in range(heads):
        q[:, torch.arange(Lq), h, torch.from_numpy(pi[:, h])] = a
        k[:, torch.arange(Lk), h, torch.arange(Lk)] = a
    v = torch.from_numpy(gen.standard_normal((B, Lk, heads, d)).astype(np.float32)).to(td)
    out = attention("vk_attention", q.view(B * Lq, H).to(G.DEV), k.view(B * Lk, H).to(G.DEV), v.view(B * Lk, H).to(G.DEV), None, B, heads,
                    Lq, Lk, d, dt, "lds")
    want = torch.stack([v[:, torch.from_numpy(pi[:, h]), h] for h in range(heads)], 2)        # [B, Lq, heads, d]
    got = out.view(B, Lq, heads, d).cpu()
    wrong = [(b, r, h) for b in range(B) for r in range(Lq) for h in range(heads) if not same_bits(got[b, r, h], want[b, r, h])]
    assert not wrong, f"(batch, row, head) that do not return v[batch, pi, head]: {wrong[:8]}"
