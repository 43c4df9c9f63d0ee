"""-m gpu: the two small-sequence attention kernels, attention_mfma_kernel (matrix cores, Lq <= 48, Lk <= 64) and attention_kernel
(LDS), which run LXMERT at 20 text and 36 visual tokens, and the per-element metric on the tiled and streaming kernels' 16-bit
builds.

1. every output element against a float64 reference, within the bound of tests/transformer_check.py, with Lq and Lk walked across
   the 16- and 32-element block edges, every dtype, both staging branches of the LDS kernel, idle waves in the last workgroup;
2. - 4. bit-exact: the uniform average (the key index through the P and V^T images), one-hot over every key, and a row / head
   permutation (the row mapping qb*16 + 4g + e and the head offset);
5. the output's surroundings: nothing written outside [B*Lq, H], two launches give the same bytes; the tiled and streaming
   kernels too, at lengths whose last query block is mostly padding rows.

tests/test_gpu_attention_builds.py holds every build of the tiled and streaming kernels, and the head dims up to the limits, to 1. - 4.

Every launch goes through vk_attention / vk_attention_tiled, with the route asked of vk_attention_route immediately before it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
import transformer_check as T                          # noqa: E402
from test_gpu_attention_long import ALL, FMIN, IDS, ROUTES, attention, mixed_mask      # noqa: E402
from test_gpu_lxmert import TDT                        # noqa: E402

SIXTEEN = [L.VK_F16, L.VK_BF16]
PAIRS = [(1, 1), (1, 64), (15, 17), (16, 16), (17, 15), (32, 33), (33, 31), (47, 49), (48, 64), (48, 63), (20, 36), (36, 20)]
LDS_PAIRS = PAIRS + [(49, 20), (50, 100)]
OTHER_BH = {"mfma": [(20, 36), (48, 64)], "lds": [(20, 36), (50, 100)]}       # the pairs that also run at (B, heads) = (1, 1), (2, 4)


def on_route(route, dt, monkeypatch):
    """The environment under which a 16-bit call reaches `route` (fp32 reaches the LDS and streaming kernels by itself)."""
    if route in ("lds", "stream") and dt != L.VK_F32:
        monkeypatch.setenv("VK_ATTENTION_MFMA", "0")
    else:
        monkeypatch.delenv("VK_ATTENTION_MFMA", raising=False)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def per_element(dt, route, B, heads, Lq, Lk, d, masked, extra=0, entry=None):
    """One launch on column slices of fused projections [rows, 2H + extra] (q the second half of its own buffer, k and v the
    halves of theirs), every element against float64 -> the worst ratio.  `entry`: the entry point, where it is not the route's
    usual one (vk_attention reaches the streaming kernel by itself past the LDS kernel's image)."""
    td, H = TDT[dt], heads * d
    gen = np.random.Generator(np.random.PCG64([Lq, Lk, d, B, heads, extra]))
    qq = torch.from_numpy(gen.standard_normal((B * Lq, 2 * H + extra)).astype(np.float32)).to(td)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H + extra)).astype(np.float32)).to(td)
    add = mixed_mask(B, Lk) if masked else None
    qd, kvd = qq.to(G.DEV), kv.to(G.DEV)
    entry = entry or ("vk_attention_tiled" if route in ("tiled", "stream") else "vk_attention")
    out = attention(entry, qd[:, H:2 * H], kvd[:, :H], kvd[:, H:2 * H], add.to(G.DEV) if masked else None, B, heads, Lq, Lk, d, dt, route)
    r = T.attention_reference(qq[:, H:2 * H], kv[:, :H], kv[:, H:2 * H], add, B, heads, Lq, Lk, d)
    return T.assert_within(out, r["ref"], T.attention_bound(r, td, route),
                           f"attention {route} {IDS[dt]} B {B} heads {heads} Lq {Lq} Lk {Lk} d {d} {'masked' if masked else 'plain'}"
                           + (f" ld +{extra}" if extra else ""))


# ---- 1. per element against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", SIXTEEN, ids=[IDS[d] for d in SIXTEEN])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_mfma_per_element(dt, d, Lq, Lk, monkeypatch):
    """(3, 3): nine (batch, head) pairs, three idle waves in the last workgroup; (1, 1); (2, 4): no idle wave."""
    on_route("mfma", dt, monkeypatch)
    for B, heads in [(3, 3)] + ([(1, 1), (2, 4)] if (Lq, Lk) in OTHER_BH["mfma"] else []):
        for masked in (True, False):
            per_element(dt, "mfma", B, heads, Lq, Lk, d, masked)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("Lq,Lk", LDS_PAIRS)
def test_lds_per_element(dt, d, Lq, Lk, monkeypatch):
    on_route("lds", dt, monkeypatch)
    for B, heads in [(3, 3)] + ([(1, 1), (2, 4)] if (Lq, Lk) in OTHER_BH["lds"] else []):
        for masked in (True, False):
            per_element(dt, "lds", B, heads, Lq, Lk, d, masked)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("d,extra", [(20, 0), (64, 2)])
def test_lds_scalar_staging_per_element(dt, d, extra, monkeypatch):
    """The LDS kernel's element-by-element staging: a head dim that is no whole number of 16-byte vectors (d = 20 in a 16-bit type;
    fp32 takes the vector branch there), and rows whose stride is no multiple of a vector (2H + 2 elements, every type)."""
    on_route("lds", dt, monkeypatch)
    for Lq, Lk in ((20, 36), (33, 31)):
        for masked in (True, False):
            per_element(dt, "lds", 3, 3, Lq, Lk, d, masked, extra)


LONG_CASES = [(dt, r) for dt in ALL for r in ("tiled", "stream") if not (r == "tiled" and dt == L.VK_F32)]     # no fp32 tiled build


@pytest.mark.parametrize("dt,route", LONG_CASES, ids=[f"{IDS[dt]}-{r}" for dt, r in LONG_CASES])
@pytest.mark.parametrize("Lq,Lk", [(17, 65), (33, 129)])
def test_tiled_and_stream_per_element(dt, route, Lq, Lk, monkeypatch):
    on_route(route, dt, monkeypatch)
    for masked in (True, False):
        per_element(dt, route, 3, 3, Lq, Lk, 64, masked)


# ---- 2. exact: the uniform average -----------------------------------------------------------------------------------------
def live_sets(Lk, counts_lead, counts_alt):
    """[(name, live keys)]: the last n keys live (a leading block masked), keys 0, 2, .. 2(n - 1) live (every other key masked),
    every key masked (the soft-max of equal scores: uniform over Lk) and no key masked."""
    idx = np.arange(Lk)
    sets = [(f"last {n}", idx >= Lk - n, False) for n in counts_lead if n < Lk]
    sets += [(f"even {n}", (idx % 2 == 0) & (idx < 2 * n), False) for n in counts_alt if 2 * n - 1 <= Lk]
    return sets + [("all masked", np.ones(Lk, bool), True), ("none masked", np.ones(Lk, bool), False)]


def uniform_case(dt, route, Lk, d, sets):
    """One batch per live set, q = 0, integer v -> (out [B, Lq, H], the integer column sums S [B, H] as fp32, the counts n [B])."""
    B, heads, Lq, td = len(sets), 3, 33, TDT[dt]
    H = heads * d
    gen = np.random.Generator(np.random.PCG64(Lk + d))
    q = torch.zeros((B * Lq, H), dtype=td, device=G.DEV)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H)).astype(np.float32)).to(td)
    vi = torch.from_numpy(gen.integers(-8, 9, (B, Lk, H)).astype(np.float32))
    kv[:, H:] = vi.view(B * Lk, H).to(td)
    add = np.zeros((B, Lk), np.float32)
    for b, (_, live, everything) in enumerate(sets):
        add[b] = FMIN if everything else np.where(live, 0.0, FMIN)
    kvd = kv.to(G.DEV)
    out = attention("vk_attention", q, kvd[:, :H], kvd[:, H:], torch.from_numpy(add).to(G.DEV), B, heads, Lq, Lk, d, dt, route)
    S = torch.stack([vi[b][torch.from_numpy(live)].sum(0) for b, (_, live, _) in enumerate(sets)])
    return out.view(B, Lq, H).cpu(), S, [int(live.sum()) for _, live, _ in sets]


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("Lk", [37, 50, 64])
@pytest.mark.parametrize("d", [32, 64])
def test_exact_uniform_average_lds(dt, Lk, d, monkeypatch):
    """n a power of two: 1 / n and every partial sum of p v are exact in fp32, so the output is S / n rounded once."""
    on_route("lds", dt, monkeypatch)
    sets = [s for s in live_sets(Lk, [1, 2, 4, 8, 16, 32], [2, 16, 32]) if int(s[1].sum()) & (int(s[1].sum()) - 1) == 0]
    assert len(sets) >= 7
    out, S, ns = uniform_case(dt, "lds", Lk, d, sets)
    for b, n in enumerate(ns):
        want = (S[b] / np.float32(n)).to(TDT[dt])
        assert same_bits(out[b], want[None].expand_as(out[b])), (sets[b][0], n)


@pytest.mark.parametrize("dt", SIXTEEN, ids=[IDS[d] for d in SIXTEEN])
@pytest.mark.parametrize("Lk", [37, 50, 64])
@pytest.mark.parametrize("d", [32, 64])
def test_exact_uniform_average_mfma(dt, Lk, d, monkeypatch):
    """Any n: every live p is round_T(fp32(1 / n)), at most 11 bits, and S at most 10, so p S is exact in fp32 in any order and the
    output is that product rounded once.  The counts are chosen so that round_T does not hang on the division's last bit."""
    on_route("mfma", dt, monkeypatch)
    td = TDT[dt]
    sets = live_sets(Lk, [1, 3, 5, 7, 19, 32], [2, 3, 19, 25])
    out, S, ns = uniform_case(dt, "mfma", Lk, d, sets)
    assert {n for n in ns if n & (n - 1)} and max(ns) == Lk
    for b, n in enumerate(ns):
        inv = np.float32(1.0) / np.float32(n)
        p = torch.tensor([np.nextafter(inv, np.float32(0)), inv, np.nextafter(inv, np.float32(1))]).to(td)
        assert p[0] == p[1] == p[2], f"round(1 / {n}) depends on the division's last bit: choose another count"
        want = (p[1].float() * S[b]).to(td)
        assert same_bits(out[b], want[None].expand_as(out[b])), (sets[b][0], n)


# ---- 3. exact: one-hot over every key --------------------------------------------------------------------------------------
def route_cases(dts=ALL):
    return [(dt, r) for dt in dts for r in ("mfma", "lds") if not (r == "mfma" and dt == L.VK_F32)]


ROUTE_CASES = route_cases()
ROUTE_IDS = [f"{IDS[dt]}-{r}" for dt, r in ROUTE_CASES]


@pytest.mark.parametrize("dt,route", ROUTE_CASES, ids=ROUTE_IDS)
@pytest.mark.parametrize("Lk", [37, 64])
@pytest.mark.parametrize("d", [32, 64])
def test_exact_one_hot_every_key(dt, route, Lk, d, monkeypatch):
    """Batch j: q = 32 e0, k[j] = 32 e0, every other key 0.  The scaled gap is 1024 / sqrt(d) >= 128, past the 104 at which fp32's exp
    is 0: the weights are one-hot exactly and every output row of batch j is v[j] bit for bit."""
    on_route(route, dt, monkeypatch)
    B, Lq, td = Lk, 3, TDT[dt]
    gen = np.random.Generator(np.random.PCG64(Lk + d))
    q = torch.zeros((B * Lq, d), dtype=td)
    q[:, 0] = 32
    k = torch.zeros((B, Lk, d), dtype=td)
    k[torch.arange(B), torch.arange(Lk), 0] = 32
    v = torch.from_numpy(gen.standard_normal((B, Lk, d)).astype(np.float32)).to(td)
    out = attention("vk_attention", q.to(G.DEV), k.view(B * Lk, d).to(G.DEV), v.view(B * Lk, d).to(G.DEV), None, B, 1, Lq, Lk, d, dt, route)
    want = v[torch.arange(B), torch.arange(Lk)][:, None, :].expand(B, Lq, d)
    got = out.view(B, Lq, d).cpu()
    wrong = [j for j in range(B) if not same_bits(got[j], want[j])]
    assert not wrong, f"keys whose batch does not return v[key]: {wrong}"


# ---- 4. exact: row and head permutation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,route", ROUTE_CASES, ids=ROUTE_IDS)
@pytest.mark.parametrize("d", [32, 64])
def test_exact_row_and_head_permutation(dt, route, d, monkeypatch):
    """Lk = d and k_j = 32 e_j in every head; query row r of head h is 32 e_pi with pi = (7 r + 3 h) mod Lk, so out[b, r, head h] is
    v[b, pi, head h] bit for bit: a wrong row, a wrong head offset or a wrong batch returns another v."""
    on_route(route, dt, monkeypatch)
    B, heads, Lk, td = 2, 3, d, TDT[dt]
    Lq = 48 if route == "mfma" else 50
    H = heads * d
    gen = np.random.Generator(np.random.PCG64(d))
    pi = (7 * np.arange(Lq)[:, None] + 3 * np.arange(heads)[None]) % Lk                        # [Lq, heads]
    q = torch.zeros((B, Lq, heads, d), dtype=td)
    k = torch.zeros((B, Lk, heads, d), dtype=td)
    for h in range(heads):
        q[:, torch.arange(Lq), h, torch.from_numpy(pi[:, h])] = 32
        k[:, torch.arange(Lk), h, torch.arange(Lk)] = 32
    v = torch.from_numpy(gen.standard_normal((B, Lk, heads, d)).astype(np.float32)).to(td)
    out = attention("vk_attention", q.view(B * Lq, H).to(G.DEV), k.view(B * Lk, H).to(G.DEV), v.view(B * Lk, H).to(G.DEV), None, B, heads,
                    Lq, Lk, d, dt, route)
    want = torch.stack([v[:, torch.from_numpy(pi[:, h]), h] for h in range(heads)], 2)        # [B, Lq, heads, d]
    got = out.view(B, Lq, heads, d).cpu()
    wrong = [(b, r, h) for b in range(B) for r in range(Lq) for h in range(heads) if not same_bits(got[b, r, h], want[b, r, h])]
    assert not wrong, f"(batch, row, head) that do not return v[batch, pi, head]: {wrong[:8]}"


# ---- 5. the output's surroundings -------------------------------------------------------------------------------------------
def surroundings(dt, route, entry, Lq, Lk):
    """out is [B*Lq + 1, H + 8], prefilled with a finite sentinel: the 8 columns past H and the row past the last hold it bit for
    bit after the launch, the rest is within the bound, and a second launch of the same arguments gives the same bytes."""
    B, heads, d, td = 3, 3, 64, TDT[dt]
    H, lib = heads * d, L.load()
    gen = np.random.Generator(np.random.PCG64(11))
    qq = torch.from_numpy(gen.standard_normal((B * Lq, 2 * H)).astype(np.float32)).to(td)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H)).astype(np.float32)).to(td)
    add = mixed_mask(B, Lk)
    qd, kvd, md = qq.to(G.DEV), kv.to(G.DEV), add.to(G.DEV)
    q, k, v = qd[:, H:], kvd[:, :H], kvd[:, H:]
    outs = []
    for _ in range(2):
        out = torch.full((B * Lq + 1, H + 8), -77.0, dtype=td, device=G.DEV)
        aligned = int((q.data_ptr() | k.data_ptr() | v.data_ptr()) % 16 == 0)
        got = lib.vk_attention_route(Lq, Lk, d, dt, q.stride(0), k.stride(0), v.stride(0), aligned, int(entry == "vk_attention_tiled"))
        assert got >= 0 and ROUTES[got] == route
        L.call(entry, G.P(q), q.stride(0), G.P(k), k.stride(0), G.P(v), v.stride(0), G.P(md), G.P(out), H + 8, B, heads, Lq, Lk, d,
               dt, G.stream())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    sentinel = torch.full((1,), -77.0, dtype=td)
    assert same_bits(outs[0][:-1, H:], sentinel.expand(B * Lq, 8)) and same_bits(outs[0][-1], sentinel.expand(H + 8))
    assert same_bits(outs[0], outs[1])
    r = T.attention_reference(qq[:, H:], kv[:, :H], kv[:, H:], add, B, heads, Lq, Lk, d)
    T.assert_within(outs[0][:-1, :H], r["ref"], T.attention_bound(r, td, route), f"attention {route} {IDS[dt]} Lq {Lq} Lk {Lk} into a wider out")


@pytest.mark.parametrize("dt,route", ROUTE_CASES, ids=ROUTE_IDS)
def test_output_surroundings_and_repeatability(dt, route, monkeypatch):
    on_route(route, dt, monkeypatch)
    surroundings(dt, route, "vk_attention", 36, 20)


@pytest.mark.parametrize("dt,route", LONG_CASES, ids=[f"{IDS[dt]}-{r}" for dt, r in LONG_CASES])
@pytest.mark.parametrize("Lq", [36, 17])
def test_output_surroundings_and_repeatability_long(dt, route, Lq, monkeypatch):
    """The same around the tiled and streaming kernels, two key tiles (Lk = 70).  Lq = 36: the last query block (rows 32 .. 35 of
    the tiled kernel's 32, rows 32 .. 35 of the streaming kernel's 16) is mostly padding rows, whose stores would land in the next
    batch's rows or, for the last batch, in the guard row; Lq = 17: a last block of one live row."""
    on_route(route, dt, monkeypatch)
    surroundings(dt, route, "vk_attention_tiled", Lq, 70)
