"""-m gpu: vk_linear's epilogues -- act(x . w^T + bias + residual), act = none / ReLU / GELU (erf) / tanh, to the storage type or
to fp32 -- per element against float64, on the generic kernel (csrc/conv_mfma.hip) and the two-per-CU kernel
(csrc/conv_mfma_duo.hip), whose bf16 GELU build is what the encoders' feed-forward runs on.

Dyadic data (tests/linear_util.py) makes the pre-activation the same fp32 number in every kernel: with act 0 / 1 the output must
have the BITS of the float64 value rounded once, with GELU and tanh it must lie within linear_bound (tests/transformer_check.py),
which is then the activation's own error and one rounding.  Random data, as the encoders see it, runs under the same bound with
the pre-activation's error term.  Every launch states its kernel (`expect_route=`; route_plan() below is asked of the dispatcher by
the CPU suite, tests/test_abi.py).  The store discipline -- nothing outside rows 0 .. M - 1 and columns 0 .. cout8 - 1 of y is
written, no residual row past M reaches an output -- is tested with sentinels, as tests/test_gpu_layernorm.py does."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
import linear_util as U                                # noqa: E402
import transformer_check as T                          # noqa: E402

IDS = {U.F32: "fp32", U.F16: "fp16", U.BF16: "bf16"}
SENTINEL = -77.0
REPORT = {}                                             # (dtype, out dtype, route, act, data) -> [worst ratio, launches, elements, bit-exact launches]
STORE_N = (2, 5, 72, 136)                               # cout8 = 8, 8, 72, 136: pads, the narrow and the wide column tile
STORE_PAD = (0, 8, 64)                                  # ldy - cout8
FRONT = 64                                              # elements in front of y (a multiple of 8: the stores are 16-byte chunks)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def store_case(dt, N):
    return U.Case("generic", 129, 768, N, 1, True, dt)


def route_plan():
    """(label, environment, gpu_util.conv_route arguments, kernel) of every launch of this module, for the CPU suite
    (tests/test_abi.py)."""
    for c in U.all_cases():
        yield c.name, {}, c.route_geometry(), c.route
    for dt in U.DTYPES:
        for N in STORE_N:
            c = store_case(dt, N)
            for pad in STORE_PAD:
                yield f"store-{c.name}-ldy+{pad}", {}, dict(c.route_geometry(), ldy=(N + 7) // 8 * 8 + pad), c.route


def launch(c, x, w, bias, res, pad=0, extra_rows=0, front=0):
    """One vk_linear launch of the case on CPU operands -> (y [M, N] on the CPU, the device x and res for the reference).  y lies
    in a [M + extra_rows, ldy] buffer, ldy = cout8 + pad, `front` elements into an allocation prefilled with the sentinel; the
    residual has y's row stride, zero pads, and 1e4 in the rows past M.  Everything but rows < M, columns < cout8 of y must keep
    its bits."""
    M, K = x.shape
    N = c.N
    td, od = U.TORCH_DT[c.dt], U.TORCH_DT[c.odt]
    cout8 = (N + 7) // 8 * 8
    ldy = cout8 + pad
    wp, bp = G.pack_conv(w.float().numpy().reshape(N, K, 1, 1), None, bias.numpy(), c.dt)
    xd = x.to(G.DEV)
    rd = rfull = None
    if res is not None:
        rfull = torch.zeros((M + extra_rows, ldy), dtype=td)
        rfull[:M, :N] = res
        rfull[M:] = 1e4
        rfull = rfull.to(G.DEV)
        rd = rfull[:M, :N]
    yf = torch.full((front + (M + extra_rows) * ldy,), SENTINEL, dtype=od)
    yd = yf.to(G.DEV)
    G.launch("vk_linear", G.P(xd), M, K, G.P(wp), G.P(bp), G.P(rfull), G.P(yd[front:]), N, ldy, c.act, c.dt, c.odt, G.stream(),
             expect_route=c.route)
    torch.cuda.synchronize()
    got = yd.cpu()
    assert torch.equal(bits(got[:front]), bits(yf[:front])), f"{c.name}: elements in front of y were written"
    y = got[front:].view(M + extra_rows, ldy)
    assert torch.equal(bits(y[M:]), bits(yf[front:].view(M + extra_rows, ldy)[M:])), f"{c.name}: rows of y past M were written"
    assert torch.equal(bits(y[:M, cout8:]), bits(torch.full((M, pad), SENTINEL, dtype=od))), f"{c.name}: columns of y past cout8 were written"
    return y[:M, :N], xd, rd


def check(c, **where):
    """Draw the case, assert the data conditions, launch, and hold every element to the bound (act 0 / 1 on exact data: to the bits).
    Returns the worst ratio."""
    x, w, bias, res = U.make_inputs(c)
    exact = c.data != "random"
    y, xd, rd = launch(c, x, w, bias, res, **where)
    r = T.linear_reference(xd, w, bias, rd, c.act, exact)           # the float64 GEMM on the device, everything after it on the host
    if exact:
        U.check_conditions(c, xd, w.to(G.DEV), bias.to(G.DEV), rd, r["z"])      # (its sum of magnitudes is a GEMM too: on the device)
    od = U.TORCH_DT[c.odt]
    wr = T.assert_within(y, r["ref"], T.linear_bound(r, od), c.name)
    rep = REPORT.setdefault((IDS[c.dt], IDS[c.odt], c.route, U.ACT_NAMES[c.act], "random" if not exact else "exact"), [0.0, 0, 0, 0])
    rep[0], rep[1], rep[2] = max(rep[0], wr), rep[1] + 1, rep[2] + y.numel()
    if exact and c.act <= 1:
        want = r["ref"].to(od)
        same = bits(y) == bits(want)
        assert bool(same.all()), f"{c.name}: {int((~same).sum())} of {same.numel()} outputs differ from float64 rounded once, first at " \
                                 f"{tuple(int(i) for i in (~same).nonzero()[0])}"
        rep[3] += 1
    return wr


# ---- 0. the one measured constant -----------------------------------------------------------------------------------------------
def test_math_library_allowance():
    """E_ERF / E_TANH of tests/transformer_check.py: fp32 erf and tanh ON THE DEVICE against float64 on the host, over z on the
    2^-7 grid of [-10, 10] (erf at fp32(z * 0.70710678f), the kernels' argument).  E is twice the worst error in ulps of the
    result, rounded up, at least 2; the figures are printed."""
    z = (torch.arange(-1280, 1281, dtype=torch.float64) * 2.0 ** -7).float()
    t = z * np.float32(0.70710678118654752)
    e_dev = torch.erf(t.to(G.DEV)).cpu()
    h_dev = torch.tanh(z.to(G.DEV)).cpu()
    worst_erf = T.ulp_error(e_dev, torch.erf(t.double()))
    worst_tanh = T.ulp_error(h_dev, torch.tanh(z.double()))
    print(f"\n[math library] erf worst {worst_erf:.3f} ulp (E_ERF {T.E_ERF}), tanh worst {worst_tanh:.3f} ulp (E_TANH {T.E_TANH})", end="")
    assert bool((h_dev[z.abs() >= 9.5].abs() == 1.0).all()), "fp32 tanh is not +-1 from 9.5 on"
    assert T.E_ERF >= max(2, math.ceil(2 * worst_erf)) and T.E_TANH >= max(2, math.ceil(2 * worst_tanh))


# ---- 1. the generic kernel's table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", range(4), ids=U.ACT_NAMES)
@pytest.mark.parametrize("dt", U.DTYPES, ids=[IDS[d] for d in U.DTYPES])
def test_generic_table(dt, act):
    """Nine launches: N over {2, 5, 7, 64, 72, 128, 136, 384}, M over {1, 127, 128, 129, 300}, one K-tile and K = 768, with and
    without the residual, the output in the storage type and (16-bit types) in fp32."""
    for c in U.generic_cases(dt, act):
        check(c)


# ---- 2. the two-per-CU kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [U.F16, U.BF16], ids=["fp16", "bf16"])
def test_duo_table(dt):
    """M over {1024, 1025, 1151, 2600}, N 256 / 768, K 64 (two stages, the minimum) to 3072; bf16 with act 0 / 1 / 2 (the GELU
    build), f16 with act 0 / 1; each with and without the residual."""
    cases = U.duo_cases(dt)
    assert all(c.route == "duo" for c in cases) and (dt != U.BF16 or sum(c.act == 2 for c in cases) >= 4)
    for c in cases:
        check(c)


@pytest.mark.parametrize("c", U.DUO_FALLBACK, ids=[c.name for c in U.DUO_FALLBACK])
def test_duo_geometry_falls_back_to_generic(c):
    """f16 GELU, tanh, and an fp32 output at the two-per-CU kernel's geometry: it has no such epilogue, the generic kernel takes the
    launch (asserted) and is right."""
    assert c.route == "generic" and G.conv_route(**dict(c.route_geometry(), relu=1, out_dt=c.dt)) == "duo"
    check(c)


@pytest.mark.parametrize("dt", U.DTYPES, ids=[IDS[d] for d in U.DTYPES])
def test_fine_data(dt):
    """z a multiple of 2^-12: more bits than fp16 keeps where the activations bend, so the one rounding of the output is exercised
    in fp16 as in bf16 -- to the bits with act 0 / 1 -- and a second rounding would show."""
    for c in U.fine_cases(dt):
        check(c)


# ---- 3. random data, as the encoders see it -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", U.DTYPES, ids=[IDS[d] for d in U.DTYPES])
def test_random_data(dt):
    """x ~ N(0, 1), w ~ N(0, 1 / K): two generic launches and the feed-forward pair 768 -> 3072 GELU, 3072 -> 768 + residual at 2600
    rows (16-bit types: on the two-per-CU kernel, the GELU in bf16 only)."""
    for c in U.random_cases(dt):
        check(c)


# ---- 4. what the launch leaves alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", STORE_N)
@pytest.mark.parametrize("dt", U.DTYPES, ids=[IDS[d] for d in U.DTYPES])
def test_store_discipline(dt, N):
    """Generic kernel, M = 129 (one row into the second row tile), ReLU + residual on dyadic data: y in a buffer of row stride
    cout8, cout8 + 8 and cout8 + 64 with 40 rows after M and 64 elements in front.  `launch` asserts that the columns from cout8 on,
    the rows from M on and the elements in front keep their bits; the residual's rows past M hold 1e4, and the outputs -- held to
    the bits here -- show none of it.  Columns cout .. cout8 - 1 are pads (include/vltk_hip.h): written, nothing asserted."""
    c = store_case(dt, N)
    for pad in STORE_PAD:
        check(c, pad=pad, extra_rows=40, front=FRONT)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_unknown_activation_is_refused_and_y_untouched():
    """act / relu outside 0 .. 3: VK_EINVAL from vk_linear and vk_conv2d before any launch, the same from vk_conv_route; y keeps
    its bytes.  The same launch with act 3 then writes it."""
    lib = L.load()
    M, K, N = 129, 64, 72
    x = torch.zeros((M, K), dtype=torch.float16, device=G.DEV)
    y = torch.full((M, N), SENTINEL, dtype=torch.float16, device=G.DEV)
    wp, bp = G.pack_conv(np.zeros((N, K, 1, 1), np.float32), None, np.ones(N, np.float32), L.VK_F16)
    for act in (4, -1, 255):
        args = (G.P(x), M, K, G.P(wp), G.P(bp), None, G.P(y), N, N, act, L.VK_F16, L.VK_F16, G.stream())
        assert lib.vk_linear(*args) == L.VK_EINVAL
        with pytest.raises(ValueError, match="activation"):
            L.call("vk_linear", *args)
        conv = (G.P(x), 1, 1, M, K, G.P(wp), G.P(bp), None, G.P(y), N, N, 1, 1, 1, 0, 1, 1, act, L.VK_F16, L.VK_F16, G.stream())
        assert lib.vk_conv2d(*conv) == L.VK_EINVAL
        with pytest.raises(ValueError, match="activation"):
            G.conv_route(1, 1, M, K, N, relu=act)
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL))
    G.launch("vk_linear", G.P(x), M, K, G.P(wp), G.P(bp), None, G.P(y), N, N, 3, L.VK_F16, L.VK_F16, G.stream(), expect_route="generic")
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, math.tanh(1.0)))


def test_zz_report(capsys):
    """Not a check of its own: prints, once, the worst |out - ref| / bound per dtype, kernel and activation of the launches above."""
    with capsys.disabled():
        print("\n[linear] dtype -> out, kernel, act, data: worst |out - ref| / bound, launches, elements, launches held to the bits")
        for k in sorted(REPORT):
            w, n, el, ex = REPORT[k]
            print(f"[linear]   {k[0]:>4s} -> {k[1]:4s} {k[2]:8s} {k[3]:5s} {k[4]:6s} {w:6.3f} {n:4d} {el:10d} {ex:4d}")
    if any(k[2] == "duo" for k in REPORT):              # (a run of this test alone has nothing to report)
        assert any(k[0] == "bf16" and k[2] == "duo" and k[3] == "gelu" and k[4] == "exact" for k in REPORT), "no two-per-CU bf16 GELU line"
