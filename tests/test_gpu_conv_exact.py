"""-m gpu: every convolution kernel and form on integer data, bit for bit against float64 arithmetic rounded once.

tests/exact_util.py makes the data (activations 0..15, weights -8..8, integer bias levels that spread the channels over the
f16 binades, integer residual) and states why the result does not depend on MFMA, K order, tile shape or wave split: every
partial sum is an integer below 2^24.  The expected tensor is the float64 convolution (torch, on the device) + bias +
residual, ReLU, ONE round-to-nearest-even to the storage type; the assertion is torch.equal on the whole tensor and "no
NaN".  A truncating store, a residual added after the rounding, a bias applied in f16, a flushed subnormal, an overflow
clamped instead of becoming inf, or an error that only hits outputs small against the tensor's maximum all fail here; the
max-normalised 1e-3 of the parity tests admits each of them.

Every case names the kernel it must run on and the switches that pin it (asserted immediately before the launch, and on the
CPU by tests/test_abi.py through `route_plan`); the shapes are those of tests/test_gpu_stages.py's tables, which encode
where each kernel's edges are.  tests/test_conv_exact_host.py proves the data's conditions for the whole table on the CPU.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                 # noqa: E402

import exact_util as X                         # noqa: E402
import gpu_util as G                           # noqa: E402
import test_gpu_stages as S                    # noqa: E402
from exact_util import Case                    # noqa: E402

F32, F16, BF16 = L.VK_F32, L.VK_F16, L.VK_BF16
OFF = {"ws": ("VK_CONV_WS", "0"), "gemm4": ("VK_CONV_GEMM4", "0"), "duo": ("VK_CONV_DUO", "0"), "panel": ("VK_CONV3X3_PANEL", "0"),
       "blk": ("VK_CONV3X3_BLK", "0"), "ring2": ("VK_CONV256_DUAL", "0")}


def _env(*off, **kw):
    return tuple(OFF[o] for o in off) + tuple(kw.items())


PIN_RING = _env("ws", "gemm4", "duo", "panel")
PIN_DUO = _env("ws", "gemm4") + (("VK_CONV_DUO", "1"),)
GEMM4_ANY = (("VK_CONV_GEMM4", "2"),)                       # the four-wave GEMM also on grids below its floor


def _conv(name, route, shape, env=(), **kw):
    """A Case from a row of test_gpu_stages.CONV_CASES."""
    _, N, H, W, cin, cout, k, stride, pad, dil, res, relu = shape
    return Case(name, route, "conv", N, H, W, cin, cout, k, stride, pad, dil, res=res, relu=int(relu), env=env, **kw)


def _flat(name, route, M, cin, cout, env=(), kind="conv", **kw):
    return Case(name, route, kind, 1, 1, M, cin, cout, env=env, **kw)


def _table():
    cc = {c[0]: c for c in S.CONV_CASES}
    t = []
    # ---- generic (conv_mfma_kernel): fp32 exact-f32 MFMA; f16 128- and 64-wide column tiles; f16 -> f32 out, 75 channels; bf16;
    # grouped as slice-diagonal GEMMs; (its stem form: test_stem_exact)
    for n in ("1x1", "3x3", "3x3_s2", "3x3_dil2", "1x1_res", "1x1_narrow"):
        t.append(_conv(f"generic/f32/{n}", "generic", cc[n], dt=F32))
    for n in ("1x1", "1x1_narrow", "1x1_s2", "3x3_wide", "3x3_dil2", "1x1_res", "3x3_s2"):
        t.append(_conv(f"generic/f16/{n}", "generic", cc[n]))
    t.append(Case("generic/f16_f32out_c75", "generic", "conv", 2, 9, 13, 128, 75, out_dt=F32))
    t.append(_flat("generic/bf16/linear_640", "generic", 640, 128, 384, kind="linear", relu=1, res=True, dt=BF16))
    t.append(_flat("generic/bf16/linear_77", "generic", 77, 128, 128, kind="linear", dt=BF16))
    t.append(_flat("generic/f16/linear_108", "generic", 108, 768, 256, kind="linear", res=True))
    for n, N, H, W, c, groups, stride, dil in S.GROUPED_CASES:
        t.append(Case(f"generic/grouped/{n}", "generic", "conv", N, H, W, c, c, 3, stride, dil, dil, groups, relu=1, env=_env("blk")))
    # ---- ring (conv_mfma256_kernel): K-ring lengths 2, 4, 6, 16, 18, 36; 3x3, dilation 2, stride 2; two inputs with K >= 1024
    for n in ("ring_s2", "ring_s4", "ring_s6", "ring_1x1_k512", "ring_3x3", "ring_3x3_dil2", "ring_1x1_s2"):
        t.append(_conv(f"ring/{n}", "ring", cc[n], PIN_RING))
    t.append(_flat("ring/dual_512_1024", "ring", 4000, 512, 512, _env("ws", "gemm4"), "dual", cin2=1024, relu=1))
    t.append(_flat("ring/dual_256_768_res", "ring", 1030, 256, 256, _env("ws", "gemm4"), "dual", cin2=768, relu=1, res=True))
    # ---- duo (conv_duo_kernel): stage counts 2, 4, 6, 10, 16; stride 2; two inputs; the bf16 build through vk_linear
    for n in ("duo_s2", "duo_s4", "duo_s6", "duo_s10", "duo_s16", "duo_s2_stride2"):
        t.append(_conv(f"duo/{n}", "duo", cc[n], PIN_DUO))
    t.append(_flat("duo/dual_128_192_res", "duo", 2600, 128, 256, (), "dual", cin2=192, relu=1, res=True))
    t.append(_flat("duo/dual_128_256_small", "duo", 130, 128, 256, (), "dual", cin2=256, relu=1, res=True))
    t.append(_flat("duo/dual_512_1024", "duo", 2500, 512, 2048, _env("ws", "gemm4", "ring2"), "dual", cin2=1024, relu=1))
    t.append(_flat("duo/bf16/ffn_up_relu", "duo", 2600, 768, 3072, (), "linear", relu=1, dt=BF16))
    t.append(_flat("duo/bf16/ffn_down_res", "duo", 2600, 3072, 768, (), "linear", res=True, dt=BF16))
    t.append(_flat("duo/bf16/relu_res", "duo", 1024, 768, 768, (), "linear", relu=1, res=True, dt=BF16))
    t.append(_flat("duo/bf16/plain", "duo", 1100, 256, 512, (), "linear", dt=BF16))
    t.append(_flat("duo/f16/ffn_down_res", "duo", 2600, 3072, 768, (), "linear", res=True))
    # ---- ws (conv_ws_kernel): K = 64 / 128 / 256 / 512; 8 and 4 waves; stride 2 and 3; 64 + 64 channels; ragged last tiles
    for i, ((N, H, W), cin, cout, res) in enumerate(S.WS_CASES):
        t.append(Case(f"ws/k{cin}_{cout}_{N}x{H}x{W}", "ws", "conv", N, H, W, cin, cout, res=res, relu=1))
    t.append(Case("ws/k128_waves4", "ws", "conv", 3, 37, 41, 128, 512, res=True, relu=1, env=(("VK_WS_WAVES", "4"),)))
    t.append(Case("ws/k512_waves4", "ws", "conv", 1, 32, 33, 512, 256, res=True, relu=1, env=(("VK_WS_WAVES", "4"),)))
    t.append(Case("ws/stride2_512", "ws", "conv", 2, 51, 85, 512, 256, stride=2, relu=1))
    t.append(Case("ws/stride2_256", "ws", "conv", 3, 100, 167, 256, 512, stride=2))
    t.append(Case("ws/stride3_256", "ws", "conv", 4, 67, 40, 256, 256, stride=3, relu=1))
    t.append(_flat("ws/dual_64_64", "ws", 1500, 64, 256, (), "dual", cin2=64, relu=1))
    t.append(_flat("ws/dual_64_64_res", "ws", 9000, 64, 512, (), "dual", cin2=64, relu=1, res=True))
    # ---- gemm4 (conv_gemm4_kernel): K = 1024 / 1152 / 2048; 512 + 1024; ragged tiles; several tiles per workgroup; the dynamic
    # tail on and off; rows past the descriptor's 14-bit stride
    for (N, H, W), cin, cout, res, relu in S.GEMM4_CASES:
        t.append(Case(f"gemm4/k{cin}_{cout}_{N}x{H}x{W}", "gemm4", "conv", N, H, W, cin, cout, res=res, relu=int(relu), env=GEMM4_ANY))
    t.append(_flat("gemm4/dual_512_1024", "gemm4", 4000, 512, 512, GEMM4_ANY, "dual", cin2=1024, relu=1))
    t.append(_flat("gemm4/many_k2048", "gemm4", 40000, 2048, 512, GEMM4_ANY, relu=1))
    t.append(_flat("gemm4/many_dual", "gemm4", 39917, 512, 2048, GEMM4_ANY, "dual", cin2=1024, relu=1))
    t.append(_flat("gemm4/many_k2048_res", "gemm4", 33000, 2048, 2048, GEMM4_ANY, relu=1, res=True))
    t.append(_flat("gemm4/row_12544", "gemm4", 32000, 12544, 1024, GEMM4_ANY, relu=1))
    t.append(_flat("gemm4/row_16512", "gemm4", 2100, 16512, 256, GEMM4_ANY))
    t.append(Case("gemm4/tail_dynamic", "gemm4", "conv", 5400, 14, 14, 1024, 512, relu=1))
    t.append(Case("gemm4/tail_static", "gemm4", "conv", 5400, 14, 14, 1024, 512, relu=1, env=(("VK_GEMM4_DYNAMIC", "0"),),
                  seed_name="gemm4/tail_dynamic"))
    # ---- panel (conv3x3_panel_kernel): halo 64 and 128; 8 and 9 row tiles; M < one tile; 84- and 100-wide maps; the res4 map;
    # RoI-shaped 14 x 14 with dilation 2 and an image count that is not a multiple of the tile; the dynamic tail on and off
    for n in ("panel_head", "panel_head_res", "panel_d1", "panel_wide", "panel_wide_d1", "panel_tiny", "panel_res4"):
        t.append(_conv(f"panel/{n}", "panel", cc[n]))
    for mi in ("8", "9"):
        for n in ("panel_head_res", "panel_d1", "panel_res4"):
            t.append(_conv(f"panel/{n}_mi{mi}", "panel", cc[n], (("VK_PANEL_MI", mi),), seed_name=f"panel/{n}"))
    t.append(Case("panel/tail_dynamic", "panel", "conv", 5400, 14, 14, 512, 512, 3, 1, 2, 2, relu=1))
    t.append(Case("panel/tail_static", "panel", "conv", 5400, 14, 14, 512, 512, 3, 1, 2, 2, relu=1, env=(("VK_PANEL_DYNAMIC", "0"),),
                  seed_name="panel/tail_dynamic"))
    # ---- blk (conv3x3_blk_kernel): its four variants (32- / 64-channel blocks x dilation 1 / 2), ragged edges, a tiny image
    for n, N, H, W, c, groups, dil in S.BLK_CASES:
        t.append(Case(f"blk/{n}", "blk", "conv", N, H, W, c, c, 3, 1, dil, dil, groups, relu=int(c != 128)))
    # ---- the fused mean: fp64 sums per image on ws, integer partials per tile on duo
    for N, HW, cin, cout in ((23, 196, 512, 512), (9, 130, 512, 256)):
        t.append(Case(f"mean/ws/{N}x{HW}_{cin}_{cout}", "ws", "mean", N, 1, HW, cin, cout, res=True, relu=1))
    for N, HW, cin, cout in ((7, 196, 128, 256), (3, 255, 64, 256), (40, 130, 256, 1024), (1, 128, 64, 256)):
        t.append(Case(f"mean/duo/{N}x{HW}_{cin}_{cout}", "duo", "mean", N, 1, HW, cin, cout, res=True, relu=1))
    t.append(Case("mean/duo/23x196_512_512", "duo", "mean", 23, 1, 196, 512, 512, res=True, relu=1, env=_env("ws"),
                  seed_name="mean/ws/23x196_512_512"))
    # ---- three edge cases per epilogue: overflow to +-inf, subnormal results, one large activation beside small ones
    edge_shapes = [_conv("generic", "generic", cc["1x1"]), _conv("generic_norelu", "generic", cc["1x1_s2"]),
                   _conv("ring", "ring", cc["ring_s4"], PIN_RING), _conv("duo", "duo", cc["duo_s4"], PIN_DUO),
                   Case("ws", "ws", "conv", 3, 37, 41, 128, 512, res=True, relu=1),
                   Case("gemm4", "gemm4", "conv", 11, 14, 14, 1024, 512, relu=1, env=GEMM4_ANY),
                   Case("gemm4_norelu", "gemm4", "conv", 1, 45, 47, 1152, 512, res=True, env=GEMM4_ANY),
                   _conv("panel", "panel", cc["panel_head_res"]), _conv("blk", "blk", cc["3x3"]),
                   Case("blk_norelu", "blk", "conv", 5, 14, 14, 128, 128, 3, 1, 2, 2, 4),
                   # -inf needs a layer without the ReLU: one more overflow leg for the other four epilogues
                   _conv("ring_norelu", "ring", cc["ring_s2"], PIN_RING), _conv("duo_norelu", "duo", cc["duo_s2"], PIN_DUO),
                   Case("ws_norelu", "ws", "conv", 3, 100, 167, 256, 512, stride=2), _conv("panel_norelu", "panel", cc["panel_wide"])]
    for base in edge_shapes:
        for edge in X.EDGES[1:]:
            if base.name.endswith("_norelu") and edge != "overflow":
                continue
            t.append(dataclasses.replace(base, name=f"edge/{edge}/{base.name}", edge=edge))
    assert len({c.name for c in t}) == len(t)
    return t


EXACT_CASES = _table()


def route_plan():
    """(label, environment, gpu_util.conv_route arguments, kernel) of every case, for the CPU suite (tests/test_abi.py)."""
    for c in EXACT_CASES:
        yield c.name, dict(c.env), c.route_geometry(), c.route


REPORT = {}                                                 # route -> [cases, output elements compared]


def _rows(t):
    """[N, C, H, W] float64 -> [N*H*W, C] (the kernels' NHWC rows)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _pack(c, w, bias):
    """Packed weights and bias on the device; the two-input form: [first input's row | second input's row] per output channel."""
    wn, bn = w.numpy().astype(np.float32), bias.numpy().astype(np.float32)
    if not c.cin2:
        return G.pack_conv(wn, None, bn, c.dt, c.groups)
    p1, b1 = G.pack_conv(np.ascontiguousarray(wn[:, :c.cin]), None, bn, c.dt)
    p2, _ = G.pack_conv(np.ascontiguousarray(wn[:, c.cin:]), None, None, c.dt)
    rows = b1.numel()
    return torch.cat([p1.view(rows, c.cin * 2), p2.view(rows, c.cin2 * 2)], dim=1).contiguous(), b1


def run_case(c, monkeypatch):
    """Generate, check the data's conditions, launch on the named kernel, compare whole tensors; returns (got, expected)."""
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    td, tod = X.TORCH_DT[c.dt], X.TORCH_DT[c.odt]
    x, w, bias, res = X.make_inputs(c, G.DEV)
    v, want = X.expected(c, x, w, bias, res)
    X.check_conditions(c, x, w, bias, res, v, want)
    del v
    wd, bd = _pack(c, w, bias)
    ho, wo = c.out_hw
    M = c.M
    xd = x.permute(0, 2, 3, 1).to(td).contiguous()          # NHWC
    rd = _rows(res).to(td).contiguous() if res is not None else None
    del x, res
    if c.kind == "mean":
        nb = L.load().vk_conv1x1_meanpool_workspace_bytes(c.N, c.W, c.cout)
        ws = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
        got = torch.full((c.N, c.cout), float("nan"), dtype=torch.float32, device=G.DEV)
        G.launch("vk_conv1x1_meanpool", G.P(xd), c.N, c.W, c.cin, G.P(wd), G.P(bd), G.P(rd), c.cout, c.relu, G.P(got), G.P(ws), nb,
                 G.stream(), expect_route=c.route)
        torch.cuda.synchronize()
        return got, want
    ldy = (c.cout + 7) // 8 * 8
    y = torch.full((M, ldy), float("nan"), dtype=tod, device=G.DEV)
    if c.kind == "dual":
        x2 = xd.view(M, -1)
        x1d, x2d = x2[:, :c.cin].contiguous(), x2[:, c.cin:].contiguous()
        G.launch("vk_conv1x1_dual", G.P(x1d), c.cin, G.P(x2d), c.cin2, M, G.P(wd), G.P(bd), G.P(rd), G.P(y), c.cout, c.relu, G.stream(),
                 expect_route=c.route)
    elif c.kind == "linear":
        G.launch("vk_linear", G.P(xd), M, c.cin, G.P(wd), G.P(bd), G.P(rd), G.P(y), c.cout, ldy, c.relu, c.dt, c.odt, G.stream(),
                 expect_route=c.route)
    else:
        G.launch("vk_conv2d", G.P(xd), c.N, c.H, c.W, c.cin, G.P(wd), G.P(bd), G.P(rd), G.P(y), c.cout, ldy, c.k, c.k, c.stride, c.pad,
                 c.dil, c.groups, c.relu, c.dt, c.odt, G.stream(), expect_route=c.route)
    torch.cuda.synchronize()
    return y[:, :c.cout], _rows(want)


def assert_exact(c, got, want):
    assert not bool(torch.isnan(got).any()), f"{c.name}: NaN in the output"
    if not torch.equal(got, want):
        bad = got != want
        rows = bad.any(dim=1).nonzero().flatten()
        cols = bad.any(dim=0).nonzero().flatten()
        i = bad.nonzero()[0].tolist()
        raise AssertionError(
            f"{c.name} on the {c.route} kernel: {int(bad.sum())} of {bad.numel()} outputs differ from float64 rounded once; rows "
            f"{rows[:8].tolist()}... ({rows.numel()}), channels {cols[:8].tolist()}... ({cols.numel()}); first at {i}: got "
            f"{float(got[i[0], i[1]])!r}, expected {float(want[i[0], i[1]])!r}")
    r = REPORT.setdefault(c.route + (" (fused mean)" if c.kind == "mean" else ""), [0, 0])
    r[0] += 1
    r[1] += got.numel()


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c.name for c in EXACT_CASES])
def test_conv_exact(case, monkeypatch):
    got, want = run_case(case, monkeypatch)
    assert_exact(case, got, want)


BNECK_SHAPES = [(2, 20, 27), (1, 67, 30), (3, 13, 45)]


def _pack_bneck(p, proj):
    f = lambda k: p[k].numpy().astype(np.float32)            # noqa: E731
    w1d, b1d = G.pack_conv(f("w1"), None, f("b1"), F16)
    w2d, b2d = G.pack_conv(f("w2"), None, f("b2"), F16)
    w3d, b3d = G.pack_conv(f("w3"), None, f("b3"), F16)
    if proj:                                                # rows [conv3 | shortcut]: vk_conv1x1_dual's layout
        wsd, _ = G.pack_conv(f("wsc"), None, None, F16)
        rows = b3d.numel()
        w3d = torch.cat([w3d.view(rows, 64 * 2), wsd.view(rows, 64 * 2)], dim=1).contiguous()
    return w1d, b1d, w2d, b2d, w3d, b3d


def _run_bneck(shape, proj, form, edge, monkeypatch):
    monkeypatch.setenv("VK_BNECK_ROWS", "1" if form == "rows" else "0")
    N, H, W = shape
    p = X.make_bneck(proj, N, H, W, edge=edge)
    layers, bounds = X.bneck_expected(p, proj)
    X.check_bneck_conditions(layers, bounds, edge)
    want = layers[2][1].permute(0, 2, 3, 1).contiguous()
    cin = 64 if proj else 256
    assert L.load().vk_bottleneck64_eligible(cin, 64, 256, 1, 1, 1, int(proj), int(proj), N, H, W, F16) == 1
    w1d, b1d, w2d, b2d, w3d, b3d = _pack_bneck(p, proj)
    xd = p["x"].permute(0, 2, 3, 1).to(torch.float16).contiguous().to(G.DEV)
    y = torch.full((N, H, W, 256), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_bottleneck64", G.P(xd), N, H, W, cin, int(proj), G.P(w1d), G.P(b1d), G.P(w2d), G.P(b2d), G.P(w3d), G.P(b3d), G.P(y), G.stream())
    torch.cuda.synchronize()
    c = Case(f"bottleneck64/{form}" + (f"/{edge}" if edge else ""), "bneck64")
    assert_exact(c, y.cpu().view(-1, 256), want.view(-1, 256))


@pytest.mark.parametrize("form", ["rows", "tiles"])
@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("shape", BNECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bottleneck64_exact(shape, proj, form, monkeypatch):
    """vk_bottleneck64, both forms: the three layers in float64 with a round to f16 after each (the two intermediates never
    leave the CU, so only data that rounds them can see how the kernel does it)."""
    _run_bneck(shape, proj, form, None, monkeypatch)


@pytest.mark.parametrize("form", ["rows", "tiles"])
@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("edge", X.EDGES[1:])
def test_bottleneck64_exact_edges(edge, proj, form, monkeypatch):
    """The three edge cases on the fused block's own epilogues: an output that overflows to +inf (0 behind the ReLU), subnormal
    intermediates and outputs (kept, and read back as MFMA operands), one activation of 2047 beside values <= 3."""
    _run_bneck(BNECK_SHAPES[0], proj, form, edge, monkeypatch)


STEM_CASES = [((2, 37, 53), 1), ((1, 123, 200), 0), ((3, 64, 64), 1)]


def pack_stem(w, beta):
    """(packed f16 weight bytes, packed f32 bias) of the integer stem on the host: BN as gamma 1, beta, mean 0, var 1 - 1e-5."""
    import ctypes as C
    bn = np.concatenate([np.ones(64), beta.numpy(), np.zeros(64), np.full(64, 1.0 - 1e-5)]).astype(np.float32)
    wp = np.zeros(L.load().vk_packed_stem_bytes(64, F16), dtype=np.uint8)
    bp = np.zeros(L.load().vk_packed_cout(64), dtype=np.float32)
    L.call("vk_pack_stem_weight", np.ascontiguousarray(w.numpy().astype(np.float32)).ctypes.data_as(C.c_void_p),
           bn.ctypes.data_as(C.c_void_p), 64, F16, wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    return wp, bp


def _run_stem(shape, caffe, fused, edge, monkeypatch):
    import ctypes as C
    monkeypatch.setenv("VK_STEM_FUSED", fused)
    N, H, W = shape
    x, w, beta = X.make_stem(N, H, W, edge=edge)
    _, _, want = X.stem_expected(x, w, beta, caffe)
    wp, bp = pack_stem(w, beta)
    assert np.array_equal(np.sort(wp.view(np.float16).astype(np.float64))[-5:], np.full(5, float(w.max()))) and np.array_equal(bp[:64], beta.numpy())
    wd, bd, xd = torch.from_numpy(wp).to(G.DEV), torch.from_numpy(bp).to(G.DEV), x.float().to(G.DEV)
    ho, wo = C.c_int(), C.c_int()
    L.load().vk_stem_out_hw(H, W, caffe, C.byref(ho), C.byref(wo))
    assert (ho.value, wo.value) == tuple(want.shape[2:])
    ws = torch.empty(L.load().vk_stem_workspace_bytes(N, H, W, 64, F16), dtype=torch.uint8, device=G.DEV)
    y = torch.full((N, ho.value, wo.value, 64), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_stem", G.P(xd), N, H, W, G.P(wd), G.P(bd), 64, caffe, G.P(y), F16, G.P(ws), ws.numel(), G.stream())
    torch.cuda.synchronize()
    form = "fused" if fused == "1" else "unfused"
    c = Case(f"stem/{form}" + (f"/{edge}" if edge else ""), "stem " + form)
    assert_exact(c, y.cpu().view(-1, 64), want.permute(0, 2, 3, 1).reshape(-1, 64))


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape,caffe", STEM_CASES)
def test_stem_exact(shape, caffe, fused, monkeypatch):
    """vk_stem on integer pixels, as one kernel (stem_pool.hip) and as the generic kernel's stem form + the pool kernel."""
    _run_stem(shape, caffe, fused, None, monkeypatch)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
@pytest.mark.parametrize("edge", X.EDGES[1:])
def test_stem_exact_edges(edge, fused, monkeypatch):
    """The three edge cases on the stem's own epilogues (the conv's store, the pool on top of it): +inf through the max-pool,
    subnormal results, one pixel of 2047 beside pixels <= 3."""
    _run_stem(*STEM_CASES[0], fused, edge, monkeypatch)


def test_zz_report(capsys):
    """Not a check of its own: prints, once, what the cases above compared (per kernel: cases, output elements)."""
    with capsys.disabled():
        print("\n[conv exact] kernel: cases, output elements compared bit for bit")
        for k in sorted(REPORT):
            print(f"[conv exact]   {k:22s} {REPORT[k][0]:4d} {REPORT[k][1]:14d}")
