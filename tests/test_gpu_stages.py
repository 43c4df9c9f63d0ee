"""-m gpu: stage-level parity of the HIP kernels against the oracle, through the C ABI.

Tolerances (metric: max|a-b| / max|ref|):
  * convolution / GEMM, fp32 strict mode ...... 2e-5 (exact-f32 MFMA, different summation order)
  * convolution / GEMM, fp16 fast mode ........ 1e-3 against the fp16-emulating oracle
    (same fp16-rounded operands, fp32 accumulate; differences = summation order + one fp16 ulp)
  * convolution on integer data ............... bit-exact (tests/test_gpu_conv_exact.py: the anchor of every conv kernel)
  * pooling, NMS, top-k, index outputs ........ bit-exact
  * box decode ................................ 2e-6 (expf implementations differ by <= 1 ulp)

Every launch of a test that is about one kernel names that kernel (`expect_route=`): the dispatcher is asked
(vk_conv_route) immediately before the launch, so a change of an eligibility rule cannot quietly empty an A/B test.  The
`*_legs` functions below hold, per case, the environment of each run and the kernel it must run on; tests/test_abi.py
checks the same tables against the dispatcher without a GPU (`route_plan`).
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import frcnn_oracle as orc          # noqa: E402
from oracle.frcnn_oracle import FRCNNOracle    # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402
from vltk_amd.config import Config, vg_c4_config_dict   # noqa: E402

import gpu_util as G                           # noqa: E402
from proposals_util import _nms_gpu, _rpn_gpu  # noqa: E402  (the proposal stage's call helpers)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


CONV_CASES = [
    # name, N,H,W, cin, cout, k, stride, pad, dil, residual, relu
    ("1x1", 2, 13, 17, 64, 256, 1, 1, 0, 1, False, True),
    ("1x1_narrow", 1, 20, 21, 64, 64, 1, 1, 0, 1, False, True),
    ("1x1_s2", 2, 14, 19, 256, 128, 1, 2, 0, 1, False, False),
    ("3x3", 2, 12, 15, 64, 64, 3, 1, 1, 1, False, True),
    ("3x3_wide", 1, 9, 11, 128, 128, 3, 1, 1, 1, False, True),
    ("3x3_dil2", 3, 14, 14, 128, 128, 3, 1, 2, 2, False, True),
    ("1x1_res", 2, 10, 13, 128, 512, 1, 1, 0, 1, True, True),
    ("3x3_s2", 1, 15, 16, 64, 128, 3, 2, 1, 1, False, True),
    ("1x1_big", 1, 40, 50, 512, 256, 1, 1, 0, 1, False, True),   # 2000 rows: several pixel tiles + an edge tile
    # 256x256 LDS-ring kernel (Cout % 256 == 0, M >= 1024): K-stage ring lengths 2, 4, 6, 16, 18, 36 (fp16 packing makes the stage count even)
    ("ring_s2", 2, 24, 24, 64, 256, 1, 1, 0, 1, False, False),
    ("ring_s4", 2, 24, 24, 128, 512, 1, 1, 0, 1, True, True),
    ("ring_s6", 1, 33, 37, 192, 256, 1, 1, 0, 1, True, True),
    ("ring_1x1_k512", 2, 30, 50, 512, 1024, 1, 1, 0, 1, True, True),
    ("ring_3x3", 2, 25, 31, 64, 256, 3, 1, 1, 1, False, True),
    ("ring_3x3_dil2", 7, 14, 14, 128, 256, 3, 1, 2, 2, False, True),
    ("ring_1x1_s2", 2, 47, 51, 256, 512, 1, 2, 0, 1, False, False),
    # LDS-panel 3x3 kernel (stride 1, pad == dil, Cin >= 128, Cout % 256 == 0): halo 64 (PP=3) and 128 (PP=4),
    # RoI-shaped maps whose taps cross image borders inside a tile, image-count not a multiple of the tile
    ("panel_head", 9, 14, 14, 128, 256, 3, 1, 2, 2, False, True),
    ("panel_head_res", 11, 14, 14, 256, 512, 3, 1, 2, 2, True, True),
    ("panel_d1", 3, 20, 31, 128, 256, 3, 1, 1, 1, False, True),
    ("panel_wide", 1, 18, 84, 192, 256, 3, 1, 1, 1, False, False),
    ("panel_wide_d1", 2, 30, 100, 128, 256, 3, 1, 1, 1, True, True),
    ("panel_tiny", 1, 14, 14, 128, 256, 3, 1, 2, 2, False, True),      # M = 196 < one tile (last RoI chunk of a batch)
    ("panel_res4", 1, 50, 84, 128, 256, 3, 1, 1, 1, True, True),       # one 800 x 1333 image at res4: 4200 px, reach 85 (halo 112 / 128)
    # two-workgroups-per-CU 1x1 kernel (128x256 tiles, 3-slot ring): stage counts 2, 4, 6, 10, 16 (prologue-only,
    # tail-only and steady-state paths), an edge tile, stride 2, with and without residual / ReLU
    ("duo_s2", 3, 24, 24, 64, 256, 1, 1, 0, 1, False, False),
    ("duo_s4", 2, 24, 30, 128, 512, 1, 1, 0, 1, True, True),
    ("duo_s6", 1, 33, 37, 192, 256, 1, 1, 0, 1, True, True),
    ("duo_s10", 2, 23, 29, 320, 256, 1, 1, 0, 1, True, False),
    ("duo_s16", 2, 30, 50, 512, 1024, 1, 1, 0, 1, True, True),
    ("duo_s2_stride2", 2, 47, 51, 256, 512, 1, 2, 0, 1, False, True),
]


# fp16 route of the cases that are named after a shape, not a kernel, under test_conv's first environment
CONV_SHAPE_ROUTES = {"1x1": "generic", "1x1_narrow": "generic", "1x1_s2": "generic", "3x3": "blk", "3x3_wide": "generic",
                     "3x3_dil2": "generic", "1x1_res": "generic", "3x3_s2": "generic", "1x1_big": "ws"}
# the cases that the weight-stationary kernel takes when nothing pins it: that run is kept as a second leg
CONV_ALSO_WS = ("ring_s2", "ring_s4", "ring_1x1_k512", "ring_1x1_s2", "duo_s2", "duo_s4", "duo_s16", "duo_s2_stride2")


def _set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# test_conv's further runs of a panel case, each bit-identical to the first: 288- and 256-pixel tiles (9 / 8 row tiles per wave; the
# launcher picks by grid rounds), then the epilogue straight from the accumulators against its first form through LDS (halo-64
# build: VK_CONV256_DBG=8)
PANEL_FORM_LEGS = (({"VK_PANEL_MI": "9"}, "panel"), ({"VK_PANEL_MI": "8"}, "panel"), ({"VK_PANEL_MI": "8", "VK_CONV256_DBG": "8"}, "panel"))


def panel_mi9_legal(W, dil):
    """conv3x3_panel.hip panel_pp: 9 row tiles need the halo dil * (W + 1) <= 112; beyond that VK_PANEL_MI=9 silently runs 8 and the
    8 / 9 comparison would be empty."""
    return dil * (W + 1) <= 112


def conv_geom(case, dt):
    _, N, H, W, cin, cout, k, stride, pad, dil, use_res, relu = case
    return dict(N=N, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, pad=pad, dil=dil, relu=int(relu), res=use_res, dt=dt)


def conv_legs(case, dt):
    """[(environment, kernel)] of test_conv's runs.  The dispatcher re-reads the switches per call: "ring_*" cases pin the
    256x256 ring kernel and "duo_*" the two-per-CU kernel, which the weight-stationary / four-wave / panel kernels would
    otherwise take over; fp32 always runs the generic kernel."""
    name = case[0]
    ring = name.startswith("ring_")
    env = {"VK_CONV_DUO": "0" if ring else "1", "VK_CONV3X3_PANEL": "0" if ring else "1", "VK_CONV_WS": None, "VK_CONV_GEMM4": None}
    if dt != L.VK_F16:
        return [(env, "generic")]
    if ring or name.startswith("duo_"):
        legs = [(dict(env, VK_CONV_WS="0", VK_CONV_GEMM4="0"), "ring" if ring else "duo")]
        if name in CONV_ALSO_WS:
            legs.append((env, "ws"))
        return legs
    return [(env, "panel" if name.startswith("panel_") else CONV_SHAPE_ROUTES[name])]


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv(case, dt, monkeypatch):
    _, N, H, W, cin, cout, k, stride, pad, dil, use_res, relu = case
    g = _rng(zlib.crc32(case[0].encode()))
    x = torch.from_numpy(g.standard_normal((N, cin, H, W)).astype(np.float32))
    w = (g.standard_normal((cout, cin, k, k)) * (2.0 / (cin * k * k)) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    res = torch.from_numpy(g.standard_normal((N, cout, Ho, Wo)).astype(np.float32)) if use_res else None
    wf, bf = G.fold_ref(w, bn, dt)
    q = (lambda t: t.half().float()) if dt == L.VK_F16 else (lambda t: t)
    ref = F.conv2d(q(x), wf, None, stride, pad, dil) + bf.view(1, -1, 1, 1)
    if use_res:
        ref = ref + q(res)
    if relu:
        ref = F.relu(ref)
    ref = q(ref)
    tol = 1e-3 if dt == L.VK_F16 else 2e-5
    for env, route in conv_legs(case, dt):
        _set_env(monkeypatch, env)
        y = G.conv2d(x, w, bn=bn, residual_nchw=res, stride=stride, pad=pad, dil=dil, relu=relu, dt=dt, expect_route=route)
        assert G.rel_err(y, ref) <= tol, route
    if case[0].startswith("panel_") and dt == L.VK_F16:
        assert panel_mi9_legal(W, dil)
        ys = []
        for env, route in PANEL_FORM_LEGS:
            _set_env(monkeypatch, env)
            ys.append(G.conv2d(x, w, bn=bn, residual_nchw=res, stride=stride, pad=pad, dil=dil, relu=relu, dt=dt, expect_route=route))
        assert all(torch.equal(y, t) for t in ys)


GROUPED_CASES = [
    # name, N,H,W, channels, groups, stride, dil   (BottleneckBlock conv2 of ResNeXt: frcnn.py:942-952)
    ("x152_res2", 2, 20, 27, 256, 32, 1, 1),        # 8 channels per group
    ("x152_res3", 1, 17, 19, 512, 32, 1, 1),        # 16
    ("x152_res4", 1, 13, 15, 1024, 32, 1, 1),       # 32
    ("x152_res5", 3, 14, 14, 2048, 32, 1, 2),       # 64, dilation 2 (RoI head)
    ("wide_groups", 1, 11, 13, 256, 2, 1, 1),       # 128 per group: slice wider than the output tile
    ("stride2", 1, 21, 22, 128, 4, 2, 1),           # STRIDE_IN_1X1 = false puts the stride on conv2
]


def grouped_geom(case, dt):
    _, N, H, W, c, groups, stride, dil = case
    return dict(N=N, H=H, W=W, cin=c, cout=c, k=3, stride=stride, pad=dil, dil=dil, groups=groups, relu=1, dt=dt)


def grouped_legs(case, dt):
    """The slice-diagonal form of the generic kernel; in fp16 the block kernel takes the four ResNeXt shapes first (that run
    is the second leg)."""
    legs = [({"VK_CONV3X3_BLK": "0"}, "generic")]
    if dt == L.VK_F16 and case[0].startswith("x152_"):
        legs.append(({"VK_CONV3X3_BLK": None}, "blk"))
    return legs


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", GROUPED_CASES, ids=[c[0] for c in GROUPED_CASES])
def test_grouped_conv(case, dt, monkeypatch):
    _, N, H, W, c, groups, stride, dil = case
    g = _rng(zlib.crc32(case[0].encode()))
    x = torch.from_numpy(g.standard_normal((N, c, H, W)).astype(np.float32))
    w = (g.standard_normal((c, c // groups, 3, 3)) * (2.0 / (c // groups * 9)) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, c), g.standard_normal(c) * 0.1, g.standard_normal(c) * 0.1, g.uniform(0.5, 1.5, c))
    wf, bf = G.fold_ref(w, bn, dt)
    q = (lambda t: t.half().float()) if dt == L.VK_F16 else (lambda t: t)
    ref = q(F.relu(F.conv2d(q(x), wf, None, stride, dil, dil, groups) + bf.view(1, -1, 1, 1)))
    for env, route in grouped_legs(case, dt):
        _set_env(monkeypatch, env)
        y = G.conv2d(x, w, bn=bn, stride=stride, pad=dil, dil=dil, relu=True, dt=dt, groups=groups, expect_route=route)
        assert G.rel_err(y, ref) <= (1e-3 if dt == L.VK_F16 else 2e-5), route


BLK_CASES = [
    # name, N,H,W, channels, groups, dil: what conv3x3_blk.hip takes (64-channel slabs of 2-D tiles, weights in registers)
    ("dense64_ragged", 3, 37, 70, 64, 1, 1),        # res2 conv2 of ResNet-50/101: tiles of 8 x 32 with ragged right / bottom edges
    ("dense64_tiny", 1, 5, 9, 64, 1, 1),            # an image smaller than one tile
    ("g8_multi_tile", 2, 41, 67, 256, 32, 1),       # 8 channels per group, several tiles per slab and per workgroup
    ("g16", 2, 19, 33, 512, 32, 1),
    ("g32", 3, 50, 84, 1024, 32, 1),                # res4 of ResNeXt-152 32x8d at its real map size
    ("g64_roi", 37, 14, 14, 2048, 32, 2),           # Res5 head: one tile per RoI, dilation 2, ragged last pixel block
    ("g32_roi", 5, 14, 14, 128, 4, 2),
]


BLK_LEGS = (("1", "blk"), ("0", "generic"))                 # VK_CONV3X3_BLK, kernel


def blk_geom(case):
    _, N, H, W, c, groups, dil = case
    return dict(N=N, H=H, W=W, cin=c, cout=c, k=3, pad=dil, dil=dil, groups=groups, relu=int(c != 128))


@pytest.mark.parametrize("case", BLK_CASES, ids=[c[0] for c in BLK_CASES])
def test_conv3x3_blk_kernel(case, monkeypatch):
    """conv3x3_blk.hip against the fp32 reference AND bit-for-bit against the im2col kernel it replaces (same K order; the
    products it skips are with structurally-zero weights)."""
    _, N, H, W, c, groups, dil = case
    g = _rng(zlib.crc32(case[0].encode()))
    x = torch.from_numpy(g.standard_normal((N, c, H, W)).astype(np.float32))
    w = (g.standard_normal((c, c // groups, 3, 3)) * (2.0 / (c // groups * 9)) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, c), g.standard_normal(c) * 0.1, g.standard_normal(c) * 0.1, g.uniform(0.5, 1.5, c))
    ys = []
    for on, route in BLK_LEGS:
        monkeypatch.setenv("VK_CONV3X3_BLK", on)
        ys.append(G.conv2d(x, w, bn=bn, stride=1, pad=dil, dil=dil, relu=(c != 128), dt=L.VK_F16, groups=groups, expect_route=route))
    assert torch.equal(ys[0], ys[1])
    wf, bf = G.fold_ref(w, bn, L.VK_F16)
    ref = F.conv2d(x.half().float(), wf, None, 1, dil, dil, groups) + bf.view(1, -1, 1, 1)
    ref = (F.relu(ref) if c != 128 else ref).half().float()
    assert G.rel_err(ys[0], ref) <= 1e-3


DUAL_CASES = [(1500, 64, 64, 256, False), (33403, 64, 64, 256, False), (9000, 64, 64, 512, True), (4000, 512, 1024, 512, False),
              (130, 128, 256, 256, True), (2600, 128, 192, 256, True),
              (2500, 512, 1024, 2048, False), (1030, 256, 768, 256, True)]
# the switches test_conv1x1_dual turns off, run after run, and the kernel of each run: 64 + 64 channels; K >= 1024 at M >= 2048;
# K >= 1024 below the four-wave GEMM's floor; short K
DUAL_OFF = ((), ("VK_CONV_WS",), ("VK_CONV_WS", "VK_CONV_GEMM4"), ("VK_CONV_WS", "VK_CONV_GEMM4", "VK_CONV256_DUAL"))


def dual_geom(M, c1, c2, cout, res):
    return dict(N=1, H=1, W=M, cin=c1, cin2=c2, cout=cout, relu=1, res=res)


def dual_legs(M, c1, c2, cout, res):
    if c1 == 64 and c2 == 64:
        routes = ("ws", "duo", "duo", "duo")
    elif c1 + c2 >= 1024:
        routes = ("gemm4", "gemm4", "ring", "duo") if M >= 2048 else ("ring", "ring", "ring", "duo")
    else:
        routes = ("duo",) * 4
    return [(dict({"VK_CONV_GEMM4": "2"}, **{k: "0" for k in off}), r) for off, r in zip(DUAL_OFF, routes)]


@pytest.mark.parametrize("M,c1,c2,cout,res", DUAL_CASES)
def test_conv1x1_dual(M, c1, c2, cout, res, monkeypatch):
    """conv3 + stride-1 projection shortcut as one GEMM (`out += shortcut`, frcnn.py:970-977): two inputs, K = c1 + c2.
    K >= 1024 runs on the 256 x 256 ring kernel, shorter K on the two-per-CU kernel; where both apply they give the same bits."""
    g = _rng(M + c1)
    x1 = torch.from_numpy(g.standard_normal((M, c1)).astype(np.float32)).half()
    x2 = torch.from_numpy(g.standard_normal((M, c2)).astype(np.float32)).half()
    w1 = (g.standard_normal((cout, c1, 1, 1)) * (1.0 / c1) ** 0.5).astype(np.float32)
    w2 = (g.standard_normal((cout, c2, 1, 1)) * (1.0 / c2) ** 0.5).astype(np.float32)
    bn1 = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    bn2 = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    r = torch.from_numpy(g.standard_normal((M, cout)).astype(np.float32)).half() if res else None
    p1, b1 = G.pack_conv(w1, bn1, None, L.VK_F16)
    p2, b2 = G.pack_conv(w2, bn2, None, L.VK_F16)
    rows = b1.numel()
    wcat = torch.cat([p1.view(rows, c1 * 2), p2.view(rows, c2 * 2)], dim=1).contiguous()
    x1d, x2d, rd = x1.to(G.DEV), x2.to(G.DEV), (r.to(G.DEV) if res else None)
    y = torch.empty((M, cout), dtype=torch.float16, device=G.DEV)
    legs = dual_legs(M, c1, c2, cout, res)
    _set_env(monkeypatch, legs[0][0])                       # VK_CONV_GEMM4=2: the four-wave GEMM also on grids this small
    G.launch("vk_conv1x1_dual", G.P(x1d), c1, G.P(x2d), c2, M, G.P(wcat), G.P(b1 + b2), G.P(rd), G.P(y), cout, 1, G.stream(),
             expect_route=legs[0][1])
    torch.cuda.synchronize()
    # the same layer on the other kernels that take it: weight-stationary kernel (64 + 64 channels) / four-wave GEMM (K >= 1024) ->
    # ring kernel -> two-per-CU kernel
    for env, route in legs[1:]:
        _set_env(monkeypatch, env)
        y2 = torch.full_like(y, float("nan"))
        G.launch("vk_conv1x1_dual", G.P(x1d), c1, G.P(x2d), c2, M, G.P(wcat), G.P(b1 + b2), G.P(rd), G.P(y2), cout, 1, G.stream(),
                 expect_route=route)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), env
    f1, fb1 = G.fold_ref(w1, bn1, L.VK_F16)
    f2, fb2 = G.fold_ref(w2, bn2, L.VK_F16)
    ref = x1.float() @ f1.view(cout, c1).t() + x2.float() @ f2.view(cout, c2).t() + (fb1 + fb2)
    if res:
        ref = ref + r.float()
    ref = F.relu(ref).half().float()
    assert G.rel_err(y.float().cpu(), ref) <= 1e-3


MEANPOOL_CASES = [(7, 196, 128, 256), (23, 196, 512, 512), (3, 255, 64, 256), (1, 128, 64, 256),
                  (301, 196, 512, 2048), (40, 130, 256, 1024), (9, 130, 512, 256)]


def meanpool_geom(N, HW, cin, cout):
    return dict(N=N, H=1, W=HW, cin=cin, cout=cout, relu=1, res=True, mean=True)


def meanpool_route(N, HW, cin, cout):
    """The weight-stationary kernel's fp64 sums from K = 512 and 1024 rows on; else the two-per-CU kernel's integer partials."""
    return "ws" if cin == 512 and N * HW >= 1024 else "duo"


def meanpool_legs(N, HW, cin, cout):
    """(environment, images, kernel) of test_conv1x1_meanpool's launches: the default kernel (run twice), the two-per-CU kernel, and
    -- from three images on -- the default kernel on the images behind the first two."""
    legs = [({"VK_CONV_WS": None}, N, meanpool_route(N, HW, cin, cout)), ({"VK_CONV_WS": "0"}, N, "duo")]
    if N > 2:
        legs.append(({"VK_CONV_WS": None}, N - 2, meanpool_route(N - 2, HW, cin, cout)))
    return legs


NONFINITE_SHAPE = (12, 196, 512, 512)
NONFINITE_LEGS = {"1": "ws", "0": "duo"}                    # VK_CONV_WS -> kernel of test_conv1x1_meanpool_nonfinite


@pytest.mark.parametrize("N,HW,cin,cout", MEANPOOL_CASES)
def test_conv1x1_meanpool(N, HW, cin, cout, monkeypatch):
    """Last Res5 conv3 + residual + ReLU with `.mean(dim=[2,3])` (frcnn.py:1401) folded into the epilogue: equal to
    conv -> f16 -> mean, bit-reproducible, and the same bits from the weight-stationary kernel (K = 512: 64-row tiles,
    fp64 sums per image handed over with atomics) and the two-per-CU kernel (128-row tiles, integer sums per tile):
    either way the per-image sums are exact."""
    g = _rng(N * HW)
    M = N * HW
    x = torch.from_numpy(g.standard_normal((M, cin)).astype(np.float32)).half()
    r = torch.from_numpy(g.standard_normal((M, cout)).astype(np.float32)).half()
    w = (g.standard_normal((cout, cin, 1, 1)) * (1.0 / cin) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    wp, bp = G.pack_conv(w, bn, None, L.VK_F16)
    xd, rd = x.to(G.DEV), r.to(G.DEV)
    nb = L.load().vk_conv1x1_meanpool_workspace_bytes(N, HW, cout)
    legs = meanpool_legs(N, HW, cin, cout)
    outs = []
    _set_env(monkeypatch, legs[0][0])
    for _ in range(2):
        ws = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
        out = torch.empty((N, cout), dtype=torch.float32, device=G.DEV)
        G.launch("vk_conv1x1_meanpool", G.P(xd), N, HW, cin, G.P(wp), G.P(bp), G.P(rd), cout, 1, G.P(out), G.P(ws), nb, G.stream(),
                 expect_route=legs[0][2])
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    _set_env(monkeypatch, legs[1][0])
    ws = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
    out = torch.empty((N, cout), dtype=torch.float32, device=G.DEV)
    G.launch("vk_conv1x1_meanpool", G.P(xd), N, HW, cin, G.P(wp), G.P(bp), G.P(rd), cout, 1, G.P(out), G.P(ws), nb, G.stream(),
             expect_route=legs[1][2])
    torch.cuda.synchronize()
    assert torch.equal(outs[0], out.cpu())
    wf, bf = G.fold_ref(w, bn, L.VK_F16)
    y = F.relu(x.float() @ wf.view(cout, cin).t() + bf + r.float()).half().float()
    ref = y.view(N, HW, cout).mean(dim=1)
    assert G.rel_err(outs[0], ref) <= 1e-3
    # position independence: the same images behind a different number of leading rows give the same bits
    for env, n2, route in legs[2:]:
        _set_env(monkeypatch, env)
        k = N - n2
        out2 = torch.empty((N - k, cout), dtype=torch.float32, device=G.DEV)
        ws = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
        xs, rs = xd[k * HW:].contiguous(), rd[k * HW:].contiguous()
        G.launch("vk_conv1x1_meanpool", G.P(xs), N - k, HW, cin, G.P(wp), G.P(bp), G.P(rs), cout, 1, G.P(out2), G.P(ws), nb, G.stream(),
                 expect_route=route)
        torch.cuda.synchronize()
        assert torch.equal(out2.cpu(), outs[0][k:])


@pytest.mark.parametrize("ws", ["1", "0"])
def test_conv1x1_meanpool_nonfinite(ws, monkeypatch):
    """An output that overflows f16 makes that image's mean of that channel NaN and touches nothing else -- on both
    fused-mean kernels, including an image that shares its 64-row tile with the overflowing one."""
    monkeypatch.setenv("VK_CONV_WS", ws)
    N, HW, cin, cout = NONFINITE_SHAPE
    g = _rng(5)
    M = N * HW
    x = torch.from_numpy(g.standard_normal((M, cin)).astype(np.float32)).half()
    r = torch.from_numpy(g.standard_normal((M, cout)).astype(np.float32)).half()
    w = (g.standard_normal((cout, cin, 1, 1)) * (1.0 / cin) ** 0.5).astype(np.float32)
    wp, bp = G.pack_conv(w, None, np.zeros(cout, np.float32), L.VK_F16)
    nb = L.load().vk_conv1x1_meanpool_workspace_bytes(N, HW, cout)

    xd = x.to(G.DEV)

    def run(rr):
        rd = rr.to(G.DEV)
        ws_ = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
        out = torch.empty((N, cout), dtype=torch.float32, device=G.DEV)
        G.launch("vk_conv1x1_meanpool", G.P(xd), N, HW, cin, G.P(wp), G.P(bp), G.P(rd), cout, 1, G.P(out), G.P(ws_), nb, G.stream(),
                 expect_route=NONFINITE_LEGS[ws])
        torch.cuda.synchronize()
        return out.cpu()

    clean = run(r)
    assert bool(torch.isfinite(clean).all())
    r2 = r.clone()
    hits = [(3, 195, 17), (7, 0, 300), (7, 100, 301)]        # (image, row of the image, channel): last row, first row, middle
    for n, row, c in hits:
        r2[n * HW + row, c] = float("inf")
    out = run(r2)
    mask = torch.zeros((N, cout), dtype=torch.bool)
    for n, _, c in hits:
        mask[n, c] = True
    assert bool(torch.isnan(out[mask]).all())
    assert torch.equal(out[~mask], clean[~mask])


def scale_shape(kernel):
    return (64, 14, 14, 256, 512, 3, 2, 2) if kernel == "panel" else (300, 14, 14, 512, 2048, 1, 0, 1)


def scale_env(kernel):
    """The named kernel; "ws": nothing pinned, the weight-stationary kernel takes 512 -> 2048 as it does in production."""
    if kernel == "ws":
        return {"VK_CONV_DUO": None, "VK_CONV3X3_PANEL": None, "VK_CONV_WS": None, "VK_CONV_GEMM4": None}
    return {"VK_CONV_DUO": "1" if kernel == "duo" else "0", "VK_CONV3X3_PANEL": "1" if kernel == "panel" else "0", "VK_CONV_WS": "0",
            "VK_CONV_GEMM4": "0"}


def scale_geom(kernel):
    N, H, W, cin, cout, k, pad, dil = scale_shape(kernel)
    return dict(N=N, H=H, W=W, cin=cin, cout=cout, k=k, pad=pad, dil=dil, relu=1, res=True)


SCALE_KERNELS = ["duo", "ring", "panel", "ws"]


@pytest.mark.parametrize("kernel", SCALE_KERNELS)
def test_conv_reproducible_at_scale(kernel, monkeypatch):
    """Thousands of workgroups, launched back to back: bit-identical output run to run and no wrong block.  (A copy
    of a fragment register whose hand-issued ds_read was still in flight once made rare 16-row blocks wrong on a
    loaded GPU: tests/test_asm_hazards.py checks the compiled code, this checks the device.)"""
    _set_env(monkeypatch, scale_env(kernel))
    g = _rng(99)
    N, H, W, cin, cout, k, pad, dil = scale_shape(kernel)
    M = N * H * W
    x = torch.randn((N, H, W, cin)).half().to(G.DEV)
    r = torch.randn((M, cout)).half().to(G.DEV)
    w = (g.standard_normal((cout, cin, k, k)) * (1.0 / (cin * k * k)) ** 0.5).astype(np.float32)
    wp, bp = G.pack_conv(w, None, np.zeros(cout, np.float32), L.VK_F16)
    ys = []
    for _ in range(4):
        y = torch.empty((M, cout), dtype=torch.float16, device=G.DEV)
        G.launch("vk_conv2d", G.P(x), N, H, W, cin, G.P(wp), G.P(bp), G.P(r), G.P(y), cout, cout, k, k, 1, pad, dil, 1, 1,
                 L.VK_F16, L.VK_F16, G.stream(), expect_route=kernel)
        torch.cuda.synchronize()
        ys.append(y)
    for y in ys[1:]:
        assert torch.equal(ys[0], y)
    wf = torch.from_numpy(w).half().float().to(G.DEV)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wf, None, 1, pad, dil).permute(0, 2, 3, 1).reshape(M, cout)
    ref = F.relu(ref + r.float())
    assert float((ys[0].float() - ref).abs().max()) <= 0.02 * float(ref.abs().max())


ONE_BY_ONE_GEOM = dict(N=2, H=30, W=40, cin=256, cout=512, relu=1, res=True)
ONE_BY_ONE_LEGS = (({"VK_CONV_WS": "0", "VK_CONV_DUO": "0"}, "ring"), ({"VK_CONV_WS": "0", "VK_CONV_DUO": "1"}, "duo"),
                   ({"VK_CONV_WS": None, "VK_CONV_DUO": None}, "ws"))


def test_conv_1x1_kernels_bit_identical(monkeypatch):
    """The two 1x1 kernels (256x256 ring, 128x256 two-per-CU) walk K in the same order with the same MFMA: a
    layer's bits do not depend on which of them the dispatcher picks (it picks by problem size) -- nor on the weight-stationary
    kernel, which takes this layer when nothing is pinned."""
    g = _rng(11)
    x = torch.from_numpy(g.standard_normal((2, 256, 30, 40)).astype(np.float32))
    w = (g.standard_normal((512, 256, 1, 1)) * 0.08).astype(np.float32)
    b = g.standard_normal(512).astype(np.float32)
    res = torch.from_numpy(g.standard_normal((2, 512, 30, 40)).astype(np.float32))
    ys = []
    for env, route in ONE_BY_ONE_LEGS:
        _set_env(monkeypatch, env)
        ys.append(G.conv2d(x, w, bias=b, residual_nchw=res, relu=True, dt=L.VK_F16, expect_route=route))
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


WS_CASES = [((7, 50, 84), 256, 1024, True), ((200, 14, 14), 512, 2048, True), ((3, 37, 41), 128, 512, True),
            ((200, 14, 14), 512, 512, False), ((1, 32, 33), 512, 256, True),
            ((2, 100, 167), 64, 256, True), ((1, 33, 35), 64, 512, False)]
WS_LEGS = (("1", "8", "ws"), ("0", "8", "duo"), ("1", "4", "ws"), ("1", "8", "ws"))      # VK_CONV_WS, VK_WS_WAVES, kernel


def ws_geom(M_hw, cin, cout, res):
    return dict(N=M_hw[0], H=M_hw[1], W=M_hw[2], cin=cin, cout=cout, relu=1, res=res)


@pytest.mark.parametrize("M_hw,cin,cout,res", WS_CASES)
def test_conv_ws_kernel_bit_identical(M_hw, cin, cout, res, monkeypatch):
    """conv_ws.hip (weight-stationary 1x1, K <= 512: weights in registers, pixels through an LDS-DMA ring that runs across
    tile boundaries) against the two-per-CU kernel on the same layer: bit-identical (same K order, same epilogue
    arithmetic), with many tiles per workgroup, a ragged last tile, every stage count (1 / 2 / 4 per tile) and both stage widths
    (K = 64: 64-channel stages)."""
    N, H, W = M_hw
    g = _rng(cin * cout + N)
    x = torch.from_numpy(g.standard_normal((N, cin, H, W)).astype(np.float32))
    w = (g.standard_normal((cout, cin, 1, 1)) * (2.0 / cin) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    r = torch.from_numpy(g.standard_normal((N, cout, H, W)).astype(np.float32)) if res else None
    ys = []
    for ws, waves, route in WS_LEGS:
        monkeypatch.setenv("VK_CONV_WS", ws)
        monkeypatch.setenv("VK_WS_WAVES", waves)            # two waves per SIMD (the default) / one
        ys.append(G.conv2d(x, w, bn=bn, residual_nchw=r, relu=True, dt=L.VK_F16, expect_route=route))
    assert all(torch.equal(ys[0], y) for y in ys[1:])
    wf, bf = G.fold_ref(w, bn, L.VK_F16)
    ref = F.conv2d(x.half().float(), wf) + bf.view(1, -1, 1, 1)
    if res:
        ref = ref + r.half().float()
    assert G.rel_err(ys[0], F.relu(ref).half().float()) <= 1e-3


# the one-image stride-3 case has 322 output rows, below both kernels' floor of 1024: the generic kernel runs it (twice); the
# four-image one is the stride-3 layer on the two kernels the test is about
WS_STRIDED_CASES = [((3, 100, 167), 256, 512, 2, False), ((5, 50, 84), 512, 1024, 2, False),
                    ((2, 51, 85), 512, 256, 2, True), ((1, 67, 40), 256, 256, 3, True), ((4, 67, 40), 256, 256, 3, True)]


def ws_strided_geom(M_hw, cin, cout, stride, relu):
    return dict(N=M_hw[0], H=M_hw[1], W=M_hw[2], cin=cin, cout=cout, stride=stride, relu=int(relu))


def ws_strided_legs(M_hw, cin, cout, stride, relu):
    """(VK_WS_STRIDED, kernel) of the three runs."""
    small = M_hw[0] * ((M_hw[1] - 1) // stride + 1) * ((M_hw[2] - 1) // stride + 1) < 1024
    return [(sw, "generic" if small else r) for sw, r in (("1", "ws"), ("0", "duo"), ("1", "ws"))]


@pytest.mark.parametrize("M_hw,cin,cout,stride,relu", WS_STRIDED_CASES)
def test_conv_ws_strided_bit_identical(M_hw, cin, cout, stride, relu, monkeypatch):
    """conv_ws.hip on strided 1x1 convs (the stride-2 projection shortcuts and first conv1s of res3 / res4, frcnn.py:934-941: the DMA
    lane maps its output row to an input pixel) against the two-per-CU kernel: bit-identical, odd sizes, ragged tiles."""
    N, H, W = M_hw
    g = _rng(cin * cout + N + stride)
    x = torch.from_numpy(g.standard_normal((N, cin, H, W)).astype(np.float32))
    w = (g.standard_normal((cout, cin, 1, 1)) * (2.0 / cin) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    ys = []
    for sw, route in ws_strided_legs(M_hw, cin, cout, stride, relu):
        monkeypatch.setenv("VK_WS_STRIDED", sw)
        ys.append(G.conv2d(x, w, bn=bn, stride=stride, relu=relu, dt=L.VK_F16, expect_route=route))
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    wf, bf = G.fold_ref(w, bn, L.VK_F16)
    ref = F.conv2d(x.half().float(), wf, None, stride) + bf.view(1, -1, 1, 1)
    assert G.rel_err(ys[0], (F.relu(ref) if relu else ref).half().float()) <= 1e-3


GEMM4_CASES = [((13, 14, 14), 2048, 512, False, True), ((11, 14, 14), 1024, 512, False, True),
               ((17, 14, 14), 1024, 256, True, True), ((2, 50, 84), 1024, 256, False, False),
               ((1, 45, 47), 1152, 512, True, False)]
GEMM4_LEGS = (("2", "1", "gemm4"), ("0", "1", "duo"), ("0", "0", "ring"), ("2", "1", "gemm4"))   # VK_CONV_GEMM4, VK_CONV_DUO, kernel


def gemm4_geom(M_hw, cin, cout, res, relu):
    return dict(N=M_hw[0], H=M_hw[1], W=M_hw[2], cin=cin, cout=cout, relu=int(relu), res=res)


@pytest.mark.parametrize("M_hw,cin,cout,res,relu", GEMM4_CASES)
def test_conv_gemm4_kernel_bit_identical(M_hw, cin, cout, res, relu, monkeypatch):
    """conv_gemm4.hip (1x1, K >= 1024: 256 x 256 tile, four waves of 128 x 128, accumulators in AGPRs) against the kernels that
    take the layer without it (two-per-CU / ring): bit-identical, with full and ragged tiles, with and without residual / ReLU,
    and nine groups of four stages (K = 1152)."""
    N, H, W = M_hw
    g = _rng(cin + cout + N)
    x = torch.from_numpy(g.standard_normal((N, cin, H, W)).astype(np.float32))
    w = (g.standard_normal((cout, cin, 1, 1)) * (2.0 / cin) ** 0.5).astype(np.float32)
    bn = (g.uniform(0.5, 1.5, cout), g.standard_normal(cout) * 0.1, g.standard_normal(cout) * 0.1, g.uniform(0.5, 1.5, cout))
    r = torch.from_numpy(g.standard_normal((N, cout, H, W)).astype(np.float32)) if res else None
    ys = []
    for g4, duo, route in GEMM4_LEGS:                       # "2": also on grids this small
        monkeypatch.setenv("VK_CONV_GEMM4", g4)
        monkeypatch.setenv("VK_CONV_DUO", duo)
        ys.append(G.conv2d(x, w, bn=bn, residual_nchw=r, relu=relu, dt=L.VK_F16, expect_route=route))
    assert all(torch.equal(ys[0], y) for y in ys[1:])
    wf, bf = G.fold_ref(w, bn, L.VK_F16)
    ref = F.conv2d(x.half().float(), wf) + bf.view(1, -1, 1, 1)
    if res:
        ref = ref + r.half().float()
    if relu:
        ref = F.relu(ref)
    assert G.rel_err(ys[0], ref.half().float()) <= 1e-3


GEMM4_MANY_CASES = [(40000, 2048, 0, 512, True, False), (39917, 512, 1024, 2048, True, False),
                    (70001, 1024, 0, 512, False, False), (33000, 2048, 0, 2048, True, True),
                    # res4's conv1 (full and half batch: 525 / 263 tiles), other grids of full rounds + a few tiles
                    (67200, 1024, 0, 256, True, False), (134400, 1024, 0, 256, True, False),
                    (66000, 512, 1024, 512, True, False), (66500, 2048, 0, 256, True, True),
                    # rows beyond the descriptor's 14-bit stride (stride = pitch / 2 or / 4, index = row * 2 or * 4):
                    # the FPN box head's fc1 (12544 -> 1024 at 32 x 1000 RoIs) and a 33 KB row
                    (32000, 12544, 0, 1024, True, False), (2100, 16512, 0, 256, False, False)]


def gemm4_many_geom(M, c1, c2, cout, relu, use_res):
    return dict(N=1, H=1, W=M, cin=c1, cin2=c2, cout=cout, relu=int(relu), res=use_res)


def gemm4_many_legs(M, c1, c2, cout, relu, use_res):
    """(VK_CONV_GEMM4, kernel): without the four-wave GEMM the two-input layers run on the ring kernel, the others on the
    two-per-CU kernel (M < 400 000)."""
    return [("2", "gemm4"), ("0", "ring" if c2 else "duo")]


@pytest.mark.parametrize("M,c1,c2,cout,relu,use_res", GEMM4_MANY_CASES)
def test_conv_gemm4_many_tiles_per_workgroup(M, c1, c2, cout, relu, use_res, monkeypatch):
    """conv_gemm4's persistent workgroups at sizes where each walks several tiles (one LDS ring across tile boundaries, the
    next tile's first stages requested by the previous tile's last ones, a ragged last tile): bit-identical to the kernel that
    takes the layer without it (two inputs: the ring kernel; one: the two-per-CU kernel)."""
    g = torch.Generator(device="cpu").manual_seed(M + c1)
    x1 = (torch.randn((M, c1), generator=g) * 0.7).half().to(G.DEV)
    x2 = (torch.randn((M, c2), generator=g) * 0.7).half().to(G.DEV) if c2 else None
    K = c1 + c2
    w = (np.random.Generator(np.random.PCG64(M)).standard_normal((cout, K, 1, 1)) * (2.0 / K) ** 0.5).astype(np.float32)
    b = np.random.Generator(np.random.PCG64(M + 1)).standard_normal(cout).astype(np.float32)
    wd, bd = G.pack_conv(w, None, b, L.VK_F16)
    res = (torch.randn((M, cout), generator=g) * 0.5).half().to(G.DEV) if use_res else None     # (ResNeXt's conv3: K = 2048 with the identity shortcut)
    ys = []
    for g4, route in gemm4_many_legs(M, c1, c2, cout, relu, use_res):   # "2": also on grids below its usual floor (here 2 - 5 tiles per workgroup)
        monkeypatch.setenv("VK_CONV_GEMM4", g4)
        y = torch.full((M, cout), float("nan"), dtype=torch.float16, device=G.DEV)
        if c2:
            G.launch("vk_conv1x1_dual", G.P(x1), c1, G.P(x2), c2, M, G.P(wd), G.P(bd), None, G.P(y), cout, int(relu), G.stream(),
                     expect_route=route)
        else:
            G.launch("vk_conv2d", G.P(x1), 1, 1, M, c1, G.P(wd), G.P(bd), G.P(res), G.P(y), cout, cout, 1, 1, 1, 0, 1, 1, int(relu), L.VK_F16,
                     L.VK_F16, G.stream(), expect_route=route)
        torch.cuda.synchronize()
        ys.append(y)
    assert torch.equal(ys[0], ys[1])
    # and against plain fp32 arithmetic on a sample of rows (first tile, a middle tile, the ragged last one)
    rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2, M // 2 + 300), torch.arange(M - 300, M)]).to(G.DEV)
    xa = x1[rows].float() if not c2 else torch.cat([x1[rows], x2[rows]], dim=1).float()
    ref = xa @ torch.from_numpy(w.reshape(cout, K)).to(G.DEV).half().float().t() + torch.from_numpy(b).to(G.DEV)
    if use_res:
        ref = ref + res[rows].float()
    ref = (F.relu(ref) if relu else ref).half().float()
    assert G.rel_err(ys[0][rows].float().cpu(), ref.cpu()) <= 1e-3


F32OUT_SHAPE = (2, 128, 9, 13, 75)                          # N, cin, H, W, cout
F32OUT_GEOM = dict(N=2, H=9, W=13, cin=128, cout=75, out_dt=L.VK_F32)


def test_conv_bias_f32_out():
    """fp16 operands, fp32 output with bias and a channel count that is not a multiple of 8 (RPN heads: 75)."""
    g = _rng(7)
    N, cin, H, W, cout = F32OUT_SHAPE
    assert (N, H, W, cin, cout) == tuple(F32OUT_GEOM[k] for k in ("N", "H", "W", "cin", "cout"))
    x = torch.from_numpy(g.standard_normal((N, cin, H, W)).astype(np.float32))
    w = (g.standard_normal((cout, cin, 1, 1)) * 0.1).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    y = G.conv2d(x, w, bias=b, dt=L.VK_F16, out_dt=L.VK_F32, expect_route="generic")
    ref = F.conv2d(x.half().float(), torch.from_numpy(w).half().float(), torch.from_numpy(b))
    assert y.shape == ref.shape
    assert G.rel_err(y, ref) <= 1e-5


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "kat_ops.npz"))


@pytest.mark.parametrize("tag", ["blk_s2_in1x1", "blk_s2_in3x3", "blk_identity", "blk_dil2", "blk_groups"])
def test_bottleneck_kat(kat, tag):
    """BottleneckBlock.forward (frcnn.py:963-979) chained from vk_conv2d calls, fp32 strict mode, against the
    reference's own output: stride in the 1x1 / in the 3x3, identity shortcut, dilation 2, groups 8."""
    cin, cout, mid, stride, groups, s1x1, dil = kat[tag + "/args"].tolist()
    sd = {k.split("/sd/")[1]: kat[k] for k in kat.files if k.startswith(tag + "/sd/")}
    x = torch.from_numpy(kat[tag + "/x"])
    if mid * 4 % 128:       # fp32 K-tiles are 32 channels: widen a 16-channel bottleneck with zero channels (same math)
        assert groups == 1
        pad = 32 - mid
        sd["conv1.weight"] = np.concatenate([sd["conv1.weight"], np.zeros((pad, cin, 1, 1), np.float32)])
        w2 = np.zeros((32, 32, 3, 3), np.float32)
        w2[:mid, :mid] = sd["conv2.weight"]
        sd["conv2.weight"] = w2
        sd["conv3.weight"] = np.concatenate([sd["conv3.weight"], np.zeros((cout, pad, 1, 1), np.float32)], axis=1)
        for c in ("conv1", "conv2"):
            for n, v in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0)):
                sd[f"{c}.norm.{n}"] = np.concatenate([sd[f"{c}.norm.{n}"], np.full(pad, v, np.float32)])

    def bn(p):
        return tuple(sd[f"{p}.norm.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))
    s1, s3 = (stride, 1) if s1x1 else (1, stride)
    dt = L.VK_F32
    sc = G.conv2d(x, sd["shortcut.weight"], bn=bn("shortcut"), stride=stride, dt=dt) if "shortcut.weight" in sd else x
    t = G.conv2d(x, sd["conv1.weight"], bn=bn("conv1"), stride=s1, relu=True, dt=dt)
    t = G.conv2d(t, sd["conv2.weight"], bn=bn("conv2"), stride=s3, pad=dil, dil=dil, relu=True, dt=dt, groups=groups)
    y = G.conv2d(t, sd["conv3.weight"], bn=bn("conv3"), residual_nchw=sc, relu=True, dt=dt)
    assert G.rel_err(y, kat[tag + "/y"]) <= 2e-5


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("tag,caffe", [("stem_caffe", 1), ("stem_pad1", 0)])
def test_stem(kat, tag, caffe, dt):
    """BasicStem (7x7 s2 conv + BN + ReLU + max-pool) against the reference's own output (golden)."""
    x = torch.from_numpy(kat[tag + "/x"])
    sd = {k.split("/sd/")[1]: kat[k] for k in kat.files if k.startswith(tag + "/sd/")}
    w = sd["conv1.weight"]
    cout = w.shape[0]
    bn = np.concatenate([sd["conv1.norm.weight"], sd["conv1.norm.bias"], sd["conv1.norm.running_mean"],
                         sd["conv1.norm.running_var"]]).astype(np.float32)
    wp = np.zeros(L.load().vk_packed_stem_bytes(cout, dt), dtype=np.uint8)
    bp = np.zeros(L.load().vk_packed_cout(cout), dtype=np.float32)
    L.call("vk_pack_stem_weight", np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p),
           cout, dt, wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    wd, bd = torch.from_numpy(wp).to(G.DEV), torch.from_numpy(bp).to(G.DEV)
    N, _, H, W = x.shape
    ho, wo = C.c_int(), C.c_int()
    L.load().vk_stem_out_hw(H, W, caffe, C.byref(ho), C.byref(wo))
    ref = kat[tag + "/y"]
    assert (ho.value, wo.value) == ref.shape[2:]
    ws = torch.empty(L.load().vk_stem_workspace_bytes(N, H, W, cout, dt), dtype=torch.uint8, device=G.DEV)
    y = torch.empty((N, ho.value, wo.value, cout), dtype=G.TDT[dt], device=G.DEV)
    xd = x.to(G.DEV)
    L.call("vk_stem", G.P(xd), N, H, W, G.P(wd), G.P(bd), cout, caffe, G.P(y), dt, G.P(ws), ws.numel(), G.stream())
    out = G.to_nchw(y, dt)
    if dt == L.VK_F32:
        assert G.rel_err(out, ref) <= 2e-5
    else:
        d = vg_c4_config_dict()
        d["model"]["max_pool"] = bool(caffe)
        o = FRCNNOracle(Config(d), {"backbone.stem." + k: torch.from_numpy(v) for k, v in sd.items()}, emulate="fp16")
        assert G.rel_err(out, o.stem(x)) <= 1e-3
        assert G.rel_err(out, ref) <= 1e-2      # fp16 storage vs the fp32 reference (reported, loose)


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("hw,caffe", [((17, 23), 1), ((16, 22), 1), ((16, 22), 0), ((9, 9), 1)])
def test_maxpool(hw, caffe, dt):
    g = _rng(11)
    x = torch.from_numpy(g.standard_normal((2, 16, *hw)).astype(np.float32))
    if dt == L.VK_F16:
        x = x.half().float()
    ref = F.max_pool2d(x, 3, 2, 0, ceil_mode=True) if caffe else F.max_pool2d(x, 3, 2, 1)
    xd = G.to_nhwc(x, dt)
    y = torch.empty((2, ref.shape[2], ref.shape[3], 16), dtype=G.TDT[dt], device=G.DEV)
    L.call("vk_maxpool3x3s2", G.P(xd), 2, hw[0], hw[1], 16, caffe, G.P(y), dt, G.stream())
    np.testing.assert_array_equal(G.to_nchw(y, dt).numpy(), ref.numpy())


@pytest.mark.parametrize("caffe", [1, 0], ids=["caffe", "pad1"])
@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 37, 53), (3, 64, 64), (1, 123, 200), (2, 131, 67), (1, 800, 1333)],
                         ids=lambda s: "x".join(map(str, s)))
def test_stem_fused_bit_identical(shape, caffe, monkeypatch):
    """The one-kernel stem (7x7 conv + BN + ReLU + max-pool out of LDS, csrc/stem_pool.hip) gives the bits of the
    im2col conv followed by the pool kernel: same MFMA, same K order, same epilogue; tile edges, odd sizes, both pools."""
    N, H, W = shape
    g = _rng(H * 1000 + W)
    x = torch.from_numpy((g.standard_normal((N, 3, H, W)) * 60.0).astype(np.float32))
    w = (g.standard_normal((64, 3, 7, 7)) * 0.05).astype(np.float32)
    bn = np.concatenate([g.uniform(0.5, 1.5, 64), g.standard_normal(64) * 0.1, g.standard_normal(64) * 0.1, g.uniform(0.5, 1.5, 64)]).astype(np.float32)
    dt = L.VK_F16
    wp = np.zeros(L.load().vk_packed_stem_bytes(64, dt), dtype=np.uint8)
    bp = np.zeros(L.load().vk_packed_cout(64), dtype=np.float32)
    L.call("vk_pack_stem_weight", np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p), 64, dt,
           wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    wd, bd, xd = torch.from_numpy(wp).to(G.DEV), torch.from_numpy(bp).to(G.DEV), x.to(G.DEV)
    ho, wo = C.c_int(), C.c_int()
    L.load().vk_stem_out_hw(H, W, caffe, C.byref(ho), C.byref(wo))
    outs = []
    for fused in ("1", "0", "1"):
        monkeypatch.setenv("VK_STEM_FUSED", fused)
        ws = torch.empty(L.load().vk_stem_workspace_bytes(N, H, W, 64, dt), dtype=torch.uint8, device=G.DEV)
        y = torch.full((N, ho.value, wo.value, 64), float("nan"), dtype=torch.float16, device=G.DEV)
        L.call("vk_stem", G.P(xd), N, H, W, G.P(wd), G.P(bd), 64, caffe, G.P(y), dt, G.P(ws), ws.numel(), G.stream())
        torch.cuda.synchronize()
        outs.append(y.cpu())
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
def test_roi_pool(dt):
    """RoIPool incl. the edge cases torchvision defines: negative / oversize / degenerate boxes, .5 rounding."""
    g = _rng(3)
    N, Cc, H, W, Pp = 2, 32, 11, 15, 7
    x = torch.from_numpy(g.standard_normal((N, Cc, H, W)).astype(np.float32))
    if dt == L.VK_F16:
        x = x.half().float()
    rois = [
        [0, 0, 0, 240, 176], [1, 8, 8, 8, 8], [0, -50, -30, 20, 40], [1, 100, 60, 400, 300],
        [0, 24, 40, 8, 8],            # x2 < x1: malformed -> forced 1x1
        [1, 8.0, 24.0, 56.0, 72.0],   # *1/16 -> exact .5 values (round half away from zero)
        [0, 300, 300, 400, 400],      # completely outside -> empty bins -> 0
        [1, 7.99, 8.01, 199.5, 130.2],
    ]
    for _ in range(24):
        xs, ys = sorted(g.uniform(-20, 260, 2)), sorted(g.uniform(-20, 200, 2))
        rois.append([int(g.integers(0, N)), xs[0], ys[0], xs[1], ys[1]])
    r = np.asarray(rois, dtype=np.float32)
    ref = orc.roi_pool(x, torch.from_numpy(r), Pp, 1.0 / 16)
    xd = G.to_nhwc(x, dt)
    rd = torch.from_numpy(r).to(G.DEV)
    y = torch.empty((len(r), Pp, Pp, Cc), dtype=G.TDT[dt], device=G.DEV)
    L.call("vk_roi_pool", G.P(xd), N, H, W, Cc, G.P(rd), len(r), 1.0 / 16, Pp, G.P(y), dt, G.stream())
    np.testing.assert_array_equal(G.to_nchw(y, dt).numpy(), ref.numpy())


def test_roi_pool_at_real_size():
    """The f16 RoIPool at the head's real shape (res4 map 50 x 84 x 1024, 14 x 14 bins, 600 RoIs from slivers to the whole image,
    boxes reaching outside): every output written, a sample of RoIs bit-exact against the oracle."""
    g = _rng(17)
    N, Cc, H, W, Pp = 2, 1024, 50, 84, 14
    x = torch.from_numpy(g.standard_normal((N, Cc, H, W)).astype(np.float32)).half().float()
    rois = [[0, 0, 0, 1333, 800], [1, -40, -40, 1400, 900], [0, 5, 5, 9, 9], [1, 640, 0, 660, 800], [0, 0, 400, 1333, 410],
            [1, 1300, 780, 1333, 800], [0, 2000, 2000, 2100, 2100]]
    for _ in range(593):
        cx, cy = g.uniform(0, 1333), g.uniform(0, 800)
        w, h = np.exp(g.uniform(np.log(8), np.log(1200))), np.exp(g.uniform(np.log(8), np.log(800)))
        rois.append([int(g.integers(0, N)), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    r = np.asarray(rois, dtype=np.float32)
    xd = G.to_nhwc(x, L.VK_F16)
    rd = torch.from_numpy(r).to(G.DEV)
    y = torch.full((len(r), Pp, Pp, Cc), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_roi_pool", G.P(xd), N, H, W, Cc, G.P(rd), len(r), 1.0 / 16, Pp, G.P(y), L.VK_F16, G.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    sample = list(range(7)) + list(range(7, 600, 37))
    ref = orc.roi_pool(x, torch.from_numpy(r[sample]), Pp, 1.0 / 16)
    np.testing.assert_array_equal(y[sample].float().permute(0, 3, 1, 2).cpu().numpy(), ref.numpy())


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
def test_mean_pool(dt):
    g = _rng(5)
    K, S, Cc = 5, 196, 2048
    x = torch.from_numpy(g.standard_normal((K, S, Cc)).astype(np.float32))
    if dt == L.VK_F16:
        x = x.half().float()
    xd = x.to(G.DEV, G.TDT[dt])
    out = torch.empty((K, Cc), dtype=torch.float32, device=G.DEV)
    L.call("vk_mean_pool", G.P(xd), K, S, Cc, G.P(out), dt, G.stream())
    torch.cuda.synchronize()
    assert G.rel_err(out.cpu(), x.mean(1)) <= 1e-6


@pytest.mark.parametrize("tag,w", [("deltas_rpn", (1.0, 1.0, 1.0, 1.0)), ("deltas_roi", (10.0, 10.0, 5.0, 5.0))])
def test_box_decode(kat, tag, w):
    d = torch.from_numpy(kat[tag + "/deltas"]).to(G.DEV)
    b = torch.from_numpy(kat[tag + "/boxes"]).to(G.DEV)
    out = torch.empty_like(d)
    L.call("vk_box_decode", G.P(d), G.P(b), d.shape[0], d.shape[1] // 4, (C.c_float * 4)(*w), G.P(out), G.stream())
    torch.cuda.synchronize()
    assert G.rel_err(out.cpu(), kat[tag + "/y"]) <= 2e-6


@pytest.mark.parametrize("n,thr,ties", [(1, 0.5, False), (37, 0.3, False), (300, 0.3, True), (1000, 0.7, True),
                                        (6000, 0.7, False), (6000, 0.5, True)])
def test_nms_bit_exact(n, thr, ties):
    """Greedy NMS: kept indices identical to the oracle, incl. score ties (lower index first) and
    clustered boxes (heavy suppression)."""
    g = _rng(n * 7 + int(thr * 10))
    ctr = g.uniform(0, 1300, (max(n // 20, 1), 2))
    c = ctr[g.integers(0, len(ctr), n)] + g.normal(0, 25, (n, 2))
    wh = g.uniform(8, 220, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = g.standard_normal(n).astype(np.float32)
    if ties:
        scores = np.round(scores * 4) / 4     # many exact ties
    ref = orc.nms(torch.from_numpy(boxes), torch.from_numpy(scores), thr).numpy()
    got = _nms_gpu(boxes, scores, thr)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("lead", ["0", "64", "192"])
def test_nms_two_phases_bit_exact(monkeypatch, lead):
    """launch_nms computes the suppression masks of the leading boxes first and the rest only for images whose sweep has not reached
    the cap (csrc/rpn.hip).  VK_NMS_LEAD forces a short first phase ("0": one phase): 6000 clustered boxes where every box may be
    kept (vk_nms: the second phase always runs), and RPN proposals at full size from HEAVILY overlapping anchors (tiny deltas on a
    coarse logit grid: the 300th survivor lies thousands of candidates deep) -- kept sets identical to the oracle either way."""
    monkeypatch.setenv("VK_NMS_LEAD", lead)
    g = _rng(4242)
    n = 6000
    ctr = g.uniform(0, 1300, (150, 2))
    c = ctr[g.integers(0, len(ctr), n)] + g.normal(0, 25, (n, 2))
    wh = g.uniform(8, 220, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = (np.round(g.standard_normal(n) * 4) / 4).astype(np.float32)
    np.testing.assert_array_equal(_nms_gpu(boxes, scores, 0.5), orc.nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.5).numpy())
    N, A, Hf, Wf = 2, 15, 50, 84
    obj = torch.from_numpy(g.standard_normal((N, A, Hf, Wf)).astype(np.float32))
    # logits that rise towards one corner: the top candidates are neighbouring, heavily overlapping anchors
    obj += torch.linspace(0, 40, Hf).view(1, 1, Hf, 1) + torch.linspace(0, 40, Wf).view(1, 1, 1, Wf)
    dlt = torch.from_numpy(g.standard_normal((N, 4 * A, Hf, Wf)).astype(np.float32) * 0.02)
    shapes = [[800, 1333], [750, 1200]]
    from vltk_amd.weights import cell_anchors
    cell = cell_anchors([32, 64, 128, 256, 512], [0.5, 1.0, 2.0])
    o = FRCNNOracle(Config(vg_c4_config_dict()), {"proposal_generator.anchor_generator.cell_anchors.0": torch.from_numpy(cell)})
    ref = o.rpn_proposals(obj, dlt, shapes)
    got = _rpn_gpu(obj, dlt, shapes, cell, pre=6000, post=300, thr=0.7)
    for (rb, rl), (gb, gl) in zip(ref, got):
        assert len(gb) == len(rb)
        np.testing.assert_array_equal(gl.numpy(), rl.numpy())
        assert G.rel_err(gb, rb) <= 2e-6
    print(f"\n[VK_NMS_LEAD={lead}] survivors per image: {[len(b) for b, _ in got]}")


def test_nms_empty():
    assert len(_nms_gpu(np.zeros((0, 4), np.float32), np.zeros((0,), np.float32), 0.5)) == 0


def test_rpn_proposals_golden(kat):
    """Same RPN head outputs in -> the reference's proposals out (golden from the reference module)."""
    res = _rpn_gpu(torch.from_numpy(kat["rpn/objectness"]), torch.from_numpy(kat["rpn/deltas"]),
                   kat["rpn/shapes"].tolist(), kat["anchors/cell"], pre=400, post=40, thr=0.7)
    for i, (b, l) in enumerate(res):
        assert b.shape == kat[f"rpn/boxes_{i}"].shape          # same number of survivors
        np.testing.assert_array_equal(l.numpy(), kat[f"rpn/logits_{i}"])   # same anchors, same order
        assert G.rel_err(b, kat[f"rpn/boxes_{i}"]) <= 2e-6


@pytest.mark.parametrize("ties", [False, True])
def test_rpn_proposals_full_size(ties):
    """50x84x15 = 63 000 anchors, top 6000, NMS 0.7, keep 300: kept set identical to the oracle."""
    g = _rng(99 + ties)
    N, A, Hf, Wf = 2, 15, 50, 84
    obj = torch.from_numpy(g.standard_normal((N, A, Hf, Wf)).astype(np.float32) * 3)
    if ties:
        obj = torch.round(obj * 8) / 8
    dlt = torch.from_numpy(g.standard_normal((N, 4 * A, Hf, Wf)).astype(np.float32) * 0.3)
    shapes = [[800, 1333], [750, 1200]]
    from vltk_amd.weights import cell_anchors
    cell = cell_anchors([32, 64, 128, 256, 512], [0.5, 1.0, 2.0])
    d = vg_c4_config_dict()
    d["proposal_generator"]["min_size"] = 2
    o = FRCNNOracle(Config(d), {"proposal_generator.anchor_generator.cell_anchors.0": torch.from_numpy(cell)})
    ref = o.rpn_proposals(obj, dlt, shapes)
    got = _rpn_gpu(obj, dlt, shapes, cell, pre=6000, post=300, thr=0.7, min_size=2.0)
    for (rb, rl), (gb, gl) in zip(ref, got):
        assert len(gb) == len(rb) == 300
        np.testing.assert_array_equal(gl.numpy(), rl.numpy())
        assert G.rel_err(gb, rb) <= 2e-6


@pytest.mark.parametrize("tag", ["roiout", "roiout_scaled"])
def test_roi_outputs_golden(kat, tag):
    """ROIOutputs.inference incl. do_nms' threshold-list retry, against the reference's own outputs."""
    N, R, Cn, An, Fd = 2, 20, 10, 5, 16
    counts = [20, 17]
    props = np.zeros((N, R, 4), np.float32)
    K = N * R

    def scatter(a):
        out = np.zeros((K,) + a.shape[1:], np.float32)
        out[0:20] = a[0:20]
        out[20:37] = a[20:37]
        return out
    for i in range(N):
        props[i, :counts[i]] = kat[f"roiout/props_{i}"]
    dev = G.DEV
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    obj, attr = t(scatter(kat["roiout/obj_logits"])), t(scatter(kat["roiout/attr_logits"]))
    bd, ft = t(scatter(kat["roiout/box_deltas"])), t(scatter(kat["roiout/feats_in"]))
    pr, cn = t(props), torch.tensor(counts, dtype=torch.int32, device=dev)
    hw = torch.tensor(kat["roiout/sizes"], dtype=torch.int32, device=dev)
    sc = t(kat["roiout/scales"].astype(np.float32)) if tag == "roiout_scaled" else None
    rp = L.vk_roi_params()
    thr = kat["roiout/nms_thresh"].tolist()
    rp.num_nms_thresh = len(thr)
    for i, v in enumerate(thr):
        rp.nms_thresh[i] = v
    rp.min_detections, rp.max_detections = 6, 8
    D = 8
    bufs = dict(obj_ids=torch.zeros((N, D), dtype=torch.int64, device=dev), obj_probs=torch.zeros((N, D), device=dev),
                attr_ids=torch.zeros((N, D), dtype=torch.int64, device=dev), attr_probs=torch.zeros((N, D), device=dev),
                boxes=torch.zeros((N, D, 4), device=dev), preds_per_image=torch.zeros((N,), dtype=torch.int64, device=dev),
                roi_features=torch.zeros((N, D, Fd), device=dev))
    out = L.vk_outputs(*[bufs[k].data_ptr() for k in ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes",
                                                      "preds_per_image", "roi_features")])
    keep = torch.zeros((N, D), dtype=torch.int64, device=dev)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    L.call("vk_roi_outputs", G.P(obj), Cn + 1, G.P(attr), An + 1, G.P(bd), 4 * Cn, 0, G.P(pr), G.P(cn), G.P(ft), Fd,
           N, R, Cn, An, G.P(hw), G.P(sc), (C.c_float * 4)(10.0, 10.0, 5.0, 5.0), C.byref(rp), C.byref(out),
           G.P(keep), G.P(flag), G.stream())
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ppi = bufs["preds_per_image"].cpu().tolist()
    for i in range(N):
        n = len(kat[f"{tag}/classes_{i}"])
        assert ppi[i] == n
        np.testing.assert_array_equal(bufs["obj_ids"][i, :n].cpu().numpy(), kat[f"{tag}/classes_{i}"])
        np.testing.assert_array_equal(bufs["attr_ids"][i, :n].cpu().numpy(), kat[f"{tag}/attrs_{i}"])
        np.testing.assert_array_equal(bufs["roi_features"][i, :n].cpu().numpy(), kat[f"{tag}/feats_{i}"])
        assert G.rel_err(bufs["obj_probs"][i, :n].cpu(), kat[f"{tag}/probs_{i}"]) <= 2e-6
        assert G.rel_err(bufs["attr_probs"][i, :n].cpu(), kat[f"{tag}/attr_probs_{i}"]) <= 2e-6
        assert G.rel_err(bufs["boxes"][i, :n].cpu(), kat[f"{tag}/boxes_{i}"]) <= 2e-6
        assert (bufs["roi_features"][i, n:] == 0).all() and (bufs["boxes"][i, n:] == 0).all()


DYNAMIC_TAIL_CASES = [
    ("panel 3x3", "VK_PANEL_DYNAMIC", (5400, 14, 14, 512, 512, 3, 2, 2)),        # 7350 tiles of 288 pixels x 2 column tiles
    ("gemm4 1x1", "VK_GEMM4_DYNAMIC", (5400, 14, 14, 1024, 512, 1, 0, 1)),       # 8270 tiles on 256 persistent workgroups
]


def dynamic_tail_geom(shape):
    N, H, W, cin, cout, k, pad, dil = shape
    return dict(N=N, H=H, W=W, cin=cin, cout=cout, k=k, pad=pad, dil=dil, relu=1)


@pytest.mark.parametrize("name,switch,shape", DYNAMIC_TAIL_CASES)
def test_dynamic_tile_tail_is_bit_identical(monkeypatch, name, switch, shape):
    """Long launches hand their last tiles out through an atomic counter (the XCDs of a chip differ in speed).  Which workgroup
    computes a tile must not change a bit: the same launch with every tile static, twice with the tail (the hand-out order differs
    from run to run), at a size that has a tail."""
    N, H, W, cin, cout, k, pad, dil = shape
    g = np.random.Generator(np.random.PCG64(3))
    w = (g.standard_normal((cout, cin, k, k)) * (2.0 / (cin * k * k)) ** 0.5).astype(np.float32)
    wd, bd = G.pack_conv(w, None, g.standard_normal(cout).astype(np.float32) * 0.1, L.VK_F16)
    torch.manual_seed(1)
    x = torch.randn((N, H, W, cin), device=G.DEV).half()

    def run():
        y = torch.full((N, H, W, cout), float("nan"), dtype=torch.float16, device=G.DEV)
        G.launch("vk_conv2d", G.P(x), N, H, W, cin, G.P(wd), G.P(bd), None, G.P(y), cout, cout, k, k, 1, pad, dil, 1, 1, L.VK_F16, L.VK_F16,
                 G.stream(), expect_route=name.split()[0])
        torch.cuda.synchronize()
        return y
    monkeypatch.setenv(switch, "0")
    ref = run()
    assert torch.isfinite(ref).all()
    monkeypatch.delenv(switch)
    for _ in range(2):
        assert torch.equal(run(), ref), name


def route_plan():
    """(label, environment, gpu_util.conv_route arguments, kernel) of every run above that names its kernel: what the GPU
    tests assert launch by launch, as a table the CPU suite checks against the dispatcher (tests/test_abi.py)."""
    f16, f32 = L.VK_F16, L.VK_F32
    for dt in (f32, f16):
        for c in CONV_CASES:
            for env, r in conv_legs(c, dt):
                yield f"test_conv[{c[0]}-{dt}]", env, conv_geom(c, dt), r
            if c[0].startswith("panel_") and dt == f16:
                assert panel_mi9_legal(c[3], c[9]), c[0]
                for e, r in PANEL_FORM_LEGS:
                    yield f"test_conv[{c[0]}-form]", dict(conv_legs(c, dt)[0][0], **e), conv_geom(c, dt), r
        for c in GROUPED_CASES:
            for env, r in grouped_legs(c, dt):
                yield f"test_grouped_conv[{c[0]}-{dt}]", env, grouped_geom(c, dt), r
    for c in BLK_CASES:
        for on, r in BLK_LEGS:
            yield f"test_conv3x3_blk_kernel[{c[0]}]", {"VK_CONV3X3_BLK": on}, blk_geom(c), r
    for c in DUAL_CASES:
        for env, r in dual_legs(*c):
            yield f"test_conv1x1_dual[{c}]", env, dual_geom(*c), r
    for c in MEANPOOL_CASES:
        for env, n, r in meanpool_legs(*c):
            yield f"test_conv1x1_meanpool[{c}]", env, meanpool_geom(n, *c[1:]), r
    for ws, r in NONFINITE_LEGS.items():
        yield f"test_conv1x1_meanpool_nonfinite[{ws}]", {"VK_CONV_WS": ws}, meanpool_geom(*NONFINITE_SHAPE), r
    for kernel in SCALE_KERNELS:
        yield f"test_conv_reproducible_at_scale[{kernel}]", scale_env(kernel), scale_geom(kernel), kernel
    for env, r in ONE_BY_ONE_LEGS:
        yield "test_conv_1x1_kernels_bit_identical", env, ONE_BY_ONE_GEOM, r
    for c in WS_CASES:
        for ws, waves, r in WS_LEGS:
            yield f"test_conv_ws_kernel_bit_identical[{c}]", {"VK_CONV_WS": ws, "VK_WS_WAVES": waves}, ws_geom(*c), r
    for c in WS_STRIDED_CASES:
        for sw, r in ws_strided_legs(*c):
            yield f"test_conv_ws_strided_bit_identical[{c}]", {"VK_WS_STRIDED": sw}, ws_strided_geom(*c), r
    for c in GEMM4_CASES:
        for g4, duo, r in GEMM4_LEGS:
            yield f"test_conv_gemm4_kernel_bit_identical[{c}]", {"VK_CONV_GEMM4": g4, "VK_CONV_DUO": duo}, gemm4_geom(*c), r
    for c in GEMM4_MANY_CASES:
        for g4, r in gemm4_many_legs(*c):
            yield f"test_conv_gemm4_many_tiles_per_workgroup[{c}]", {"VK_CONV_GEMM4": g4}, gemm4_many_geom(*c), r
    yield "test_conv_bias_f32_out", {}, F32OUT_GEOM, "generic"
    for name, switch, shape in DYNAMIC_TAIL_CASES:
        for env in ({switch: "0"}, {}):
            yield f"test_dynamic_tile_tail_is_bit_identical[{name}]", env, dynamic_tail_geom(shape), name.split()[0]
