"""-m gpu: the 512-row x 128-column tile of the 3x3 panel kernel's phase form (csrc/conv3x3_panel.hip) against
the 256 x 256 tile of the same form (VK_PANEL_TALL=0).

Nothing here has a tolerance.  A row's bits depend on neither its tile nor the workgroup that computed it: every element sums
the same products in the same order (channel stage major, tap minor), so the outputs are torch.equal on the f16 bits.
vk_panel_phase_tile_rows, the function the launcher itself reads, is asserted around every launch, so a test cannot pass on
the wrong shape.  Equality of the two shapes could hide a bug they share, so two shapes also run on the integer data of
tests/exact_util.py against float64 arithmetic rounded once; the dynamic tail runs once at a size that engages it.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_util as X                         # noqa: E402
import gpu_util as G                           # noqa: E402
import test_gpu_conv_exact as E                # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

F16 = L.VK_F16

# (N, H, W, Cin, Cout), all 3x3, dilation 2, pad 2
ONE_GROUP = (16, 14, 14, 128, 256)             # M = 3136 = 6.125 row tiles: the last tile has three of four wave row blocks beyond M; two column tiles
TWO_GROUPS = (32, 14, 14, 128, 256)            # a tile straddles two groups
NON_SQUARE = (16, 6, 10, 128, 256)             # halo 96; the second tile is ragged
CENTRE_ONLY = (16, 2, 2, 128, 256)             # M = 64: one tile, every panel piece clamped, centre tap only
FOUR_COLUMNS = (48, 14, 14, 192, 512)          # four column tiles, six channel stages
REMAINDER = (20, 14, 14, 128, 256)             # 16 images in tall tiles, 4 in a second, plain launch
TAIL = (2688, 14, 14, 128, 512)                # M = 526 848: 1029 x 4 = 4116 tiles >= 4096, the dynamic tail engages

SWEPT = [(s, res, relu) for s in (ONE_GROUP, TWO_GROUPS) for res in (False, True) for relu in (0, 1)]
SINGLE = [(s, True, 1) for s in (NON_SQUARE, CENTRE_ONLY, FOUR_COLUMNS, REMAINDER)]


def _id(c):
    (n, h, w, ci, co), res, relu = c
    return f"{n}x{h}x{w}_{ci}_{co}-res{int(res)}-relu{relu}"


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Seeded normal f16 x (NHWC), packed w and bias, residual rows: made once per shape and never written."""
    N, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(7000 + 1000 * N + 100 * H + 10 * W + cin + cout)
    x = torch.randn((N, H, W, cin), generator=g).to(torch.float16).to(G.DEV)
    w = (torch.randn((cout, cin, 3, 3), generator=g) * 0.05).numpy().astype(np.float32)
    bias = torch.randn((cout,), generator=g).numpy().astype(np.float32)
    res = torch.randn((N * H * W, cout), generator=g).to(torch.float16).to(G.DEV)
    wd, bd = G.pack_conv(w, None, bias, F16)
    return x, wd, bd, res


def _launch(shape, res, relu):
    N, H, W, cin, cout = shape
    x, wd, bd, rd = _data(shape)
    y = torch.full((N * H * W, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    G.launch("vk_conv2d", G.P(x), N, H, W, cin, G.P(wd), G.P(bd), G.P(rd if res else None), G.P(y), cout, cout, 3, 3, 1, 2, 2, 1, relu,
             F16, F16, G.stream(), expect_route="panel")
    torch.cuda.synchronize()
    return y


def _same_bits(what, got, want):
    assert not bool(torch.isnan(want).any()) and float(want.float().abs().max()) > 0
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = (got.view(torch.int16) != want.view(torch.int16))
        rows = bad.any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ; rows {rows[:12].tolist()}... "
                             f"({rows.numel()} of {bad.shape[0]})")


def _tile_rows(shape):
    N, H, W, _, cout = shape
    return L.load().vk_panel_phase_tile_rows(N, H, W, 2, cout)


@pytest.mark.parametrize("case", SWEPT + SINGLE, ids=_id)
def test_tall_tile_equals_wide_tile(case, monkeypatch):
    shape, res, relu = case
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    monkeypatch.delenv("VK_PANEL_DYNAMIC", raising=False)
    monkeypatch.setenv("VK_PANEL_TALL", "0")
    assert _tile_rows(shape) == 256
    want = _launch(shape, res, relu)
    monkeypatch.delenv("VK_PANEL_TALL")
    assert _tile_rows(shape) == 512
    got = _launch(shape, res, relu)
    _same_bits(_id(case), got, want)


def test_dynamic_tail_same_bits(monkeypatch):
    """4116 tiles in either shape: the last sixteenth is drawn from the counter.  Static tiles, the tall default and the wide
    shape give the same tensor."""
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    monkeypatch.delenv("VK_PANEL_TALL", raising=False)
    N, H, W, _, cout = TAIL
    assert -(-N * H * W // 512) * (cout // 128) >= 4096 and -(-N * H * W // 256) * (cout // 256) >= 4096
    monkeypatch.setenv("VK_PANEL_DYNAMIC", "0")
    assert _tile_rows(TAIL) == 512
    want = _launch(TAIL, True, 1)
    monkeypatch.delenv("VK_PANEL_DYNAMIC")
    assert _tile_rows(TAIL) == 512
    got = _launch(TAIL, True, 1)
    _same_bits("dynamic tail, 512 x 128", got, want)
    del got
    monkeypatch.setenv("VK_PANEL_TALL", "0")
    assert _tile_rows(TAIL) == 256
    wide = _launch(TAIL, True, 1)
    _same_bits("dynamic tail, 256 x 256", wide, want)


ANCHORS = [X.Case("panel_tall/16x14x14_512", "panel", "conv", 16, 14, 14, 128, 512, 3, 1, 2, 2, res=True, relu=1),
           X.Case("panel_tall/16x6x10", "panel", "conv", 16, 6, 10, 128, 256, 3, 1, 2, 2, res=True, relu=1)]


@pytest.mark.parametrize("case", ANCHORS, ids=[c.name for c in ANCHORS])
def test_tall_tile_exact_on_integer_data(case, monkeypatch):
    """The absolute anchor: integer data, float64 arithmetic rounded once, whole-tensor equality (tests/exact_util.py)."""
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    monkeypatch.delenv("VK_PANEL_TALL", raising=False)
    assert L.load().vk_panel_phase_images(case.N, case.H, case.W, case.dil) == case.N
    assert L.load().vk_panel_phase_tile_rows(case.N, case.H, case.W, case.dil, case.cout) == 512
    got, want = E.run_case(case, monkeypatch)
    E.assert_exact(case, got, want)
