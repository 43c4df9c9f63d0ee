"""-m gpu: the phase-interleaved form of the 3x3 panel kernel (csrc/conv3x3_panel.hip; dilation 2, even H, even
W <= 14, whole groups of 16 images) against the plain form of the same kernel (VK_PANEL_PHASE=0).

Nothing here has a tolerance.  The two forms sum the same products in the same order (channel stage major, tap minor); the
taps the phase form leaves out contributed exact zeros; a row's bits do not depend on its place in a tile: the outputs are
torch.equal.  Equality of the two forms could hide a bug they share, so two shapes also run on the integer data of
tests/exact_util.py against float64 arithmetic rounded once; and the small model runs with the switch on and off.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_util as X                         # noqa: E402
import gpu_util as G                           # noqa: E402
import test_gpu_conv_exact as E                # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

F16 = L.VK_F16

# (N, H, W, Cin, Cout), all 3x3, dilation 2, pad 2
ONE_GROUP = (16, 14, 14, 128, 256)             # M = 3136 = 12.25 tiles: crosses every phase boundary, ends on a ragged tile
TWO_GROUPS = (32, 14, 14, 128, 256)            # a tile straddles two groups
NON_SQUARE = (16, 6, 10, 128, 256)             # an H / W or y / x mix-up shows here
CENTRE_ONLY = (16, 2, 2, 128, 256)             # every non-centre tap is invalid
TWO_COLUMNS = (48, 14, 14, 192, 512)           # two column tiles, six channel stages
REMAINDER = (20, 14, 14, 128, 256)             # 16 images in the phase form, 4 in a second, plain launch
TOO_FEW = (8, 14, 14, 128, 256)                # fewer than 16 images: the plain form alone

SWEPT = [(s, res, relu, dyn) for s in (ONE_GROUP, TWO_GROUPS) for res in (False, True) for relu in (0, 1) for dyn in ("1", "0")]
SINGLE = [(s, True, 1, "1") for s in (NON_SQUARE, CENTRE_ONLY, TWO_COLUMNS, REMAINDER, TOO_FEW)]


def _id(c):
    (n, h, w, ci, co), res, relu, dyn = c
    return f"{n}x{h}x{w}_{ci}_{co}-res{int(res)}-relu{relu}-dyn{dyn}"


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Seeded normal f16 x (NHWC), packed w and bias, residual rows: made once per shape and never written."""
    N, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + cin + cout)
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


@pytest.mark.parametrize("case", SWEPT + SINGLE, ids=_id)
def test_phase_form_equals_plain_form(case, monkeypatch):
    shape, res, relu, dyn = case
    N, H, W = shape[:3]
    monkeypatch.setenv("VK_PANEL_DYNAMIC", dyn)
    monkeypatch.setenv("VK_PANEL_PHASE", "0")
    assert L.load().vk_panel_phase_images(N, H, W, 2) == 0
    want = _launch(shape, res, relu)
    monkeypatch.delenv("VK_PANEL_PHASE")
    assert L.load().vk_panel_phase_images(N, H, W, 2) == N // 16 * 16      # (0 for TOO_FEW: the plain form against itself)
    got = _launch(shape, res, relu)
    assert not bool(torch.isnan(want).any()) and float(want.float().abs().max()) > 0
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = (got.view(torch.int16) != want.view(torch.int16))
        rows = bad.any(dim=1).nonzero().flatten()
        raise AssertionError(f"{_id(case)}: {int(bad.sum())} of {bad.numel()} outputs differ between the forms; rows "
                             f"{rows[:12].tolist()}... ({rows.numel()} of {bad.shape[0]})")


ANCHORS = [X.Case("panel_phase/16x14x14", "panel", "conv", 16, 14, 14, 128, 256, 3, 1, 2, 2, res=True, relu=1),
           X.Case("panel_phase/16x6x10", "panel", "conv", 16, 6, 10, 128, 256, 3, 1, 2, 2, res=True, relu=1)]


@pytest.mark.parametrize("case", ANCHORS, ids=[c.name for c in ANCHORS])
def test_phase_form_exact_on_integer_data(case, monkeypatch):
    """The absolute anchor: integer data, float64 arithmetic rounded once, whole-tensor equality (tests/exact_util.py)."""
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    assert L.load().vk_panel_phase_images(case.N, case.H, case.W, case.dil) == case.N
    got, want = E.run_case(case, monkeypatch)
    E.assert_exact(case, got, want)


STAGES = ("res4", "pooled", "feature_pooled", "obj_logits", "attr_logits")


def test_model_same_bits(monkeypatch):
    """The small model at 2 x 32 = 64 RoIs (four groups of 16): every stage and output with the form on equals the same with
    VK_PANEL_PHASE=0 (the switch is re-read per launch)."""
    cfg = vg_c4_config(post_nms_topk=32, detections=12)
    sd = make_state_dict(cfg, seed=1234)
    shapes = torch.tensor([[160, 224], [144, 200]])
    x = synthetic_images(2, 160, 224, seed=21)
    for i, (hh, ww) in enumerate(shapes.tolist()):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    x = torch.from_numpy(x).cuda()
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()

    def run():
        out = {k: v.clone() for k, v in m.forward_async(images=x, image_shapes=shapes).wait_raw().items()}
        return out, {s: m.get_stage(s).clone() for s in STAGES}

    monkeypatch.setenv("VK_PANEL_PHASE", "0")
    ref, ref_st = run()
    monkeypatch.delenv("VK_PANEL_PHASE")
    rows = ref_st["pooled"].shape[0]
    assert rows % 16 == 0 and L.load().vk_panel_phase_images(rows, 14, 14, 2) == rows
    got, got_st = run()
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["feature_pooled"].float().abs().max()) > 0
