"""-m gpu: the fragment-window schedule of the 3x3 panel kernel's 512 x 128 phase tile (csrc/conv3x3_panel.hip, REUSE;
DESIGN.md 6f) against the schedule in which every tap reads its own eight fragments (VK_PANEL_REUSE=0).

Nothing here has a tolerance.  The two schedules issue the same matrix instructions on the same operands in the same order
(channel stage major, tap minor), so the outputs are torch.equal on the f16 bits.  The route, vk_panel_phase_tile_rows and
vk_panel_phase_reuse -- the functions the launcher itself reads -- are asserted around every launch, so a test cannot pass on
the wrong schedule.  Equality of the two schedules could hide a bug they share, so two shapes also run on the integer data
of tests/exact_util.py against float64 arithmetic rounded once, and the small model runs with the switch on and off.

The route takes Cin >= 128 only (conv3x3_panel_eligible), so a single stage pair that is also the last (Cin = 64) cannot
be launched: 128 channels, one looped pair and the final one, is the minimum.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_util as X                         # noqa: E402
import test_gpu_conv_exact as E                # noqa: E402
import test_gpu_panel_tall as T                # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

# (N, H, W, Cin, Cout), all 3x3, dilation 2, pad 2: the smallest shapes at which the window can go wrong
OVERLAP = (16, 4, 4, 128, 256)                 # W/2 = 2: the windows of the three dy overlap
SIX_WIDE = (16, 8, 12, 128, 256)               # W/2 = 6

SWEPT = [(T.ONE_GROUP, res, relu) for res in (False, True) for relu in (0, 1)]       # W/2 = 7, wave row blocks beyond M
SINGLE = [(s, True, 1) for s in (T.TWO_GROUPS,      # a tile across two groups
                                 T.NON_SQUARE,      # W/2 = 5, ragged second tile
                                 OVERLAP, T.CENTRE_ONLY,      # W/2 = 2; W/2 = 1, centre tap only, every panel piece clamped
                                 SIX_WIDE,
                                 T.FOUR_COLUMNS,    # six channel stages (handover at tap 8 in both parities), four column tiles
                                 T.REMAINDER)]      # the 16 + 4 remainder split


def _queries(shape):
    N, H, W, _, cout = shape
    lib = L.load()
    return lib.vk_panel_phase_tile_rows(N, H, W, 2, cout), lib.vk_panel_phase_reuse(N, H, W, 2, cout)


def _clear(monkeypatch):
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_DYNAMIC", "VK_PANEL_REUSE", "VK_CONV3X3_PANEL"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", SWEPT + SINGLE, ids=T._id)
def test_window_equals_read_per_tap(case, monkeypatch):
    shape, res, relu = case
    _clear(monkeypatch)
    monkeypatch.setenv("VK_PANEL_REUSE", "0")
    assert _queries(shape) == (512, 0)
    want = T._launch(shape, res, relu)             # (asserts the route: expect_route="panel")
    monkeypatch.delenv("VK_PANEL_REUSE")
    assert _queries(shape) == (512, 1)
    got = T._launch(shape, res, relu)
    assert _queries(shape) == (512, 1)
    T._same_bits(T._id(case), got, want)


def test_dynamic_tail_same_bits(monkeypatch):
    """4116 tiles: the last sixteenth is drawn from the counter.  Static tiles, the default and VK_PANEL_REUSE=0 give the
    same tensor."""
    _clear(monkeypatch)
    N, H, W, _, cout = T.TAIL
    assert -(-N * H * W // 512) * (cout // 128) >= 4096
    monkeypatch.setenv("VK_PANEL_DYNAMIC", "0")
    assert _queries(T.TAIL) == (512, 1)
    want = T._launch(T.TAIL, True, 1)
    monkeypatch.delenv("VK_PANEL_DYNAMIC")
    assert _queries(T.TAIL) == (512, 1)
    got = T._launch(T.TAIL, True, 1)
    T._same_bits("dynamic tail, window", got, want)
    del got
    monkeypatch.setenv("VK_PANEL_REUSE", "0")
    assert _queries(T.TAIL) == (512, 0)
    per_tap = T._launch(T.TAIL, True, 1)
    T._same_bits("dynamic tail, read per tap", per_tap, want)


ANCHORS = [X.Case("panel_reuse/16x14x14_512", "panel", "conv", 16, 14, 14, 128, 512, 3, 1, 2, 2, res=True, relu=1),
           X.Case("panel_reuse/16x4x4", "panel", "conv", 16, 4, 4, 128, 256, 3, 1, 2, 2, res=True, relu=1)]


@pytest.mark.parametrize("case", ANCHORS, ids=[c.name for c in ANCHORS])
def test_window_exact_on_integer_data(case, monkeypatch):
    """The absolute anchor: integer data, float64 arithmetic rounded once, whole-tensor equality (tests/exact_util.py)."""
    _clear(monkeypatch)
    lib = L.load()
    assert lib.vk_panel_phase_images(case.N, case.H, case.W, case.dil) == case.N
    assert lib.vk_panel_phase_tile_rows(case.N, case.H, case.W, case.dil, case.cout) == 512
    assert lib.vk_panel_phase_reuse(case.N, case.H, case.W, case.dil, case.cout) == 1
    got, want = E.run_case(case, monkeypatch)
    assert lib.vk_panel_phase_reuse(case.N, case.H, case.W, case.dil, case.cout) == 1
    E.assert_exact(case, got, want)


STAGES = ("res4", "pooled", "feature_pooled", "obj_logits", "attr_logits")


def test_model_same_bits(monkeypatch):
    """The small model at 2 x 32 = 64 RoIs (four groups of 16): every stage and output with the window equals the same with
    VK_PANEL_REUSE=0 (the switch is re-read per launch)."""
    _clear(monkeypatch)
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

    monkeypatch.setenv("VK_PANEL_REUSE", "0")
    ref, ref_st = run()
    rows = ref_st["pooled"].shape[0]
    assert rows == 64 and L.load().vk_panel_phase_reuse(rows, 14, 14, 2, 512) == 0
    monkeypatch.delenv("VK_PANEL_REUSE")
    assert L.load().vk_panel_phase_tile_rows(rows, 14, 14, 2, 512) == 512 and L.load().vk_panel_phase_reuse(rows, 14, 14, 2, 512) == 1
    got, got_st = run()
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["feature_pooled"].float().abs().max()) > 0
