"""-m gpu: option "head_dedupe_taps" (Res5 block 0's GEMMs and conv1 of block 1 over the distinct nine-window neighbourhoods,
DESIGN.md 6h) on the small model of the dedupe tests: 1 against 0, every output and the stages "feature_pooled", "obj_logits",
"attr_logits" torch.equal, and the read-only counter "tap_dedupe_chunks" saying which chunks took the path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from roi_dedupe_util import crafted_boxes   # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402

STAGES = ("feature_pooled", "obj_logits", "attr_logits")
COUNTERS = ("dedupe_chunks", "indexed_chunks", "tap_dedupe_chunks")
SHAPES = [[160, 224], [144, 200]]


@pytest.fixture(autouse=True)
def small_grids(monkeypatch):
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_CONV3X3_PANEL", "VK_CONV_WS", "VK_WS_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VK_CONV_GEMM4", "2")        # conv_gemm4, and with it the dedupe path, also at the few tiles of these shapes


@pytest.fixture(scope="module")
def images():
    x = synthetic_images(2, 160, 224, seed=21)
    for i, (hh, ww) in enumerate(SHAPES):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    return torch.from_numpy(x).cuda()


def build(topk, precision="fp16"):
    cfg = vg_c4_config(post_nms_topk=topk, detections=12)
    return FRCNN(cfg, precision=precision).load_state_dict(make_state_dict(cfg, seed=1234)).eval()


@pytest.fixture(scope="module")
def model32():
    return build(32)


def run(m, taps, **kw):
    m.set_option("head_dedupe_taps", taps)
    n0 = [m.get_option(k) for k in COUNTERS]
    out = {k: v.clone() for k, v in m.forward_async(**kw).wait_raw().items()}
    st = {s: m.get_stage(s).clone() for s in STAGES}
    return out, st, tuple(m.get_option(k) - a for k, a in zip(COUNTERS, n0))


def on_against_off(m, **kw):
    ref, ref_st, n_ref = run(m, 0, **kw)
    got, got_st, n_got = run(m, 1, **kw)
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["feature_pooled"].float().abs().max()) > 0
    return n_ref, n_got


def test_default_and_range():
    m = build(30)
    assert m.get_option("head_dedupe_taps") == 1 and m.get_option("tap_dedupe_chunks") == 0
    m.set_option("head_dedupe_taps", 0)
    assert m.get_option("head_dedupe_taps") == 0
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="head_dedupe_taps must be 0 or 1"):
            m.set_option("head_dedupe_taps", bad)
    with pytest.raises(ValueError, match="unknown option 'tap_dedupe_chunks'"):
        m.set_option("tap_dedupe_chunks", 1)


def test_one_chunk(images, model32):
    """2 x 32 = 64 RoIs, one chunk of four groups of 16."""
    m = model32
    n_ref, n_got = on_against_off(m, images=images, image_shapes=torch.tensor(SHAPES))
    assert n_ref == (1, 1, 0) and n_got == (1, 1, 1)
    hv = m.get_stage("head_neighbourhoods")
    hw = m.get_stage("head_windows")
    print(f"64 RoIs: {64 * 196} bins, {int(hw[0])} windows, {int(hv[0])} neighbourhoods")
    assert int(hw[0]) <= int(hv[0]) < 64 * 196


def test_chunk_not_of_whole_groups(images):
    """2 x 36 = 72 RoIs in chunks of 40: the chunk of 40 (conv2 not indexed) runs today's path, the tail of 32 the new one."""
    m = build(36)
    m.set_option("head_chunk", 40)
    n_ref, n_got = on_against_off(m, images=images, image_shapes=torch.tensor(SHAPES))
    assert n_ref == (2, 1, 0) and n_got == (2, 1, 1)


def test_today_s_path_where_the_conditions_fail(images, model32):
    """Strict fp32, head_streams = 2 and head_dedupe = 0: the counter stays 0 and the outputs are those of head_dedupe_taps = 0."""
    kw = dict(images=images, image_shapes=torch.tensor(SHAPES))
    m32 = build(32, "fp32")
    assert m32.get_option("head_dedupe_taps") == 1
    assert on_against_off(m32, **kw) == ((0, 0, 0), (0, 0, 0))
    m = model32
    for key, value, back in (("head_streams", 2, 1), ("head_dedupe", 0, 1)):
        m.set_option(key, value)
        try:
            n_ref, n_got = on_against_off(m, **kw)
        finally:
            m.set_option(key, back)
        assert n_ref == (0, 0, 0) and n_got == (0, 0, 0), key
    assert on_against_off(m, **kw)[1] == (1, 1, 1)


def test_given_boxes(images, model32):
    """crafted_boxes as caller-supplied proposals: 16 per image, two groups of 16 in one chunk."""
    m = model32
    boxes = [np.ascontiguousarray(crafted_boxes([hw])[:, 1:]) for hw in ((10, 14), (9, 13))]      # (the entry point clips them to the image)
    n_ref, n_got = on_against_off(m, images=images, image_shapes=torch.tensor(SHAPES), proposals=boxes)
    assert n_ref == (1, 1, 0) and n_got == (1, 1, 1)
