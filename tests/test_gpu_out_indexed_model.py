"""-m gpu: conv2 of Res5 block 0 storing the distinct neighbourhoods' rows itself (the panel kernel's indexed output rows,
DESIGN.md 6i) on the small model of tests/test_gpu_tap_dedupe_model.py: the default against VK_PANEL_OUT_INDEXED=0 (re-read per
call: the dense conv2 and the row gather behind it), every output and the stages "feature_pooled", "obj_logits", "attr_logits"
torch.equal, and the read-only counter "out_indexed_chunks" saying which chunks took the path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from roi_dedupe_util import crafted_boxes   # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402

STAGES = ("feature_pooled", "obj_logits", "attr_logits")
COUNTERS = ("dedupe_chunks", "indexed_chunks", "tap_dedupe_chunks", "out_indexed_chunks")
SHAPES = [[160, 224], [144, 200]]
SWITCH = "VK_PANEL_OUT_INDEXED"


@pytest.fixture(autouse=True)
def small_grids(monkeypatch):
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", SWITCH, "VK_CONV3X3_PANEL", "VK_CONV_WS", "VK_WS_WAVES",
              "VK_HEAD_DEDUPE_TAPS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VK_CONV_GEMM4", "2")        # conv_gemm4, and with it the dedupe path, also at the few tiles of these shapes


@pytest.fixture(scope="module")
def images():
    x = synthetic_images(2, 160, 224, seed=21)
    for i, (hh, ww) in enumerate(SHAPES):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    return torch.from_numpy(x).cuda()


def build(topk):
    cfg = vg_c4_config(post_nms_topk=topk, detections=12)
    return FRCNN(cfg, precision="fp16").load_state_dict(make_state_dict(cfg, seed=1234)).eval()


@pytest.fixture(scope="module")
def model32():
    return build(32)


def run(m, **kw):
    n0 = [m.get_option(k) for k in COUNTERS]
    out = {k: v.clone() for k, v in m.forward_async(**kw).wait_raw().items()}
    st = {s: m.get_stage(s).clone() for s in STAGES}
    return out, st, tuple(m.get_option(k) - a for k, a in zip(COUNTERS, n0))


def on_against_off(m, monkeypatch, **kw):
    """(counters of the forward under VK_PANEL_OUT_INDEXED=0, counters of the default forward), the two held torch.equal."""
    monkeypatch.setenv(SWITCH, "0")
    ref, ref_st, n_ref = run(m, **kw)
    monkeypatch.delenv(SWITCH)
    got, got_st, n_got = run(m, **kw)
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["feature_pooled"].float().abs().max()) > 0
    assert n_ref[:3] == n_got[:3]                   # every other counter keeps its value, tap_dedupe_chunks among them
    return n_ref, n_got


def test_counter_is_read_only():
    m = build(30)
    assert m.get_option("out_indexed_chunks") == 0
    with pytest.raises(ValueError, match="unknown option 'out_indexed_chunks'"):
        m.set_option("out_indexed_chunks", 1)


def test_one_chunk(images, model32, monkeypatch):
    """2 x 32 = 64 RoIs, one chunk of four groups of 16."""
    n_ref, n_got = on_against_off(model32, monkeypatch, images=images, image_shapes=torch.tensor(SHAPES))
    assert n_ref == (1, 1, 1, 0) and n_got == (1, 1, 1, 1)
    hv = model32.get_stage("head_neighbourhoods")
    assert 0 < int(hv[0]) < 64 * 196                # (some row is stored nowhere)


def test_chunk_not_of_whole_groups(images, monkeypatch):
    """2 x 36 = 72 RoIs in chunks of 40: the chunk of 40 (conv2 in no indexed form) runs the old path, the tail of 32 the new one."""
    m = build(36)
    m.set_option("head_chunk", 40)
    n_ref, n_got = on_against_off(m, monkeypatch, images=images, image_shapes=torch.tensor(SHAPES))
    assert n_ref == (2, 1, 1, 0) and n_got == (2, 1, 1, 1)


def test_without_the_neighbourhood_path(images, model32, monkeypatch):
    """head_dedupe_taps = 0: conv2's output is the dense t2 of the fused GEMM, nothing to index; the counter stays 0."""
    m = model32
    m.set_option("head_dedupe_taps", 0)
    try:
        n_ref, n_got = on_against_off(m, monkeypatch, images=images, image_shapes=torch.tensor(SHAPES))
    finally:
        m.set_option("head_dedupe_taps", 1)
    assert n_ref == (1, 1, 0, 0) and n_got == (1, 1, 0, 0)


def test_given_boxes(images, model32, monkeypatch):
    """crafted_boxes as caller-supplied proposals: 16 per image, two groups of 16 in one chunk."""
    boxes = [np.ascontiguousarray(crafted_boxes([hw])[:, 1:]) for hw in ((10, 14), (9, 13))]      # (the entry point clips them to the image)
    n_ref, n_got = on_against_off(model32, monkeypatch, images=images, image_shapes=torch.tensor(SHAPES), proposals=boxes)
    assert n_ref == (1, 1, 1, 0) and n_got == (1, 1, 1, 1)
