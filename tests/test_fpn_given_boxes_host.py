"""CPU (-m "not gpu"): the host side of region features for caller-supplied boxes on the FPN detector -- the argument
checks of the two stage-level entry points (vk_given_boxes_ingest, vk_given_box_outputs), which run before any HIP call,
and the errors FRCNNFPN.forward raises before it enqueues anything."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import fpn_config
from vltk_amd.frcnn import MAX_GIVEN_BOXES
from vltk_amd.frcnn_fpn import FRCNNFPN

FAKE = 0x1000            # never dereferenced: every check below runs before the device


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_entry_points_are_exported(lib):
    for name in ("vk_given_boxes_ingest", "vk_given_box_outputs"):
        assert name in L.SIGNATURES and hasattr(lib, name)


def _ingest(N=2, B=4, boxes=FAKE, counts=FAKE, hw=FAKE, prop=FAKE, rois=FAKE, levels=FAKE, lo=2, hi=5, flag=FAKE):
    L.call("vk_given_boxes_ingest", boxes, counts, hw, None, N, B, prop, rois, levels, lo, hi, 224.0, 4, flag, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(boxes=None), "null"), (dict(counts=None), "null"), (dict(hw=None), "null"), (dict(prop=None), "null"),
    (dict(rois=None), "null"), (dict(flag=None), "null"),
    (dict(N=0), "N=0"), (dict(N=-1), "N=-1"), (dict(B=0), "B=0"), (dict(B=-2), "B=-2"),
    (dict(B=MAX_GIVEN_BOXES + 1), "B=1025"),
    (dict(lo=5, hi=2), "min_level"),
])
def test_ingest_rejects_before_launch(lib, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _ingest(**kw)
    assert msg in lib.vk_last_error().decode()


def test_ingest_without_levels_skips_the_level_rule_check(lib):
    # levels NULL is the C4 form: min/max level are not used, so only the shape checks apply
    with pytest.raises(ValueError, match="B=0"):
        _ingest(levels=None, lo=5, hi=2, B=0)


def _outputs(N=2, B=4, F=1024, ptrs=(FAKE,) * 8, out=(FAKE * 16,) * 7, use_out=True):
    o = L.vk_outputs(*out)
    L.call("vk_given_box_outputs", *ptrs[:7], ptrs[7], F, N, B, C.byref(o) if use_out else None, None)


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 5, 7])          # 6 is scales_yx: NULL means no scales
def test_outputs_rejects_null_inputs(lib, i):
    ptrs = [FAKE * 16] * 8
    ptrs[i] = None
    with pytest.raises(ValueError, match="null argument"):
        _outputs(ptrs=ptrs)


def test_outputs_rejects_null_block_and_arrays(lib):
    with pytest.raises(ValueError, match="null argument"):
        _outputs(ptrs=(FAKE * 16,) * 8, use_out=False)
    for i in range(7):
        out = [FAKE * 16] * 7
        out[i] = 0
        with pytest.raises(ValueError, match="null output array"):
            _outputs(ptrs=(FAKE * 16,) * 8, out=out)


@pytest.mark.parametrize("kw,msg", [
    (dict(N=0), "N=0"), (dict(B=0), "B=0"), (dict(B=1025), "B=1025"),
    (dict(F=0), "F=0"), (dict(F=1022), "F=1022"), (dict(F=-4), "F=-4"),
])
def test_outputs_rejects_sizes(lib, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _outputs(ptrs=(FAKE * 16,) * 8, **kw)


def test_outputs_rejects_unaligned_rows(lib):
    ptrs = [FAKE * 16] * 8
    ptrs[7] = FAKE * 16 + 4                                         # feat
    with pytest.raises(ValueError, match="16-byte aligned"):
        _outputs(ptrs=ptrs)
    out = [FAKE * 16] * 7
    out[6] = FAKE * 16 + 8                                          # roi_features
    with pytest.raises(ValueError, match="16-byte aligned"):
        _outputs(ptrs=(FAKE * 16,) * 8, out=out)


# ---- FRCNNFPN.forward(proposals=...): every error before anything is enqueued ----------------------------------------
def _host_only_model():
    """An FRCNNFPN without weights or a device whose device stages fail the test if they are reached."""
    m = object.__new__(FRCNNFPN)
    m.config, m.training, m._finalized, m._timing, m._stages = fpn_config(), False, True, None, {}
    m.device = torch.device("cpu")

    def launched(*a, **k):
        pytest.fail("a device stage was reached")
    m._bottom_up = m.neck = m._box_head = m._predictor = launched
    return m


def test_fpn_model_accepts_proposals():
    assert FRCNNFPN.given_boxes is True


def test_fpn_forward_errors_before_enqueue():
    m = _host_only_model()
    x, hw = torch.zeros(2, 3, 64, 64), torch.tensor([[64, 64]] * 2)
    boxes = [np.zeros((3, 4), np.float32), np.zeros((1, 4), np.float32)]
    with pytest.raises(ValueError, match="ignorey"):
        m(x, hw, proposals=boxes, ignorey=[np.zeros((1, 2))] * 2, scales_yx=torch.ones(2, 2))
    with pytest.raises(ValueError, match="2 images"):
        m(x, hw, proposals=boxes[:1])
    with pytest.raises(ValueError, match="must be \\[K, 4\\]"):
        m(x, hw, proposals=[np.zeros((3, 5)), np.zeros((1, 4))])
    with pytest.raises(ValueError, match="at most 1024"):
        m(x, hw, proposals=[np.zeros((MAX_GIVEN_BOXES + 1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError, match="at most 1024"):
        m(x, hw, proposals=torch.zeros(2, MAX_GIVEN_BOXES + 1, 4))
    with pytest.raises(ValueError, match="max_detections=2"):
        m(x, hw, proposals=boxes, max_detections=2)
    with pytest.raises(ValueError, match="image_shapes"):
        m(x, torch.tensor([[64, 64], [0, 64]]), proposals=boxes)
    m.train()
    with pytest.raises(NotImplementedError):
        m(x, hw, proposals=boxes)
