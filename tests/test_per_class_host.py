"""CPU (-m "not gpu"): the host side of roi_outputs.selection = "per_class"  -- the tests' restatement
of the contract (tests/per_class_util.py) against the vectors made from the reference's own pieces
(tests/golden/e2e_per_class.npz, tools/gen_golden_per_class.py), the new C-ABI symbols, ROIOutputs' validation, the checks
the library makes before any HIP call, and the FPN detector's refusal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import fpn_config, vg_c4_config
from vltk_amd.frcnn import ROIOutputs
from vltk_amd.frcnn_fpn import FRCNNFPN

import per_class_util as PC

FAKE = 0x1000 * 16       # never dereferenced: every check below runs before the device


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_per_class.npz"))


def test_fixture_covers_the_three_count_regimes(golden):
    g = golden
    lo, hi = int(g["min_detections"]), int(g["max_detections"])
    counts = g["counts"]
    n_ge = np.asarray([[int((g[f"max_conf_{i}"].astype(np.float64) >= t).sum()) for i in range(2)] for t in g["score_thresh"]])
    assert ((n_ge < lo) & (counts == lo)).any(), "no image falls back to min_detections"
    assert ((n_ge > hi) & (counts == hi)).any(), "no image is capped at max_detections"
    assert ((n_ge == counts) & (counts > lo) & (counts < hi)).any(), "no image lies inside the bounds"
    # the generator asserted that 1e-5 perturbations of logits and deltas change no selected id or class
    assert g["perturbation"].tolist() == [1e-5, 6]
    assert min(float(g[f"cls_margin_{i}"].min()) for i in range(2)) > 1e-3


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales_yx"])
def test_restatement_reproduces_the_fixture(golden, scaled):
    """Per-class NMS runs class by class, so the rule over the stored class columns (every box's confidence class and its
    three best classes) gives the full rule's ids, classes and confidences: all exact, max_conf and boxes bit-equal."""
    g = golden
    cfg = vg_c4_config()
    w = cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS
    for ti, t in enumerate(g["score_thresh"].tolist()):
        for i in range(2):
            cols = g[f"class_cols_{i}"]
            sc = np.concatenate([g[f"scores_cols_{i}"], np.zeros((len(g[f"scores_cols_{i}"]), 1), np.float32)], 1)
            res = PC.select_image(sc, g[f"deltas_cols_{i}"], g[f"proposal_boxes_{i}"], g["shapes"][i], w, float(g["nms_thresh"]), t,
                                  int(g["min_detections"]), int(g["max_detections"]), g["scales_yx"][i] if scaled else None)
            k = int(g["counts"][ti][i])
            assert len(res["ids"]) == k, (t, i)
            np.testing.assert_array_equal(res["ids"].numpy(), g[f"keep_ids_{i}"][:k])
            np.testing.assert_array_equal(cols[res["classes"].numpy()], g[f"obj_ids_{i}"][:k])
            np.testing.assert_array_equal(res["probs"].numpy(), g[f"obj_probs_{i}"][:k])
            np.testing.assert_array_equal(res["max_conf"].numpy(), g[f"max_conf_{i}"])
            np.testing.assert_array_equal(res["boxes"].numpy(), g[f"boxes_scaled_{i}" if scaled else f"boxes_{i}"][:k])


def test_restatement_tie_and_no_survivor_rules():
    """Two identical boxes with identical scores: the lower row survives in every class, the other in none (confidence 0,
    class 0); equal scores across classes give the smaller class; the ranking breaks ties to the lower row."""
    props = np.asarray([[10, 10, 50, 50], [10, 10, 50, 50], [100, 100, 140, 150]], np.float32)
    scores = np.asarray([[0.4, 0.4, 0.2], [0.4, 0.4, 0.2], [0.4, 0.3, 0.3]], np.float32)
    deltas = np.zeros((3, 8), np.float32)
    r = PC.select_image(scores, deltas, props, (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3, 0.35, 0, 3)
    assert r["max_conf"].tolist() == pytest.approx([0.4, 0.0, 0.4]) and r["cls"].tolist() == [0, 0, 0]
    assert r["ids"].tolist() == [0, 2]
    r = PC.select_image(scores, deltas, props, (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3, 0.35, 3, 3)
    assert r["ids"].tolist() == [0, 2, 1] and r["probs"].tolist() == pytest.approx([0.4, 0.4, 0.0])
    r = PC.select_image(scores, deltas, props, (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3, 0.0, 5, 9)
    assert len(r["ids"]) == 3                                   # min_detections > R: every proposal, no more


def test_new_symbols_are_exported(lib):
    for name in ("vk_forward_begin_select", "vk_per_class_select", "vk_class_probs", "vk_class_boxes"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert (L.VK_SELECT_CLASS_MAX, L.VK_SELECT_PER_CLASS) == (0, 1)
    # int32 mode, (pad), double score_thresh, vk_roi_params -- and the pinned structs stay as they were
    assert C.sizeof(L.vk_select_params) == 8 + 8 + C.sizeof(L.vk_roi_params)
    assert L.vk_select_params.score_thresh.offset == 8 and L.vk_select_params.roi.offset == 16
    assert C.sizeof(L.vk_roi_params) == 8 + 8 * 8 + 8 and lib.vk_version() == 1


def _roi_outputs(**kw):
    ro = ROIOutputs(vg_c4_config())
    for k, v in kw.items():
        setattr(ro, k, v)
    return ro


def test_roi_outputs_default_is_class_max():
    ro = _roi_outputs()
    assert ro.selection == "class_max" and ro.select_params() is None
    ro.nms_thresh, ro.score_thresh = [0.5, 1.0, 0.1], 7.0       # the reference's list; score_thresh stays unused there
    assert ro.select_params() is None and ro.params().num_nms_thresh == 3


def test_roi_outputs_per_class_params():
    sp = _roi_outputs(selection="per_class", nms_thresh=[0.3], score_thresh=0.2, min_detections=10, max_detections=100).select_params()
    assert sp.mode == L.VK_SELECT_PER_CLASS and sp.score_thresh == 0.2
    assert (sp.roi.num_nms_thresh, sp.roi.nms_thresh[0], sp.roi.min_detections, sp.roi.max_detections) == (1, 0.3, 10, 100)


@pytest.mark.parametrize("kw,msg", [
    (dict(selection="per-class"), "selection"),
    (dict(selection="per_class", nms_thresh=[0.5, 1.0, 0.1]), "one nms_thresh"),
    (dict(selection="per_class", nms_thresh=[]), "one nms_thresh"),
    (dict(selection="per_class", nms_thresh=[0.3], min_detections=20, max_detections=10), "exceeds max_detections"),
    (dict(selection="per_class", nms_thresh=[0.3], score_thresh=1.5), "score_thresh"),
    (dict(selection="per_class", nms_thresh=[0.3], score_thresh=-0.1), "score_thresh"),
    (dict(selection="per_class", nms_thresh=[0.3], score_thresh=float("nan")), "score_thresh"),
])
def test_roi_outputs_validation(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _roi_outputs(**kw).select_params()


def _select(lib, mode=1, thr=(0.3,), score=0.2, lo=1, hi=4, N=2, R=8, skip=None):
    sp = L.vk_select_params()
    sp.mode, sp.score_thresh = mode, score
    sp.roi.num_nms_thresh = len(thr)
    for i, t in enumerate(thr):
        sp.roi.nms_thresh[i] = t
    sp.roi.min_detections, sp.roi.max_detections = lo, hi
    out = L.vk_outputs(*([FAKE] * 7))
    w = (C.c_float * 4)(10, 10, 5, 5)
    ptr = {k: FAKE for k in ("scores", "deltas", "props", "counts", "feat", "hw", "flag")}
    if skip:
        ptr[skip] = None
    L.call("vk_per_class_select", ptr["scores"], 6, None, 0, ptr["deltas"], 20, 0, ptr["props"], ptr["counts"], ptr["feat"], 64,
           N, R, 5, 0, ptr["hw"], None, w, C.byref(sp), C.byref(out), None, None, ptr["flag"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=0), "VK_SELECT_PER_CLASS"), (dict(thr=(0.3, 0.5)), "one NMS threshold"), (dict(score=1.01), "score_thresh"),
    (dict(score=-1e-9), "score_thresh"), (dict(score=float("nan")), "score_thresh"), (dict(lo=5, hi=4), "exceeds max_detections"),
    (dict(N=0), "N=0"), (dict(R=0), "R=0"), (dict(R=1025), "R=1025"), (dict(hi=9), "max_detections=9"), (dict(skip="scores"), "null"), (dict(skip="flag"), "null"), (dict(skip="counts"), "null"),
])
def test_library_rejects_before_launch(lib, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _select(lib, **kw)


def test_forward_begin_select_rejects_bad_params_before_the_handle(lib):
    sp = L.vk_select_params()
    sp.mode = 7
    out, t = L.vk_outputs(*([FAKE] * 7)), C.c_int64(-1)
    with pytest.raises(ValueError, match="selection mode"):
        L.call("vk_forward_begin_select", None, FAKE, 1, 64, 64, FAKE, None, C.byref(sp), C.byref(out), None, C.byref(t), None)
    sp.mode, sp.score_thresh, sp.roi.num_nms_thresh = L.VK_SELECT_PER_CLASS, 0.2, 3
    with pytest.raises(ValueError, match="one NMS threshold"):
        L.call("vk_forward_begin_select", None, FAKE, 1, 64, 64, FAKE, None, C.byref(sp), C.byref(out), None, C.byref(t), None)


def test_fpn_detector_raises_before_enqueue():
    m = object.__new__(FRCNNFPN)
    m.config, m.training, m._finalized, m._timing, m._stages = fpn_config(), False, True, None, {}
    m.device = torch.device("cpu")
    m.roi_outputs = ROIOutputs(m.config)

    def launched(*a, **k):
        pytest.fail("a device stage was reached")
    m._bottom_up = m.neck = m._box_head = m._predictor = m._prepare = launched
    m.roi_outputs.selection, m.roi_outputs.nms_thresh = "per_class", [0.3]
    with pytest.raises(ValueError, match="FPN"):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
    m.roi_outputs.selection = "nonsense"
    with pytest.raises(ValueError, match="selection"):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
