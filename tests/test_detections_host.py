"""CPU (-m "not gpu"): the host side of roi_outputs.selection = "detections"  -- the tests' restatement
of the contract (tests/detections_util.py) against the vectors the reference's own methods generated
(tests/golden/e2e_per_class.npz), the new C-ABI symbols, ROIOutputs' validation, the checks the library makes before any
HIP call, and the FPN detector's refusal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import fpn_config, vg_c4_config
from vltk_amd.frcnn import SELECTIONS, ROIOutputs
from vltk_amd.frcnn_fpn import FRCNNFPN

import detections_util as DT

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


def fixture_relation(g, i, t, res, classes_of, tol=1e-3):
    """What the per-class fixture pins of a detections output `res` of image i at threshold t with max_detections = 1024: the
    rows that occur are exactly {r : max_conf_r > t}; the first occurrence of a row carries cls_r, and its score and box are
    max_conf_r and the stored box (kept rows of the fixture only) within tol.  classes_of maps res["classes"] to class ids."""
    conf, cls = g[f"max_conf_{i}"], g[f"cls_{i}"]
    ids = np.asarray(res["ids"])
    assert len(ids) < 1024, "the cut at max_detections must not bind"
    want = set(np.nonzero(conf.astype(np.float64) > t)[0].tolist())
    assert set(ids.tolist()) == want, (i, t)
    stored = {int(r): k for k, r in enumerate(g[f"keep_ids_{i}"])}
    seen = set()
    for k, r in enumerate(ids.tolist()):
        if r in seen:
            continue
        seen.add(r)
        assert int(classes_of(np.asarray(res["classes"]))[k]) == int(cls[r]), (i, t, r)
        assert abs(float(res["probs"][k]) - float(conf[r])) <= tol * float(conf.max()), (i, t, r)
        if r in stored:
            box = g[f"boxes_{i}"][stored[r]]
            assert np.abs(np.asarray(res["boxes"][k]) - box).max() <= tol * np.abs(box).max(), (i, t, r)
    return len(want), len(ids)


def test_restatement_against_the_fixture(golden):
    """NMS per class runs class by class, so the rule over the stored class columns (every box's confidence class and its three
    best classes) decides every row's best surviving class as the full rule does."""
    g = golden
    w = vg_c4_config().ROI_BOX_HEAD.BBOX_REG_WEIGHTS
    assert min(float(g[f"thresh_margin_{i}"].min()) for i in range(2)) >= 5.3e-3        # well posed at the thresholds
    multi = 0
    for t in g["score_thresh"].tolist():
        for i in range(2):
            cols = g[f"class_cols_{i}"]
            sc = np.concatenate([g[f"scores_cols_{i}"], np.zeros((len(g[f"scores_cols_{i}"]), 1), np.float32)], 1)
            res = DT.select_image(sc, g[f"deltas_cols_{i}"], g[f"proposal_boxes_{i}"], g["shapes"][i], w, float(g["nms_thresh"]), t, 1024)
            rows, outs = fixture_relation(g, i, t, res, lambda c: cols[c])
            assert res["n_survivors"] == outs
            multi += outs - rows
            p = res["probs"].numpy()
            assert (p[:-1] >= p[1:]).all() and (p.astype(np.float64) > t).all()
    assert multi > 0, "no proposal of the fixture comes out under two classes"


def test_restatement_rules():
    """Strict threshold; ties by row, then class; a proposal under several classes; nothing above the threshold -> nothing;
    the cut at max_detections falls in the ranking."""
    props = np.asarray([[10, 10, 50, 50], [10, 10, 50, 50], [100, 100, 140, 150]], np.float32)
    scores = np.asarray([[0.4, 0.4, 0.2], [0.4, 0.4, 0.2], [0.4, 0.3, 0.3]], np.float32)
    deltas = np.zeros((3, 8), np.float32)
    args = (scores, deltas, props, (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3)
    r = DT.select_image(*args, 0.0, 100)                       # row 1 duplicates row 0: suppressed in both classes
    assert list(zip(r["ids"].tolist(), r["classes"].tolist())) == [(0, 0), (0, 1), (2, 0), (2, 1)] and r["n_survivors"] == 4
    r = DT.select_image(*args, float(np.float32(0.3)), 100)    # strict: row 2's 0.3 in class 1 is not above 0.3
    assert list(zip(r["ids"].tolist(), r["classes"].tolist())) == [(0, 0), (0, 1), (2, 0)]
    r = DT.select_image(*args, 0.0, 3)
    assert list(zip(r["ids"].tolist(), r["classes"].tolist())) == [(0, 0), (0, 1), (2, 0)] and r["n_survivors"] == 4
    r = DT.select_image(*args, float(np.float32(0.4)), 100)    # nothing is above the best score itself
    assert len(r["ids"]) == 0 and r["boxes"].shape == (0, 4) and r["n_survivors"] == 0
    r = DT.select_image(scores[:0], deltas[:0], props[:0], (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3, 0.0, 5)
    assert len(r["ids"]) == 0
    nan = scores.copy()
    nan[2, 0] = np.nan
    r = DT.select_image(nan, deltas, props, (200, 200), (10.0, 10.0, 5.0, 5.0), 0.3, 0.0, 100)
    assert (2, 0) not in list(zip(r["ids"].tolist(), r["classes"].tolist()))


def test_new_symbols_are_exported(lib):
    for name in ("vk_detections_select", "vk_detections_lds_keys"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert (L.VK_SELECT_CLASS_MAX, L.VK_SELECT_PER_CLASS, L.VK_SELECT_DETECTIONS) == (0, 1, 2)
    assert SELECTIONS == ("class_max", "per_class", "detections")
    cap = lib.vk_detections_lds_keys()
    assert cap >= 1024 and cap & (cap - 1) == 0
    with open(os.path.join(os.path.dirname(L.LIB_PATH), "..", "include", "vltk_hip.h")) as f:
        text = f.read()
    assert f"#define VK_DETECTIONS_LDS_KEYS {cap}\n" in text and "#define VK_SELECT_DETECTIONS 2\n" in text
    # the pinned structs and the version stay as they were
    assert C.sizeof(L.vk_select_params) == 8 + 8 + C.sizeof(L.vk_roi_params)
    assert C.sizeof(L.vk_roi_params) == 8 + 8 * 8 + 8 and lib.vk_version() == 1


def _roi_outputs(**kw):
    ro = ROIOutputs(vg_c4_config())
    for k, v in kw.items():
        setattr(ro, k, v)
    return ro


def test_roi_outputs_detections_params():
    sp = _roi_outputs(selection="detections", nms_thresh=[0.3], score_thresh=0.05, min_detections=0, max_detections=100).select_params()
    assert sp.mode == L.VK_SELECT_DETECTIONS and sp.score_thresh == 0.05
    assert (sp.roi.num_nms_thresh, sp.roi.nms_thresh[0], sp.roi.min_detections, sp.roi.max_detections) == (1, 0.3, 0, 100)
    # max_detections may exceed POST_NMS_TOPK_TEST, up to 1024
    assert _roi_outputs(selection="detections", nms_thresh=[0.3], min_detections=0, max_detections=1024).select_params().roi.max_detections == 1024
    # the two other modes are as they were
    assert _roi_outputs().select_params() is None
    assert _roi_outputs(selection="per_class", nms_thresh=[0.3]).select_params().mode == L.VK_SELECT_PER_CLASS


OK = dict(selection="detections", nms_thresh=[0.3], score_thresh=0.05, min_detections=0, max_detections=100)


@pytest.mark.parametrize("kw,msg", [
    (dict(selection="detection"), "selection"),
    (dict(nms_thresh=[0.5, 1.0, 0.1]), "one nms_thresh"),
    (dict(nms_thresh=[]), "one nms_thresh"),
    (dict(score_thresh=1.5), "score_thresh"),
    (dict(score_thresh=-0.1), "score_thresh"),
    (dict(score_thresh=float("nan")), "score_thresh"),
    (dict(min_detections=10), "min_detections=10 must be 0"),
    (dict(min_detections=1), "no minimum count"),
    (dict(max_detections=0), "max_detections=0"),
    (dict(max_detections=1025), "max_detections=1025"),
])
def test_roi_outputs_validation(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _roi_outputs(**{**OK, **kw}).select_params()


def test_config_default_min_detections_is_rejected_with_the_reason():
    ro = _roi_outputs(selection="detections", nms_thresh=[0.3])      # min_detections is still the config's MIN_DETECTIONS
    lo = int(vg_c4_config().MIN_DETECTIONS)
    assert ro.min_detections == lo > 0
    with pytest.raises(ValueError, match=f"no minimum count to fill: min_detections={lo} must be 0.*MIN_DETECTIONS"):
        ro.select_params()


def _select(lib, mode=2, thr=(0.3,), score=0.05, lo=0, hi=4, N=2, R=8, Cn=5, skip=None):
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
    L.call("vk_detections_select", ptr["scores"], 1 << 21, None, 0, ptr["deltas"], 1 << 23, 0, ptr["props"], ptr["counts"], ptr["feat"], 64,
           N, R, Cn, 0, ptr["hw"], None, w, C.byref(sp), C.byref(out), None, None, ptr["flag"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=1), "VK_SELECT_DETECTIONS"), (dict(mode=0), "VK_SELECT_DETECTIONS"), (dict(mode=7), "VK_SELECT_DETECTIONS"),
    (dict(thr=(0.3, 0.5)), "one NMS threshold"), (dict(thr=()), "one NMS threshold"),
    (dict(score=1.01), "score_thresh"), (dict(score=-1e-9), "score_thresh"), (dict(score=float("nan")), "score_thresh"),
    (dict(lo=10), "min_detections=10 must be 0"), (dict(lo=1), "no minimum count"), (dict(lo=-1), "min_detections=-1"),
    (dict(hi=0), "max_detections=0"), (dict(hi=1025), "max_detections=1025"),
    (dict(N=0), "N=0"), (dict(N=65536), "N=65536"), (dict(R=0), "R=0"), (dict(R=1025), "R=1025"),
    (dict(Cn=0), "C=0"), (dict(Cn=1 << 20), f"C={1 << 20}"),
    (dict(skip="scores"), "null"), (dict(skip="flag"), "null"), (dict(skip="counts"), "null"),
])
def test_library_rejects_before_launch(lib, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _select(lib, **kw)


def test_per_class_select_still_rejects_the_other_modes(lib):
    sp = L.vk_select_params()
    sp.score_thresh, sp.roi.num_nms_thresh, sp.roi.min_detections, sp.roi.max_detections = 0.2, 1, 0, 4
    sp.roi.nms_thresh[0] = 0.3
    out, w = L.vk_outputs(*([FAKE] * 7)), (C.c_float * 4)(10, 10, 5, 5)
    for mode in (L.VK_SELECT_DETECTIONS, L.VK_SELECT_CLASS_MAX):
        sp.mode = mode
        with pytest.raises(ValueError, match="VK_SELECT_PER_CLASS"):
            L.call("vk_per_class_select", FAKE, 6, None, 0, FAKE, 20, 0, FAKE, FAKE, FAKE, 64, 2, 8, 5, 0, FAKE, None, w, C.byref(sp),
                   C.byref(out), None, None, FAKE, None)


def test_forward_begin_select_rejects_bad_params_before_the_handle(lib):
    sp = L.vk_select_params()
    out, t = L.vk_outputs(*([FAKE] * 7)), C.c_int64(-1)

    def begin():
        L.call("vk_forward_begin_select", None, FAKE, 1, 64, 64, FAKE, None, C.byref(sp), C.byref(out), None, C.byref(t), None)
    sp.mode = 7
    with pytest.raises(ValueError, match="selection mode 7"):
        begin()
    sp.mode, sp.score_thresh, sp.roi.num_nms_thresh, sp.roi.min_detections, sp.roi.max_detections = L.VK_SELECT_DETECTIONS, 0.05, 3, 0, 100
    with pytest.raises(ValueError, match="one NMS threshold"):
        begin()
    sp.roi.num_nms_thresh, sp.score_thresh = 1, 1.5
    with pytest.raises(ValueError, match="score_thresh"):
        begin()
    sp.score_thresh, sp.roi.min_detections = 0.05, 10
    with pytest.raises(ValueError, match="min_detections=10 must be 0"):
        begin()
    sp.roi.min_detections, sp.roi.max_detections = 0, 1025
    with pytest.raises(ValueError, match="max_detections=1025"):
        begin()
    sp.roi.max_detections = 0
    with pytest.raises(ValueError, match="max_detections=0"):
        begin()
    sp.roi.max_detections = 100                                 # valid parameters: the next check is the handle's
    with pytest.raises(ValueError, match="null argument"):
        begin()


def test_fpn_detector_raises_before_enqueue():
    m = object.__new__(FRCNNFPN)
    m.config, m.training, m._finalized, m._timing, m._stages = fpn_config(), False, True, None, {}
    m.device = torch.device("cpu")
    m.roi_outputs = ROIOutputs(m.config)

    def launched(*a, **k):
        pytest.fail("a device stage was reached")
    m._bottom_up = m.neck = m._box_head = m._predictor = m._prepare = launched
    m.roi_outputs.selection, m.roi_outputs.nms_thresh = "detections", [0.3]          # min_detections still the default: FPN first
    with pytest.raises(ValueError, match='selection="detections".*FPN'):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
    m.roi_outputs.min_detections = 0
    with pytest.raises(ValueError, match='selection="detections".*FPN'):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
    m.roi_outputs.selection = "per_class"
    with pytest.raises(ValueError, match='selection="per_class".*FPN'):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
    m.roi_outputs.selection = "nonsense"
    with pytest.raises(ValueError, match="selection"):
        m(torch.zeros(1, 3, 64, 64), torch.tensor([[64, 64]]))
