"""CPU (-m "not gpu"): the tests' restatement of the default class-max selection rule (tests/class_max_util.py, DESIGN.md
section 16) against (a) the reference's own vectors (tests/golden/kat_ops.npz, roiout/* and roiout_scaled/*: what
test_roi_outputs_golden holds the device to) and (b) FRCNNOracle.roi_outputs on the crafted data test_gpu_class_max.py runs on the
device, at R = 300 and R = 1024 in each regime of the threshold loop."""
import os

import numpy as np
import pytest
import torch

from oracle.frcnn_oracle import FRCNNOracle
from vltk_amd.config import Config, vg_c4_config_dict

import class_max_util as CM
from gpu_util import rel_err


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "kat_ops.npz"))


def oracle(thr, mind, maxd):
    d = vg_c4_config_dict()
    d["min_detections"], d["max_detections"] = mind, maxd
    o = FRCNNOracle(Config(d), {})
    o.nms_thresh = list(thr)
    assert tuple(o.cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS) == CM.WEIGHTS
    return o


@pytest.mark.parametrize("tag", ["roiout", "roiout_scaled"])
def test_restatement_reproduces_the_reference_vectors(kat, tag):
    """Classes, attributes and features (the kept rows) exact; probabilities and boxes at test_roi_outputs_golden's 2e-6."""
    thr = kat["roiout/nms_thresh"].tolist()
    prob, cls = CM.host_prob_cls(kat["roiout/obj_logits"])
    ap, ai = torch.from_numpy(kat["roiout/attr_logits"])[:, :-1].softmax(-1).max(-1)
    off = 0
    for i in range(2):
        props = kat[f"roiout/props_{i}"]
        rows = slice(off, off + len(props))
        off += len(props)
        scale = kat["roiout/scales"][i] if tag == "roiout_scaled" else None
        trace = []
        ids, classes, probs, boxes = CM.select_image(prob[rows], cls[rows], kat["roiout/box_deltas"][rows], props, kat["roiout/sizes"][i],
                                                     CM.WEIGHTS, thr, 6, 8, scale, trace=trace)
        n = len(kat[f"{tag}/classes_{i}"])
        assert len(ids) == n, (i, trace)
        np.testing.assert_array_equal(classes.numpy(), kat[f"{tag}/classes_{i}"])
        np.testing.assert_array_equal(ai[rows][ids].numpy(), kat[f"{tag}/attrs_{i}"])
        np.testing.assert_array_equal(kat["roiout/feats_in"][rows][ids.numpy()], kat[f"{tag}/feats_{i}"])
        assert rel_err(probs, kat[f"{tag}/probs_{i}"]) <= 2e-6
        assert rel_err(ap[rows][ids], kat[f"{tag}/attr_probs_{i}"]) <= 2e-6
        assert rel_err(boxes, kat[f"{tag}/boxes_{i}"]) <= 2e-6


@pytest.fixture(scope="module")
def crafted():
    out = {}
    for R in (300, 1024):
        for dups in (True, False):
            d = CM.craft(2, R, CM.SEED.get(R, R), dups=dups)
            d["prob"], d["cls"] = CM.host_prob_cls(d["logits"])
            out[R, dups] = d
    return out


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales_yx"])
@pytest.mark.parametrize("name", CM.REGIMES)
@pytest.mark.parametrize("R", [300, 1024])
def test_restatement_is_the_oracles_roi_outputs(crafted, R, name, scaled):
    """Everything exact, with prob and cls from the same F.softmax; the regime is asserted from the restatement's own trace."""
    d = crafted[R, name != "full"]
    counts = [CM.kept_counts(d, n, d["prob"], d["cls"], (0.05, 0.3, 0.7)) for n in range(2)]
    thr, mind, maxd = CM.regime(name, R, *zip(*counts))
    scales = torch.tensor([[1.25, 1.5], [2.0, 0.75]]) if scaled else None
    ref = oracle(thr, mind, maxd).roi_outputs(d["logits"], d["attr"], d["deltas"], list(d["props"]), d["feats"], d["hw"].tolist(), scales)
    for n, (mb, cls, ms, aid, ap, ft, ids) in enumerate(ref):
        rows = slice(n * R, (n + 1) * R)
        trace = []
        got = CM.select_image(d["prob"][rows], d["cls"][rows], d["deltas"][rows], d["props"][n], d["hw"][n], CM.WEIGHTS, thr, mind, maxd,
                              None if scales is None else scales[n], trace=trace)
        CM.assert_regime(name, trace, len(got[0]), mind, maxd, R)
        print(f"[class-max host] R={R} {name} image {n}: thresholds {thr} bounds [{mind}, {maxd}] kept (uncapped) "
              f"{[k for _, k, _ in trace]} -> {len(got[0])}")
        for a, b in zip(got, (ids, cls, ms, mb)):
            np.testing.assert_array_equal(a.numpy(), b.numpy())
        np.testing.assert_array_equal(d["feats"][rows][got[0]].numpy(), ft.numpy())


def test_table_counts_at_R300(crafted):
    """The crafted data at R = 300 keeps about 17 / 80 / 276 / 300 boxes at 0.05 / 0.3 / 0.7 / 0.9: inside every bound of
    the table for both images, from the oracle's NMS alone."""
    d = crafted[300, True]
    for n in range(2):
        n05, n03, n07, n09 = CM.kept_counts(d, n, d["prob"], d["cls"], (0.05, 0.3, 0.7, 0.9))
        assert 10 <= n05 <= 20 and n05 < 36 <= n03 and 50 <= n03 <= 100 and n07 < 290 and n09 >= 290, (n05, n03, n07, n09)


def test_edge_rows_of_the_crafted_data(crafted):
    """What the edge-case rows are for, from the restatement: the copy of a row is suppressed at every threshold < 1 and the
    lower row kept; equal probabilities come out in row order; the two zero-area boxes (IoU 0/0) both survive; the box on the
    image edge is a line."""
    d = crafted[300, True]
    for n in range(2):
        rows = slice(n * 300, (n + 1) * 300)
        B = CM.chosen_boxes(d["cls"][rows], d["deltas"][rows], d["props"][n], d["hw"][n], CM.WEIGHTS)
        for r in CM.OUTSIDE:
            assert B[r].tolist() == [600.0, 400.0, 600.0, 400.0]
        assert B[CM.LINE, 0] == B[CM.LINE, 2] == 600.0 and B[CM.LINE, 3] > B[CM.LINE, 1]
        assert float(d["prob"][rows][CM.EQUAL[0]]) == float(d["prob"][rows][CM.EQUAL[1]])
        for t in (0.05, 0.97):
            ids = CM.select_image(d["prob"][rows], d["cls"][rows], d["deltas"][rows], d["props"][n], d["hw"][n], CM.WEIGHTS, [t], 300, 300)[0].tolist()
            for src, dst in CM.DUP:
                assert dst not in ids
            assert all(r in ids for r in CM.OUTSIDE)             # 0/0 is not above any threshold, and they touch nothing
        assert all(r in ids for r in CM.EQUAL + tuple(src for src, _ in CM.DUP))
        assert ids.index(CM.EQUAL[1]) == ids.index(CM.EQUAL[0]) + 1


def test_boxes_in_place_of_deltas_and_an_empty_image():
    d = CM.craft(1, 37, 3)
    prob, cls = CM.host_prob_cls(d["logits"])
    a = CM.select_image(prob, cls, d["deltas"], d["props"][0], CM.IMG_HW, CM.WEIGHTS, [0.3], 1, 37)
    B = CM.chosen_boxes(cls, d["deltas"], d["props"][0], CM.IMG_HW, CM.WEIGHTS)
    allc = torch.zeros((37, CM.C, 4))
    allc[torch.arange(37), cls] = B
    for boxes in (B, allc):
        b = CM.select_image(prob, cls, boxes, None, CM.IMG_HW, CM.WEIGHTS, [0.3], 1, 37)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.numpy(), y.numpy())
    e = CM.select_image(prob[:0], cls[:0], d["deltas"][:0], d["props"][0, :0], CM.IMG_HW, CM.WEIGHTS, [0.3, 0.5], 1, 37)
    assert [len(x) for x in e] == [0, 0, 0, 0]
    bad = d["deltas"].clone()
    bad[3, 4 * int(cls[3]) + 1] = float("inf")
    with pytest.raises(AssertionError, match="infinite or NaN"):
        CM.select_image(prob, cls, bad, d["props"][0], CM.IMG_HW, CM.WEIGHTS, [0.3], 1, 37)
    bad = d["deltas"].clone()
    bad[3, 4 * ((int(cls[3]) + 1) % CM.C) + 1] = float("inf")       # an unchosen class's deltas are never decoded
    CM.select_image(prob, cls, bad, d["props"][0], CM.IMG_HW, CM.WEIGHTS, [0.3], 1, 37)
