"""CPU: the numpy restatement of the output-row table (tests/roi_out_rows_util.py) has the properties the
device table and the panel kernel's indexed store rely on: values in {-1} u [0, V), every id exactly once, at its
representative row, -1 on every other row, the non-negative entries ascending with the row."""
import numpy as np
import pytest

from roi_dedupe_util import crafted_boxes, distinct_boxes
from roi_nbr_util import neighbourhood_table
from roi_out_rows_util import NOWHERE, out_rows


def _two_images():
    one = crafted_boxes([(10, 14)])
    two = np.concatenate([one, one])
    two[len(one):, 0] = 1
    return two


# (name, boxes, images, H, W, P)
CASES = [("crafted", lambda: crafted_boxes([(10, 14), (7, 9)]), 2, 10, 14, 14),
         ("crafted_p6", lambda: crafted_boxes([(10, 14), (7, 9)]), 2, 10, 14, 6),
         ("distinct", lambda: distinct_boxes([(14, 28), (14, 28)], 2, P=14), 2, 14, 28, 14),
         ("equal_boxes_on_two_images", _two_images, 2, 10, 14, 14)]


@pytest.mark.parametrize("dil", [2, 1])
@pytest.mark.parametrize("name,make,N,H,W,P", CASES, ids=[c[0] for c in CASES])
def test_properties(name, make, N, H, W, P, dil):
    rois = make()
    _, nid, rep, _ = neighbourhood_table(rois, N, H, W, P, dil)
    rows, V = len(nid), len(rep)
    o = out_rows(nid, rep)
    assert o.shape == (rows,) and o.dtype == np.int32
    assert int(o.min()) >= NOWHERE and int(o.max()) == V - 1                  # values in {-1} u [0, V)
    kept = o[o >= 0]
    assert np.array_equal(np.sort(kept), np.arange(V))                        # each id exactly once
    assert np.array_equal(o[rep], np.arange(V))                               # out_row[rep[v]] == v
    other = np.ones(rows, dtype=bool)
    other[rep] = False
    assert bool((o[other] == NOWHERE).all())                                  # every other row is -1
    assert bool((np.diff(kept) > 0).all())                                    # ascending with the row, since rep is
    if name == "distinct":
        assert V == rows and np.array_equal(o, np.arange(rows))               # no -1 at all
    else:
        assert V < rows and int((o == NOWHERE).sum()) == rows - V
    if name == "equal_boxes_on_two_images":                                   # no id shared across images: the second half repeats the first, shifted
        half = rows // 2
        assert V % 2 == 0
        assert np.array_equal(o[half:], np.where(o[:half] >= 0, o[:half] + V // 2, NOWHERE))
