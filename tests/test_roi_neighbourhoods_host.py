"""CPU: the numpy restatement of the neighbourhood table (tests/roi_nbr_util.py) has the properties the device
table is then held to: ids onto [0, V), equal ids exactly where the nine (image, y0, y1, x0, x1) keys are equal, rep the
smallest such row, duplicates of a box sharing their ids."""
import numpy as np
import pytest

from roi_dedupe_util import crafted_boxes, distinct_boxes, window_table
from roi_nbr_util import neighbourhood_table, nine_ids, nine_keys, rank_by_first_row

CASES = [("crafted", [(10, 14), (7, 9)], 14), ("crafted", [(10, 14), (7, 9)], 6), ("distinct", [(14, 28), (14, 28)], 14),
         ("distinct", [(6, 12), (12, 6)], 6)]


def boxes(kind, hw, P):
    return crafted_boxes(hw) if kind == "crafted" else distinct_boxes(hw, 2, P=P)


@pytest.mark.parametrize("dil", [2, 1])
@pytest.mark.parametrize("kind,hw,P", CASES)
def test_properties(kind, hw, P, dil):
    rois = boxes(kind, hw, P)
    N, H, W = len(hw), max(h for h, _ in hw), max(w for _, w in hw)
    idx, nid, rep, idx_rep = neighbourhood_table(rois, N, H, W, P, dil)
    rows = len(rois) * P * P
    V = len(rep)
    assert nid.shape == (rows,) and V >= 1
    assert np.array_equal(np.unique(nid), np.arange(V))                       # onto [0, V)
    keys = nine_keys(rois, N, H, W, P, dil).reshape(rows, 45)
    # equal nid <=> equal nine keys: every row carries the keys of its id's representative, and representatives differ
    assert np.array_equal(keys, keys[rep][nid])
    assert len(np.unique(keys[rep], axis=0)) == V
    # rep is the smallest row of its id, ascending
    first = np.full(V, rows, dtype=np.int64)
    np.minimum.at(first, nid, np.arange(rows))
    assert np.array_equal(first, rep) and bool((np.diff(rep) > 0).all())
    assert np.array_equal(idx_rep, idx[rep])
    # the window ids say the same as the full keys (ids are ranks of the full key)
    nid2, rep2 = rank_by_first_row(nine_ids(idx, len(rois), P, dil))
    assert np.array_equal(nid2, nid) and np.array_equal(rep2, rep)
    if kind == "distinct":
        assert V == rows
    else:
        assert V < rows
        per = P * P                                                           # boxes 0 and 1 of each image are duplicates
        for n in range(len(hw)):
            b0 = n * 16 * per
            assert np.array_equal(nid[b0:b0 + per], nid[b0 + per:b0 + 2 * per])


def test_no_sharing_across_images():
    """The same boxes on two images of the same map: no id is shared, V doubles."""
    one = crafted_boxes([(10, 14)])
    two = np.concatenate([one, one])
    two[len(one):, 0] = 1
    _, nid1, rep1, _ = neighbourhood_table(one, 2, 10, 14, 14, 2)
    _, nid2, rep2, _ = neighbourhood_table(two, 2, 10, 14, 14, 2)
    assert len(rep2) == 2 * len(rep1)
    half = len(nid1)
    assert np.array_equal(nid2[:half], nid1) and np.array_equal(nid2[half:], nid1 + len(rep1))


def test_window_ids_alone_do_not_decide():
    """A bin's own window is one of nine: rows with equal windows can differ in their neighbourhood (V > U on the crafted boxes)."""
    rois = crafted_boxes([(10, 14)])
    idx, _ = window_table(rois, 1, 10, 14, 14)
    _, _, rep, _ = neighbourhood_table(rois, 1, 10, 14, 14, 2)
    assert len(rep) > int(idx.max()) + 1
