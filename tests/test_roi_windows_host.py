"""CPU: the numpy restatement of the distinct-window path (tests/roi_dedupe_util.py: window table -> pool of the distinct
windows -> expansion by idx) equals oracle.frcnn_oracle.roi_pool bit for bit on crafted boxes.  The GPU tests hold
csrc/roi_windows.hip to this restatement."""
import numpy as np
import pytest
import torch

from oracle import frcnn_oracle
from roi_dedupe_util import SCALE, bin_windows, crafted_boxes, distinct_boxes, pool_windows, window_table

P = 14
MAPS = [(6, 9), (13, 21)]


def feature_maps(N, H, W, C=8, seed=3):
    g = np.random.default_rng(seed)
    return g.standard_normal((N, H, W, C)).astype(np.float32)


@pytest.mark.parametrize("hw", MAPS + [(20, 31)])
def test_table_pool_expand_equals_oracle(hw):
    H, W = hw
    rois = np.concatenate([crafted_boxes([hw, hw]), distinct_boxes([hw, hw], 2)])
    feat = feature_maps(2, H, W)
    idx, win = window_table(rois, 2, H, W, P)
    got = pool_windows(feat, win)[idx].reshape(len(rois), P, P, -1)
    ref = frcnn_oracle.roi_pool(torch.from_numpy(feat).permute(0, 3, 1, 2), torch.from_numpy(rois), P, SCALE)
    assert np.array_equal(got, ref.permute(0, 2, 3, 1).numpy())


def test_crafted_boxes_cover_the_cases():
    """What the crafted set is there for: repeated windows within and across boxes, empty windows, windows of one cell and of
    several, and ids that are the lexicographic rank of the window."""
    hw = MAPS[1]
    H, W = hw
    rois = crafted_boxes([hw])
    bw = bin_windows(rois, 1, H, W, P)
    idx, win = window_table(rois, 1, H, W, P)
    assert len(win) < len(idx) / 3                                   # mostly repeats
    assert np.array_equal(win[idx], bw)                              # the id's window is the row's window
    assert [tuple(r) for r in win.tolist()] == sorted(set(map(tuple, bw.tolist())))
    empty = (win[:, 2] <= win[:, 1]) | (win[:, 4] <= win[:, 3])
    assert empty.any() and not empty.all()
    cells = (win[:, 2] - win[:, 1]) * (win[:, 4] - win[:, 3])
    assert (cells[~empty] == 1).any() and (cells[~empty] > 1).any()
    per_roi = idx.reshape(len(rois), P * P)
    assert np.array_equal(per_roi[0], per_roi[1]) and np.array_equal(per_roi[0], per_roi[2])   # duplicates, and same cells
    assert len(np.unique(per_roi[0])) < P * P                        # repeats inside one box


def test_rounding_ties_follow_roundf():
    """x = 16 n + 8 is n + 0.5 cells: roundf goes away from zero (numpy's rint would go to even)."""
    rois = np.array([[0, 8.0, 24.0, 72.0, 88.0]], dtype=np.float32)   # 0.5, 1.5, 4.5, 5.5 -> 1, 2, 5, 6
    bw = bin_windows(rois, 1, 13, 21, P)
    assert bw[:, 3].min() == 1 and bw[:, 1].min() == 2 and bw[:, 4].max() == 6 and bw[:, 2].max() == 7


def test_distinct_set_has_no_repeated_window():
    hw = (28, 45)
    rois = distinct_boxes([hw], 6)
    assert len(rois) == 6
    idx, win = window_table(rois, 1, hw[0], hw[1], P)
    assert len(win) == len(idx) == 6 * P * P and len(np.unique(idx)) == len(idx)
