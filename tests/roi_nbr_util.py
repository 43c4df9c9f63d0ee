"""Numpy restatement of the neighbourhood table of csrc/roi_windows.hip (vk_roi_neighbourhoods), built on
roi_dedupe_util.bin_windows, shared by tests/test_roi_neighbourhoods_host.py and tests/test_gpu_roi_neighbourhoods.py.

The neighbourhood of bin (k, i, j) is the nine windows at (i + {-d, 0, d}, j + {-d, 0, d}) of RoI k, a position outside the
P x P map being a value of its own.  Ids number the distinct neighbourhoods in the order of their smallest rows."""
import numpy as np

from roi_dedupe_util import SCALE, bin_windows, window_table

OUTSIDE = -1


def nine_keys(rois, N, H, W, P, dil, scale=SCALE):
    """int64 [K*P*P, 9, 5]: the (image, y0, y1, x0, x1) of the nine windows of each row, OUTSIDE in all five for a position off
    the map.  Straight from bin_windows: no window id in between."""
    bw = bin_windows(rois, N, H, W, P, scale).reshape(-1, P, P, 5)
    K = bw.shape[0]
    pad = np.full((K, P + 2 * dil, P + 2 * dil, 5), OUTSIDE, dtype=np.int64)
    pad[:, dil:dil + P, dil:dil + P] = bw
    taps = [pad[:, dil + a * dil:dil + a * dil + P, dil + b * dil:dil + b * dil + P] for a in (-1, 0, 1) for b in (-1, 0, 1)]
    return np.stack(taps, axis=3).reshape(K * P * P, 9, 5)


def nine_ids(idx, K, P, dil):
    """int64 [K*P*P, 9]: the window ids of the nine positions, OUTSIDE off the map (what the device compares)."""
    g = np.asarray(idx, dtype=np.int64).reshape(K, P, P)
    pad = np.full((K, P + 2 * dil, P + 2 * dil), OUTSIDE, dtype=np.int64)
    pad[:, dil:dil + P, dil:dil + P] = g
    taps = [pad[:, dil + a * dil:dil + a * dil + P, dil + b * dil:dil + b * dil + P] for a in (-1, 0, 1) for b in (-1, 0, 1)]
    return np.stack(taps, axis=3).reshape(K * P * P, 9)


def rank_by_first_row(keys2d):
    """keys2d [rows, n] -> (nid [rows] i32, rep [V] i32): equal rows share an id, ids in the order of their smallest rows."""
    _, first, inv = np.unique(keys2d, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    return rank[np.asarray(inv).reshape(-1)].astype(np.int32), first[order].astype(np.int32)


def neighbourhood_table(rois, N, H, W, P, dil, scale=SCALE):
    """(idx [K*P*P] i32, nid [K*P*P] i32, rep [V] i32, idx_rep [V] i32) from the boxes: the window table, then the neighbourhoods
    over the full five-number keys."""
    idx, _ = window_table(rois, N, H, W, P, scale)
    nid, rep = rank_by_first_row(nine_keys(rois, N, H, W, P, dil, scale).reshape(len(idx), 45))
    return idx, nid, rep, idx[rep]
