"""-m gpu: the device's neighbourhood table (vk_roi_neighbourhoods, csrc/roi_windows.hip) against the numpy
restatement (tests/roi_nbr_util.py, itself held to its properties by tests/test_roi_neighbourhoods_host.py): nid, rep,
idx_rep and V, integer equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, P, stream   # noqa: E402
from roi_dedupe_util import SCALE, crafted_boxes, distinct_boxes   # noqa: E402
from roi_nbr_util import neighbourhood_table   # noqa: E402
from vltk_amd import _lib as L   # noqa: E402


def device_tables(rois, N, H, W, Pn, dil):
    K = len(rois)
    rows = K * Pn * Pn
    lib = L.load()
    wsb = lib.vk_roi_windows_workspace_bytes(N, H, W)
    nbb = lib.vk_roi_neighbourhoods_workspace_bytes(rows)
    assert wsb > 0 and nbb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    nws = torch.empty(nbb, dtype=torch.uint8, device=DEV)
    r = torch.from_numpy(np.ascontiguousarray(rois)).to(DEV)
    idx = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    win = torch.full((rows, 5), -1, dtype=torch.int32, device=DEV)
    u = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.call("vk_roi_windows", P(r), K, N, H, W, Pn, SCALE, P(idx), P(win), P(u), P(ws), wsb, stream())
    nid, rep, idx_rep = (torch.full((rows,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    v = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.call("vk_roi_neighbourhoods", P(idx), K, Pn, dil, P(nid), P(rep), P(idx_rep), P(v), P(nws), nbb, stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), nid.cpu().numpy(), rep.cpu().numpy(), idx_rep.cpu().numpy(), int(v.item())


def check(rois, N, H, W, Pn, dil):
    ref_idx, ref_nid, ref_rep, ref_idx_rep = neighbourhood_table(rois, N, H, W, Pn, dil)
    idx, nid, rep, idx_rep, V = device_tables(rois, N, H, W, Pn, dil)
    print(f"{len(rois)} RoIs, P {Pn}, dilation {dil}: {len(idx)} bins, {int(idx.max()) + 1} windows, {V} neighbourhoods")
    assert np.array_equal(idx, ref_idx)
    assert V == len(ref_rep)
    assert np.array_equal(nid, ref_nid)
    assert np.array_equal(rep[:V], ref_rep) and np.array_equal(idx_rep[:V], ref_idx_rep)
    assert bool((rep[V:] == -7).all()) and bool((idx_rep[V:] == -7).all())       # nothing past the list is written
    return V


@pytest.mark.parametrize("dil", [2, 1])
@pytest.mark.parametrize("hw", [(10, 14), (7, 9)])
def test_crafted(hw, dil):
    """Duplicates, sub-cell boxes, boxes over 14 cells, boxes partly and wholly outside, .5 ties; two images of the one map."""
    rois = crafted_boxes([hw, hw])
    V = check(rois, 2, hw[0], hw[1], 14, dil)
    assert V < len(rois) * 196


@pytest.mark.parametrize("dil", [2, 1])
def test_distinct(dil):
    rois = distinct_boxes([(14, 28), (14, 28)], 2, P=14)
    assert len(rois) == 4
    assert check(rois, 2, 14, 28, 14, dil) == 4 * 196


@pytest.mark.parametrize("dil", [2, 1])
def test_one_roi(dil):
    check(crafted_boxes([(10, 14)])[2:3], 1, 10, 14, 14, dil)
    # a box inside one cell: one window, and nine neighbourhoods told apart by which of their positions lie off the map
    assert check(np.float32([[0, 33.0, 34.0, 38.0, 39.0]]), 1, 10, 14, 14, dil) == 9


@pytest.mark.parametrize("dil", [2, 1])
def test_equal_boxes_on_two_images_share_nothing(dil):
    one = crafted_boxes([(10, 14)])
    two = np.concatenate([one, one])
    two[len(one):, 0] = 1
    V1 = check(one, 2, 10, 14, 14, dil)
    assert check(two, 2, 10, 14, 14, dil) == 2 * V1


def test_many_rows_of_one_neighbourhood_and_several_blocks():
    """400 copies of a box inside one cell (78 400 rows, nine neighbourhoods: every insert meets the same few slots) followed by the
    crafted boxes: more than one 256-bit block of the row bitmap, more than one workgroup."""
    rois = np.concatenate([np.tile(np.float32([[0, 33.0, 34.0, 38.0, 39.0]]), (400, 1)), crafted_boxes([(10, 14)])])
    check(rois, 1, 10, 14, 14, 2)
