"""-m gpu: the device's output-row table (vk_roi_out_rows, csrc/roi_windows.hip) against the numpy restatement
(tests/roi_out_rows_util.py, itself held to its properties by tests/test_roi_out_rows_host.py), integer equality, on the cases
of tests/test_gpu_roi_neighbourhoods.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, P, stream   # noqa: E402
from roi_dedupe_util import SCALE, crafted_boxes, distinct_boxes   # noqa: E402
from roi_nbr_util import neighbourhood_table   # noqa: E402
from roi_out_rows_util import out_rows   # noqa: E402
from vltk_amd import _lib as L   # noqa: E402


def device_out_rows(rois, N, H, W, Pn, dil):
    """(nid, rep, V, out_row) from the device: the window table, the neighbourhood table, then vk_roi_out_rows on their arrays."""
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
    out = torch.full((rows + 8,), -7, dtype=torch.int32, device=DEV)          # eight guard entries behind the table
    L.call("vk_roi_out_rows", P(nid), P(rep), rows, P(out), stream())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert bool((out[rows:] == -7).all())                                      # nothing past the table is written
    return nid.cpu().numpy(), rep.cpu().numpy(), int(v.item()), out[:rows]


def check(rois, N, H, W, Pn, dil):
    _, ref_nid, ref_rep, _ = neighbourhood_table(rois, N, H, W, Pn, dil)
    nid, rep, V, out = device_out_rows(rois, N, H, W, Pn, dil)
    print(f"{len(rois)} RoIs, P {Pn}, dilation {dil}: {len(nid)} rows, {V} neighbourhoods, {int((out < 0).sum())} rows stored nowhere")
    assert V == len(ref_rep) and np.array_equal(nid, ref_nid) and np.array_equal(rep[:V], ref_rep)
    assert np.array_equal(out, out_rows(ref_nid, ref_rep))
    return V


@pytest.mark.parametrize("dil", [2, 1])
@pytest.mark.parametrize("hw", [(10, 14), (7, 9)])
def test_crafted(hw, dil):
    rois = crafted_boxes([hw, hw])
    assert check(rois, 2, hw[0], hw[1], 14, dil) < len(rois) * 196


@pytest.mark.parametrize("dil", [2, 1])
def test_distinct(dil):
    """V = rows: the table is the identity, no -1 at all."""
    rois = distinct_boxes([(14, 28), (14, 28)], 2, P=14)
    assert check(rois, 2, 14, 28, 14, dil) == 4 * 196


@pytest.mark.parametrize("dil", [2, 1])
def test_one_roi(dil):
    check(crafted_boxes([(10, 14)])[2:3], 1, 10, 14, 14, dil)
    assert check(np.float32([[0, 33.0, 34.0, 38.0, 39.0]]), 1, 10, 14, 14, dil) == 9


@pytest.mark.parametrize("dil", [2, 1])
def test_equal_boxes_on_two_images(dil):
    one = crafted_boxes([(10, 14)])
    two = np.concatenate([one, one])
    two[len(one):, 0] = 1
    assert check(two, 2, 10, 14, 14, dil) == 2 * check(one, 2, 10, 14, 14, dil)


def test_many_rows_of_one_neighbourhood_and_several_blocks():
    """400 copies of a box inside one cell (78 400 rows of nine neighbourhoods: nine entries are ids, the rest -1) followed by
    the crafted boxes: more than one workgroup."""
    rois = np.concatenate([np.tile(np.float32([[0, 33.0, 34.0, 38.0, 39.0]]), (400, 1)), crafted_boxes([(10, 14)])])
    check(rois, 1, 10, 14, 14, 2)
