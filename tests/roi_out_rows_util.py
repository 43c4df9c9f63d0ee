"""Numpy restatement of the output-row table of csrc/roi_windows.hip (vk_roi_out_rows), shared by
tests/test_roi_out_rows_host.py, tests/test_gpu_roi_out_rows.py and tests/test_gpu_panel_out_indexed.py.

out_row[m] says where conv2 of Res5 block 0 stores dense row m among the rows of the distinct neighbourhoods: nid[m] where m is
its neighbourhood's representative (rep[nid[m]] == m), -1 (nowhere) for every other row."""
import numpy as np

NOWHERE = -1


def out_rows(nid, rep):
    """nid [rows] i32, rep [V] i32 (tests/roi_nbr_util.py) -> out_row [rows] i32."""
    nid = np.asarray(nid, dtype=np.int64)
    rep = np.asarray(rep, dtype=np.int64)
    m = np.arange(len(nid), dtype=np.int64)
    return np.where(rep[nid] == m, nid, NOWHERE).astype(np.int32)
