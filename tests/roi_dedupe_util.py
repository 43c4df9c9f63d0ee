"""Numpy restatement of csrc/roi_windows.hip (window table, pool of the distinct windows, expansion) and the crafted boxes
shared by tests/test_roi_windows_host.py and tests/test_gpu_roi_dedupe.py.  The window rule is oracle/tv_ops.c's
(vko_roi_pool), in float32 where the C code is float32."""
import numpy as np

SCALE = 1.0 / 16.0


def _roundf(v32):
    """C roundf (half away from zero) of float32 values, computed exactly in float64."""
    v = v32.astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def bin_windows(rois, N, H, W, P, scale=SCALE):
    """rois [K,5] f32 -> int64 [K*P*P, 5] rows (image, y0, y1, x0, x1), row (k*P + ph)*P + pw."""
    r = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    K = r.shape[0]
    s = np.float32(scale)
    b = np.clip(r[:, 0].astype(np.int64), 0, N - 1)
    rsw, rsh, rew, reh = (_roundf(r[:, i] * s) for i in (1, 2, 3, 4))
    roi_w = np.maximum(rew - rsw + 1, 1)
    roi_h = np.maximum(reh - rsh + 1, 1)
    bin_h = roi_h.astype(np.float32) / np.float32(P)
    bin_w = roi_w.astype(np.float32) / np.float32(P)
    p0 = np.arange(P, dtype=np.float32)[None, :]
    p1 = np.arange(1, P + 1, dtype=np.float32)[None, :]
    hs = np.floor(p0 * bin_h[:, None]).astype(np.int64) + rsh[:, None]        # float32 products, as in C
    he = np.ceil(p1 * bin_h[:, None]).astype(np.int64) + rsh[:, None]
    ws = np.floor(p0 * bin_w[:, None]).astype(np.int64) + rsw[:, None]
    we = np.ceil(p1 * bin_w[:, None]).astype(np.int64) + rsw[:, None]
    hs, he = np.clip(hs, 0, H), np.clip(he, 0, H)
    ws, we = np.clip(ws, 0, W), np.clip(we, 0, W)
    out = np.empty((K, P, P, 5), dtype=np.int64)
    out[..., 0] = b[:, None, None]
    out[..., 1] = hs[:, :, None]
    out[..., 2] = he[:, :, None]
    out[..., 3] = ws[:, None, :]
    out[..., 4] = we[:, None, :]
    return out.reshape(K * P * P, 5)


def window_table(rois, N, H, W, P, scale=SCALE):
    """(idx [K*P*P] i32, win [U,5] i32): ids are the ranks of (image, y0, y1, x0, x1) in lexicographic order."""
    bw = bin_windows(rois, N, H, W, P, scale)
    key = (((bw[:, 0] * (H + 1) + bw[:, 1]) * (H + 1) + bw[:, 2]) * (W + 1) + bw[:, 3]) * (W + 1) + bw[:, 4]
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return inv.astype(np.int32).reshape(-1), bw[first].astype(np.int32)


def pool_windows(feat_nhwc, win):
    """feat [N,H,W,C], win [U,5] -> [U,C]: maximum over the window, zeros for an empty one."""
    out = np.zeros((win.shape[0], feat_nhwc.shape[-1]), dtype=feat_nhwc.dtype)
    for i, (b, y0, y1, x0, x1) in enumerate(win.tolist()):
        if y1 > y0 and x1 > x0:
            out[i] = feat_nhwc[b, y0:y1, x0:x1].reshape(-1, feat_nhwc.shape[-1]).max(axis=0)
    return out


def crafted_boxes(hw):
    """[(image, x0, y0, x1, y1)] in pixels for maps hw = [(H, W), ...] (stride 16): duplicates, boxes under one cell, boxes over
    224 px, boxes partly or wholly outside the map (empty windows), coordinates on .5 rounding ties (x / 16 = n + 0.5 at
    x = 16 n + 8)."""
    rows = []
    for n, (H, W) in enumerate(hw):
        ph, pw = 16.0 * H, 16.0 * W
        rows += [
            (n, 10.0, 12.0, 90.0, 70.0), (n, 10.0, 12.0, 90.0, 70.0),              # duplicates
            (n, 10.5, 12.25, 90.0, 70.0),                                          # same cells, other pixels
            (n, 33.0, 34.0, 38.0, 40.0), (n, 3.0, 2.0, 4.0, 3.0),                  # under one cell
            (n, 0.0, 0.0, pw - 1.0, ph - 1.0), (n, 0.0, 0.0, min(pw - 1.0, 250.0), 95.0),   # over 224 px where the map allows
            (n, -40.0, -30.0, 50.0, 40.0), (n, pw - 30.0, ph - 20.0, pw + 60.0, ph + 50.0),   # partly outside
            (n, pw + 40.0, 10.0, pw + 90.0, 60.0), (n, 10.0, ph + 33.0, 60.0, ph + 80.0),     # wholly outside
            (n, -100.0, -90.0, -20.0, -18.0),
            (n, 8.0, 24.0, 72.0, 88.0), (n, 24.0, 8.0, 56.0, 40.0), (n, 7.99, 8.01, 40.0, 56.0),   # .5 ties (and just off them)
            (n, 40.0, 40.0, 20.0, 20.0),                                           # malformed: forced to 1 x 1
        ]
    return np.asarray(rows, dtype=np.float32)


def distinct_boxes(hw, per_image, P=14):
    """Boxes of P x P cells on disjoint cell ranges: each of a box's P * P bins is a window of one cell of its own, and no two
    boxes share a cell, so every window is distinct (U equals the bin count).  A map smaller than P cells holds none."""
    rows = []
    for n, (H, W) in enumerate(hw):
        for j in range(min(per_image, (W // P) * (H // P))):
            cx, cy = j % (W // P), j // (W // P)
            x0, y0 = P * 16.0 * cx, P * 16.0 * cy
            rows.append((n, x0, y0, x0 + (P - 1) * 16.0, y0 + (P - 1) * 16.0))
    return np.asarray(rows, dtype=np.float32).reshape(-1, 5)
