"""The grid-features contract (include/vltk_hip.h vk_forward_grid_begin) restated in numpy: the bins,
the fp64 sum in the contract's order, the cell boxes, and the predictor through the oracle's own functions.  Pure CPU; used
by tests/test_grid_host.py and tests/test_gpu_grid.py."""
import numpy as np
import torch


def extent(size, S, limit):
    """Content extent in map pixels: min(limit, max(1, ceil(size / S))), in integers."""
    return min(int(limit), max(1, (int(size) + S - 1) // S))


def bins(f, G):
    """[(start, end)] of the G cells over f map pixels: floor(i * f / G) .. ceil((i + 1) * f / G), end exclusive."""
    return [((i * f) // G, ((i + 1) * f + G - 1) // G) for i in range(G)]


def cells(hw, Hm, Wm, S, grid):
    """[(ys, ye, xs, xe)] of an image's Gh * Gw cells in row-major order."""
    gh, gw = grid
    fh, fw = extent(hw[0], S, Hm), extent(hw[1], S, Wm)
    return [(ys, ye, xs, xe) for ys, ye in bins(fh, gh) for xs, xe in bins(fw, gw)]


def pool(m, hws, S, grid):
    """m [N, Hm, Wm, C] (any float dtype) -> [N, Gh * Gw, C] float32: per cell and channel the float64 sum taken pixel by pixel,
    y outer and x inner (NOT np.sum, which adds pairwise), divided once by the pixel count and rounded once to float32."""
    m = np.asarray(m)
    N, Hm, Wm, C = m.shape
    out = np.zeros((N, grid[0] * grid[1], C), dtype=np.float32)
    for n in range(N):
        for r, (ys, ye, xs, xe) in enumerate(cells(hws[n], Hm, Wm, S, grid)):
            acc = np.zeros(C, dtype=np.float64)
            for y in range(ys, ye):
                for x in range(xs, xe):
                    acc = acc + m[n, y, x].astype(np.float64)
            out[n, r] = (acc / np.float64((ye - ys) * (xe - xs))).astype(np.float32)
    return out


def boxes(hws, Hm, Wm, S, grid, scales=None):
    """[N, Gh * Gw, 4] float32: (xs * S, ys * S, min(xe * S, w), min(ye * S, h)); with scales_yx one float32 multiply each, x by
    scales[n][1] and y by scales[n][0]."""
    N = len(hws)
    out = np.zeros((N, grid[0] * grid[1], 4), dtype=np.float32)
    for n in range(N):
        h, w = int(hws[n][0]), int(hws[n][1])
        for r, (ys, ye, xs, xe) in enumerate(cells(hws[n], Hm, Wm, S, grid)):
            out[n, r] = (np.float32(xs * S), np.float32(ys * S), min(np.float32(xe * S), np.float32(w)),
                         min(np.float32(ye * S), np.float32(h)))
        if scales is not None:
            sy, sx = np.float32(scales[n][0]), np.float32(scales[n][1])
            out[n, :, 0::2] *= sx
            out[n, :, 1::2] *= sy
    return out


def predict(oracle, feat, C):
    """The box predictor on feature rows [K, F] through the oracle (FRCNNOracle.predictor): soft-max over C + 1 and max /
    arg-max over the first C; the attribute branch on the raw arg-max class, its soft-max without the last column.
    -> dict of obj_ids, obj_probs, attr_ids, attr_probs and the margins (best minus second best) of the class probability,
    the attribute probability and the raw class logit."""
    scores, attr, _ = oracle.predictor(torch.as_tensor(np.asarray(feat, dtype=np.float32)))
    p = torch.softmax(scores.double(), -1)[:, :C]
    ap = torch.softmax(attr[:, :-1].double(), -1)
    top2 = lambda t: (lambda v: (v[:, 0] - v[:, 1]).numpy())(t.topk(2, dim=-1).values)      # noqa: E731
    return {"obj_ids": p.argmax(-1).numpy(), "obj_probs": p.max(-1).values.numpy(), "attr_ids": ap.argmax(-1).numpy(),
            "attr_probs": ap.max(-1).values.numpy(), "cls_margin": top2(p), "attr_margin": top2(ap),
            "logit_margin": top2(scores.double()), "obj_logits": scores.numpy(), "attr_logits": attr.numpy()}
