"""Shared by the RoIAlign-pooler tests of the C4 model (test_roi_align_c4_host.py, test_gpu_roi_align_c4.py).

AlignOracle: the C4 oracle with RoIAlign in place of RoIPool.  The rule is torchvision's / detectron2's; the reference holds
only RoIPool (frcnn.py:1179), so this is PARITY UNPINNED, exactly as RoIAlign on the FPN side is, and
oracle/fpn_oracle.py::roi_align is the yardstick.

The exact set: maps and boxes on which RoIAlign is exact in fp32 whatever the order of the sums -- P = 14, scale 1/16,
aligned, integer map values in [-8, 8], box sides of 56 .. 896 px (bins of 1/4 .. 4 cells), origins on multiples of 4 px,
sampling ratio 0 or 2.  Every sample then sits on a multiple of 1/16 cell, every bilinear weight is a multiple of 1/256, every
count is a power of two (1 .. 16): all partial sums are short dyadic numbers, so a kernel that sums in another order than
the oracle (the separable form of csrc/fpn.hip) still has to give the oracle's bits.  roi_align_fp64 is the independent restatement that proves it on the CPU."""
import ctypes as C

import numpy as np
import torch

from oracle import fpn_oracle as fo
from oracle.frcnn_oracle import FRCNNOracle, _h

POOLER_ALIGNED = {"ROIAlign": False, "ROIAlignV2": True}
EXACT_P, EXACT_SCALE = 14, 1.0 / 16
EXACT_SIDES = (56, 112, 224, 448, 896)
EXACT_MAP = (2, 40, 44)                   # N, H, W cells: 640 x 704 px


class AlignOracle(FRCNNOracle):
    """FRCNNOracle whose pooler is RoIAlign as ROI_BOX_HEAD.POOLER_TYPE / POOLER_SAMPLING_RATIO say."""

    def pool(self, feat, proposal_boxes):
        rois = torch.cat([torch.cat((torch.full((len(b), 1), float(i)), b), dim=1)
                          for i, b in enumerate(proposal_boxes)], dim=0)      # as the parent: frcnn.py:426-441
        head = self.cfg.ROI_BOX_HEAD
        out = fo.roi_align(feat, rois, head.POOLER_RESOLUTION, 1.0 / 16, int(getattr(head, "POOLER_SAMPLING_RATIO", 0)),
                           POOLER_ALIGNED[head.POOLER_TYPE])
        return _h(out) if self.emulate else out       # the device stores the pooled tensor in f16: one rounding


def exact_map(C_, seed=0):
    """[N, C, H, W] f32 of integers in [-8, 8]."""
    N, H, W = EXACT_MAP
    gen = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(gen.integers(-8, 9, (N, C_, H, W)).astype(np.float32))


def exact_rois(seed=0):
    """[K, 5] f32 (batch, x1, y1, x2, y2): every (width, height) pair of EXACT_SIDES, origins on multiples of 4 px from
    before the map to near its far edge, so that boxes start outside, run past the map and lie inside it; both images."""
    N, H, W = EXACT_MAP
    gen = np.random.Generator(np.random.PCG64(100 + seed))
    rows = []
    for w in EXACT_SIDES:
        for h in EXACT_SIDES:
            for _ in range(2):
                x0 = 4 * int(gen.integers(-16, (W * 16 - 8) // 4))
                y0 = 4 * int(gen.integers(-16, (H * 16 - 8) // 4))
                rows.append([int(gen.integers(0, N)), x0, y0, x0 + w, y0 + h])
    rows += [[0, -64, -64, -64 + 56, -64 + 56],             # wholly outside (every sample skipped)
             [1, W * 16 - 28, H * 16 - 28, W * 16 + 28, H * 16 + 28],   # straddles the far corner: the clamp at H - 1, W - 1
             [1, -8, -8, 216, 216],                         # the clamp at 0
             [0, 0, 0, 224, 224]]
    return np.asarray(rows, dtype=np.float32)


def roi_geometry(r, P, scale, sampling_ratio, aligned, ft=np.float64):
    """(sh, sw, bh, bw, gh, gw) of one RoI row (batch, x1, y1, x2, y2) in the float type `ft`, by the expressions of
    csrc/fpn.hip and oracle/tv_ops.c, one rounding per operation."""
    r = np.asarray(r, dtype=ft)
    s, off, Pf = ft(scale), ft(0.5 if aligned else 0.0), ft(P)
    sw, sh, ew, eh = (r[1:] * s - off)
    rw, rh = ew - sw, eh - sh
    if not aligned:
        rw, rh = max(rw, ft(1.0)), max(rh, ft(1.0))       # fmaxf: a NaN side becomes 1
    bh, bw = rh / Pf, rw / Pf
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / Pf))
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / Pf))
    return sh, sw, bh, bw, gh, gw


def axis_weights(start, bsz, g, size, P, ft=np.float64):
    """[P, size] float64: per output index the summed bilinear weights its g samples give every row (column) of the map.
    Positions `start + p * bsz + (i + 0.5) * bsz / g`, the `< -1 || > size` skip, the clamps at 0 and size - 1 and the weights
    `l = v - lo`, `1 - l` are computed in `ft`, operation by operation as the kernel writes them; the sums are float64."""
    m = np.zeros((P, size))
    if g <= 0:
        return m
    p, i = np.arange(P, dtype=ft)[:, None], np.arange(g, dtype=ft)[None, :]
    v = (start + p * bsz) + ((i + ft(0.5)) * bsz) / ft(g)
    keep = ~((v < ft(-1.0)) | (v > ft(size)))
    v = np.where(v <= ft(0.0), ft(0.0), v)
    lo = np.where(keep, v, 0).astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, lo, lo + 1)
    v = np.where(top, lo.astype(ft), v)
    l = (v - lo.astype(ft)).astype(ft)
    h = (ft(1.0) - l).astype(ft)
    rows = np.broadcast_to(np.arange(P)[:, None], lo.shape)
    np.add.at(m, (rows[keep], lo[keep]), h[keep].astype(np.float64))
    np.add.at(m, (rows[keep], hi[keep]), l[keep].astype(np.float64))
    return m


def roi_align_fp64(x, rois, P, scale, sampling_ratio, aligned, geometry=np.float64, magnitude=False):
    """torchvision roi_align restated in float64, separably: per box and axis a dense [P, size] matrix of the summed bilinear
    weights of every sample (positions, the `< -1 || > size` skip, the clamps at 0 and size - 1 as oracle/tv_ops.c), then
    out[c, p, q] = sum_yx Wy[p, y] * x[c, y, x] * Wx[q, x] / max(gh * gw, 1).  Returns [K, C, P, P] float64.

    geometry=np.float32: the sample positions and the weights are the kernel's own fp32 numbers (csrc/fpn.hip is built without
    contraction, so one numpy fp32 operation per operation of the source reproduces them); the products and sums stay float64.
    magnitude=True: also returns sum |w * x| / count per element, the size the rounding bounds scale with."""
    x = np.asarray(x, dtype=np.float64)
    N, C_, H, W = x.shape
    out = np.zeros((len(rois), C_, P, P))
    mag = np.zeros_like(out) if magnitude else None
    xa = np.abs(x) if magnitude else None
    for k, r in enumerate(np.asarray(rois)):
        b = int(r[0])
        sh, sw, bh, bw, gh, gw = roi_geometry(r, P, scale, sampling_ratio, aligned, geometry)
        wy, wx = axis_weights(sh, bh, gh, H, P, geometry), axis_weights(sw, bw, gw, W, P, geometry)
        ys, xs = np.nonzero(wy.any(0))[0], np.nonzero(wx.any(0))[0]
        if len(ys) == 0 or len(xs) == 0:
            continue
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
        for src, dst in ((x, out), (xa, mag)):
            if src is not None:
                t = np.tensordot(src[b, :, y0:y1, x0:x1], wx[:, x0:x1], axes=(2, 1))             # [C, y, Q]
                dst[k] = np.tensordot(wy[:, y0:y1], t, axes=(1, 1)).transpose(1, 0, 2) / max(gh * gw, 1)
    return (out, mag) if magnitude else out


# ---- the library's entry points (device tensors; GPU tests only) ----------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def align_pyramid_one_level(L, feat_nhwc, rois, P, scale, sampling_ratio, aligned, dt):
    """The existing vk_roi_align on one level -> [K, P, P, C]."""
    N, H, W, C_ = feat_nhwc.shape
    K = rois.shape[0]
    out = torch.full((K, P, P, C_), 7.0, dtype=feat_nhwc.dtype, device=feat_nhwc.device)
    maps, Hs, Ws, sc = (C.c_void_p * 1)(feat_nhwc.data_ptr()), (C.c_int32 * 1)(H), (C.c_int32 * 1)(W), (C.c_float * 1)(scale)
    L.call("vk_roi_align", maps, Hs, Ws, sc, 1, N, C_, C.c_void_p(rois.data_ptr()), None, K, P, sampling_ratio, int(aligned),
           C.c_void_p(out.data_ptr()), dt, _stream())
    torch.cuda.synchronize()
    return out
