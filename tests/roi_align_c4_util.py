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


def roi_align_fp64(x, rois, P, scale, sampling_ratio, aligned):
    """torchvision roi_align restated in float64, separably: per box and axis a dense [P, size] matrix of the summed bilinear
    weights of every sample (positions, the `< -1 || > size` skip, the clamps at 0 and size - 1 as oracle/tv_ops.c), then
    out[c, p, q] = sum_yx Wy[p, y] * x[c, y, x] * Wx[q, x] / max(gh * gw, 1).  Returns [K, C, P, P] float64."""
    x = np.asarray(x, dtype=np.float64)
    rois = np.asarray(rois, dtype=np.float64)
    N, C_, H, W = x.shape
    out = np.zeros((len(rois), C_, P, P))
    off = 0.5 if aligned else 0.0
    for k, r in enumerate(rois):
        b = int(r[0])
        sw, sh, ew, eh = (r[1:] * scale - off)
        rw, rh = ew - sw, eh - sh
        if not aligned:
            rw, rh = max(rw, 1.0), max(rh, 1.0)
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / P))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / P))
        mats = []
        for start, bsz, g, size in ((sh, rh / P, gh, H), (sw, rw / P, gw, W)):
            m = np.zeros((P, size))
            for p in range(P):
                for i in range(g):
                    v = start + p * bsz + (i + 0.5) * bsz / g
                    if v < -1.0 or v > size:
                        continue
                    v = max(v, 0.0)
                    lo = int(v)
                    if lo >= size - 1:
                        lo = hi = size - 1
                        v = float(lo)
                    else:
                        hi = lo + 1
                    m[p, lo] += 1.0 - (v - lo)
                    m[p, hi] += v - lo
            mats.append(m)
        out[k] = np.einsum("py,cyx,qx->cpq", mats[0], x[b], mats[1]) / max(gh * gw, 1)
    return out


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
