"""N4: host-side mirrors of the FPN-side pieces, all arithmetic in libvltk_hip.so.

* `FPNNeck`            detectron2-style FPN (lateral 1x1 + nearest-2x top-down + 3x3 output convs, P6 by LastLevelMaxPool
                       frcnn.py:825-836) over NHWC maps [C2..C5] -- the reference has no neck class: parity unpinned.
* `LastLevelP6P7`      frcnn.py:839-854.
* `MultiLevelRoIAlign` ROIPooler.forward's level loop (frcnn.py:1200-1224) with RoIAlign instead of RoIPool and the level rule
                       of assign_boxes_to_levels (frcnn.py:444-460).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .layers import DTYPES, Conv, stream


def _conv(w, b, precision, dev, stride=1):
    """conv + bias, padded by half the kernel; weights [cout, cin, k, k] f32."""
    return Conv(w, precision, dev, bias=b, stride=stride, pad=np.shape(w)[2] // 2)


class FPNNeck:
    def __init__(self, lateral, output, precision="fp16", device="cuda:0"):
        """lateral[i] / output[i] = (weight, bias) of level i's 1x1 / 3x3 conv, fine -> coarse (C2..C5)."""
        if not torch.cuda.is_available():
            raise RuntimeError("vltk_amd.fpn needs a GPU: there is no CPU fallback")
        self.dt, self.tdt = DTYPES[precision]
        self.dev = torch.device(device)
        self.lat = [_conv(w, b, precision, self.dev) for w, b in lateral]
        self.out = [_conv(w, b, precision, self.dev) for w, b in output]

    def __call__(self, feats, p6=True):
        """feats: NHWC device tensors [C2, ..., C5] -> [P2, ..., P5, P6]; without P6 when `p6` is false (the FPN detector's
        4-level RPN and its region features for given boxes)."""
        s = stream(self.dev)
        prev = self.lat[-1](feats[-1])
        res = [self.out[-1](prev)]
        for i in range(len(feats) - 2, -1, -1):
            lat = self.lat[i](feats[i])
            N, H, W, Cc = lat.shape
            y = torch.empty_like(lat)
            L.call("vk_upsample2x_add", lat.data_ptr(), prev.data_ptr(), y.data_ptr(), N, H, W, prev.shape[1], prev.shape[2], Cc, self.dt, s)
            prev = y
            res.insert(0, self.out[i](prev))
        if not p6:
            return res
        p5 = res[-1]
        N, H, W, Cc = p5.shape
        top = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=p5.dtype, device=self.dev)
        L.call("vk_subsample2", p5.data_ptr(), top.data_ptr(), N, H, W, Cc, self.dt, s)
        return res + [top]


class LastLevelP6P7:
    def __init__(self, w6, b6, w7, b7, precision="fp16", device="cuda:0"):
        self.dt, self.tdt = DTYPES[precision]
        self.dev = torch.device(device)
        self.p6 = _conv(w6, b6, precision, self.dev, stride=2)
        self.p7 = _conv(w7, b7, precision, self.dev, stride=2)

    def __call__(self, c5):
        p6 = self.p6(c5)
        r = torch.empty_like(p6)
        L.call("vk_relu_copy", p6.data_ptr(), r.data_ptr(), p6.numel(), self.dt, stream(self.dev))
        return p6, self.p7(r)


class MultiLevelRoIAlign:
    def __init__(self, output_size, scales, sampling_ratio=0, aligned=True, canonical_box_size=224, canonical_level=4, precision="fp16",
                 device="cuda:0"):
        self.P, self.scales = int(output_size), [float(s) for s in scales]
        self.sr, self.aligned = int(sampling_ratio), bool(aligned)
        self.min_level, self.max_level = int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1])))
        assert len(scales) == self.max_level - self.min_level + 1, "not a pyramid"          # frcnn.py:1168
        self.cbs, self.cl = float(canonical_box_size), int(canonical_level)
        self.dt, self.tdt = DTYPES[precision]
        self.dev = torch.device(device)

    def __call__(self, feats, rois, levels=None):
        """feats: NHWC maps fine -> coarse; rois [K,5] f32 (batch, x1, y1, x2, y2) -> ([K,P,P,C], levels [K]).  `levels`: the
        rois' levels as an int32 [K] device tensor when the caller has them already (vk_given_boxes_ingest); else assigned here."""
        rois = rois.to(self.dev, torch.float32).contiguous()
        K, nl = rois.shape[0], len(feats)
        s = stream(self.dev)
        if levels is None:
            levels = torch.zeros(K, dtype=torch.int32, device=self.dev)
            if nl > 1:
                L.call("vk_assign_levels", rois.data_ptr() + 4, 5, K, self.min_level, self.max_level, self.cbs, self.cl, levels.data_ptr(), s)
        N, _, _, Cc = feats[0].shape
        maps = (C.c_void_p * nl)(*[f.data_ptr() for f in feats])
        Hs = (C.c_int32 * nl)(*[f.shape[1] for f in feats])
        Ws = (C.c_int32 * nl)(*[f.shape[2] for f in feats])
        sc = (C.c_float * nl)(*self.scales)
        out = torch.empty((K, self.P, self.P, Cc), dtype=self.tdt, device=self.dev)
        L.call("vk_roi_align", maps, Hs, Ws, sc, nl, N, Cc, rois.data_ptr(), levels.data_ptr() if nl > 1 else None, K, self.P, self.sr,
               int(self.aligned), out.data_ptr(), self.dt, s)
        return out, levels
