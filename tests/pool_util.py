"""TEST INFRASTRUCTURE ONLY -- references and case builders for the memory-bound kernels of the C4 detector
(csrc/pool.hip: layout converters, max-pool, RoIPool, mean-pool) and vk_box_decode (csrc/rpn.hip).  Nothing here touches a
GPU: tests/test_pool_util_host.py checks the references against each other on the CPU, tests/test_gpu_pool_kernels.py holds
the kernels to them.

The bound of a decoded box (`box_decode_ref64`).  With u = 2^-24 and every input an fp32 number, apply_deltas1 rounds at

    widths = a2 - a0                        (1)     dx = d0 / wx,  dw = d2 / ww            (1 each)
    ctr_x  = a0 + 0.5 widths                (1; the product by 0.5 is exact)
    pcx    = dx widths + ctr_x              (2: product, sum; no FMA, rpn.hip is built with -ffp-contract=off)
    pw     = expf(dw) widths                (expf, then 1)
    x0, x1 = pcx -+ 0.5 pw                  (1 each)

and the same for y.  The reference evaluates these in fp64 and carries, next to each value V, a bound e on the distance of the
fp32 value from it: an input error moves a sum by the sum of the errors, a product X Y by |X| e_y + |Y| e_x + e_x e_y, and the
rounding of a result adds u (|V| + e).  min(dw, clamp) moves by no more than dw does.  exp(dw) moves by exp(DW) expm1(e_dw),
and the device's expf adds E ulp of its own result: 2 E u (exp(DW) + what it moved by), an ulp being at most 2^-23 of the value.

E = 1.  The figure is the one AMD publishes for the device function: the HIP documentation's table of single-precision
mathematical functions lists expf with a maximum error of 1 ulp.  It fits how the device library builds it: x log2(e) as a
compensated product (the rounding error of the product is carried into the reduced argument with an fma), v_exp_f32 of the
reduced argument, which the ISA guide gives as 1 ulp, and an exact scaling by the power of two.  (tests/lxmert_pretrain_util.py
takes the same 1 ulp for v_exp_f32 behind `__expf`.)  The bound is a derived worst case and carries no margin beyond that;
it holds for operands and results in the normal range, which the cases of the tests are.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import frcnn_oracle as orc

U32 = 2.0 ** -24
EXPF_ULP = 1                                             # E of the docstring
FLT_MAX = np.finfo(np.float32).max
SCALE_CLAMP = np.float32(math.log(1000.0 / 16.0))       # (float)log(1000.0 / 16.0) of vk_box_decode


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def bits(a):
    """The bit pattern of an fp32 / f16 array, for comparisons that tell -0.0 from 0.0."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 2: np.int16}[a.dtype.itemsize])


def assert_same_bits(got, want):
    """Bitwise equality of two float arrays; where `want` is NaN, `got` must be a NaN (of any payload)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(np.where(nan, 0, bits(got)), np.where(nan, 0, bits(want)))


# ---- layout converters ---------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 5, 3, 1), (3, 16, 9, 4)]
LAYOUT_OVER_CAP = (1, 8, 363, 363)                       # 1 054 152 elements > 4096 workgroups x 256
F16_SUBNORMAL = 3 * 2.0 ** -24
LAYOUT_SPECIALS = (float("inf"), float("-inf"), float("nan"), -0.0, F16_SUBNORMAL, 70000.0, -70000.0)


def index_tensor(shape):
    """[N,C,H,W] fp32 whose every element is its own linear index mod 2048 (exact in f16)."""
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.int64) % 2048).to(torch.float32).reshape(shape)


def specials_tensor(shape=(2, 3, 5, 7)):
    """index_tensor with LAYOUT_SPECIALS strewn over it, in each image and in several channels."""
    x = index_tensor(shape).reshape(-1)
    n = x.numel()
    for j, v in enumerate(LAYOUT_SPECIALS * 3):
        x[(j * 37 + 11) % n] = v
    return x.reshape(shape)


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x, caffe):
    """BasicStem's pool on the CPU in fp32: 3x3 stride 2, caffe = pad 0 + ceil_mode, else pad 1.  x [N,C,H,W]."""
    x = x.to(torch.float32)
    return F.max_pool2d(x, 3, 2, 0, ceil_mode=True) if caffe else F.max_pool2d(x, 3, 2, 1)


# ---- RoIPool -----------------------------------------------------------------------------------------------------------------------
ROI_MAP = (3, 320, 16, 16)                                # N, C, H, W: f16 runs all 320 channels, fp32 the first 160
ROI_P = (1, 2, 7, 14)
ROI_SCALES = (1.0 / 16, 1.0 / 32, 1.0)


def roi_pool_ref(x, rois, P, scale):
    """The oracle's restatement of torchvision's CPU kernel (oracle/tv_ops.c).  x [N,C,H,W], rois [K,5] -> [K,C,P,P]."""
    return orc.roi_pool(torch.as_tensor(x), torch.as_tensor(np.asarray(rois, dtype=np.float32)), P, scale)


def _roundf(v):
    """C's roundf of an fp32 number: half away from zero (in fp64, where v +- 0.5 is exact)."""
    v = float(v)
    t = math.trunc(v)
    return t + (int(math.copysign(1, v)) if abs(v - t) >= 0.5 else 0)


def roi_pool_by_hand(x, roi, P, scale):
    """RoIPool of ONE RoI, written from torchvision's rule without a look at oracle/tv_ops.c's loop: the box corners times the
    scale in fp32, rounded half away from zero; width and height at least 1; fp32 bin = size / P; bin ph covers
    floor(ph bin) .. ceil((ph + 1) bin) from the rounded corner, clamped to the map; an empty bin gives 0, any other the
    maximum started at -FLT_MAX and taken with `>`, so a NaN never wins.  x [N,C,H,W] fp32 numpy, roi (b, x1, y1, x2, y2)
    -> [C,P,P]."""
    x = np.asarray(x, dtype=np.float32)
    _, C, H, W = x.shape
    f = np.float32
    b = int(roi[0])
    x1, y1, x2, y2 = (_roundf(f(v) * f(scale)) for v in roi[1:])
    roi_w, roi_h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    bin_w, bin_h = f(roi_w) / f(P), f(roi_h) / f(P)
    assert bin_w.dtype == np.float32 and bin_h.dtype == np.float32

    def span(p, size, start, limit):
        lo = int(np.floor(f(p) * size)) + start
        hi = int(np.ceil(f(p + 1) * size)) + start
        return min(max(lo, 0), limit), min(max(hi, 0), limit)
    out = np.zeros((C, P, P), dtype=np.float32)
    for ph in range(P):
        hs, he = span(ph, bin_h, y1, H)
        for pw in range(P):
            ws, we = span(pw, bin_w, x1, W)
            if he <= hs or we <= ws:
                continue
            m = np.full(C, -FLT_MAX, dtype=np.float32)
            for h in range(hs, he):
                for w in range(ws, we):
                    v = x[b, :, h, w]
                    m = np.where(v > m, v, m)
            out[:, ph, pw] = m
    return out


def roi_feature_map():
    """The RoIPool tests' map: standard normal rounded to f16, so both types read the same values."""
    return torch.from_numpy(rng(29).standard_normal(ROI_MAP).astype(np.float32)).half().float()


def cell_ranges(lo=-2, hi=17):
    return [(s, e) for s in range(lo, hi + 1) for e in range(s, hi + 1)]


def sweep_rois(scale):
    """Every integer cell range [s, e], -2 <= s <= e <= 17, as the rows of a RoI (heights 1 .. 20: with P in 1, 2, 7, 14 the
    products ph * bin land on integers, e.g. 14 / 7, and next to them, e.g. 7 * fl(3 / 7)), each paired with a column range
    by the fixed permutation i -> 11 i + 5 mod 210; given in pixels as cell / scale, exact for the three scales; the image
    cycles over 0, 1, 2."""
    rows = cell_ranges()
    n = len(rows)
    assert n == 210 and math.gcd(11, n) == 1
    inv = 1.0 / scale
    assert inv == round(inv)
    r = []
    for i, (rs, re) in enumerate(rows):
        cs, ce = rows[(11 * i + 5) % n]
        r.append([i % ROI_MAP[0], cs * inv, rs * inv, ce * inv, re * inv])
    return np.asarray(r, dtype=np.float32)


# in cells of the 16 x 16 map: (image, x1, y1, x2, y2)
HAND_ROIS_CELLS = [
    (0, -0.5, -0.5, 2.5, 2.5),        # roundf(-0.5) = -1, roundf(2.5) = 3
    (1, 0.5, 0.5, 2.5, 4.0),          # roundf(0.5) = 1
    (2, -0.5, 0.5, 0.5, 2.5),
    (0, 2.5, -0.5, 9.0, 0.5),
    (1, 9.0, 3.0, 4.0, 8.0),          # x2 < x1: width forced to 1
    (2, 3.0, 12.0, 11.0, 5.0),        # y2 < y1
    (0, -9.0, 2.0, -3.0, 9.0),        # outside on the left
    (1, 18.0, 2.0, 25.0, 9.0),        # ... the right
    (2, 2.0, -12.0, 9.0, -2.0),       # ... the top
    (0, 2.0, 17.0, 9.0, 30.0),        # ... the bottom
    (1, 5.0, 7.0, 5.0, 7.0),          # one cell
    (2, 0.0, 0.0, 15.0, 15.0),        # the whole map
    (0, -4.0, -4.0, 20.0, 20.0),      # the whole map and a margin all round
]


def hand_rois(scale):
    return np.asarray([[b] + [v / scale for v in box] for b, *box in HAND_ROIS_CELLS], dtype=np.float32)


def hand_expected(x, rois, P, scale):
    return np.stack([roi_pool_by_hand(x, r, P, scale) for r in rois])


# ---- mean-pool ---------------------------------------------------------------------------------------------------------------------
def mean_pool_ref(x):
    """box_features.mean over the S positions: the fp64 sum over fp64 S, rounded to fp32.  x [K,S,C] -> [K,C] fp32.

    On small integers the kernel has to give these bits.  Its partial sums are integers far below 2^24, exact in fp32 in
    any order, so the one rounding it makes is sum / S -- and the fp64 quotient rounded again to fp32 is the correctly rounded
    fp32 quotient: for operands of at most 24 bits a 53-bit quotient cannot lie close enough to the middle of two fp32
    numbers for the second rounding to cross it, since 53 >= 2 * 24 + 2."""
    x = torch.as_tensor(x).to(torch.float64)
    return (x.sum(1) / float(x.shape[1])).to(torch.float32)


def integer_features(K, S, C, seed=0):
    """[K,S,C] fp32 of integers in [-8, 8]."""
    return torch.from_numpy(rng(1000 * K + 10 * S + C + seed).integers(-8, 9, size=(K, S, C)).astype(np.float32))


MEAN_K = (1, 3)
MEAN_S = (1, 2, 3, 4, 5, 49, 196)
MEAN_C = {"fp16": (8, 504, 512, 520, 2048), "fp32": (4, 252, 256, 260, 2048)}      # 1, 63, 64, 65 and 256 16-byte chunks


# ---- box decode --------------------------------------------------------------------------------------------------------------------
def box_decode_ref32(deltas, boxes, weights, exp=torch.exp):
    """Box2BoxTransform.apply_deltas in fp32 with the reference's operation order (FRCNNOracle.apply_deltas; rpn.hip:49-69):
    every product and sum rounded on its own, IEEE division, the clamp before the exponential.  Everything but the
    exponential is fixed by IEEE 754, so the kernel matches these bits wherever exp's argument is 0 or -inf.
    deltas [M, 4k], boxes [M, 4] -> [M, 4k] fp32."""
    d = torch.as_tensor(deltas, dtype=torch.float32)
    a = torch.as_tensor(boxes, dtype=torch.float32)
    M = d.shape[0]
    d = d.reshape(M, -1, 4)
    wx, wy, ww, wh = (float(w) for w in weights)
    clamp = torch.tensor(SCALE_CLAMP)
    widths = (a[:, 2] - a[:, 0])[:, None]
    heights = (a[:, 3] - a[:, 1])[:, None]
    ctr_x = a[:, 0, None] + 0.5 * widths
    ctr_y = a[:, 1, None] + 0.5 * heights
    dx, dy = d[..., 0] / wx, d[..., 1] / wy
    dw, dh = d[..., 2] / ww, d[..., 3] / wh
    dw = torch.where(dw > clamp, clamp, dw)
    dh = torch.where(dh > clamp, clamp, dh)
    pcx = dx * widths + ctr_x
    pcy = dy * heights + ctr_y
    pw = exp(dw) * widths
    ph = exp(dh) * heights
    out = torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1)
    assert out.dtype == torch.float32
    return out.reshape(M, -1)


def box_decode_ref64(deltas, boxes, weights):
    """-> (the decoded boxes in fp64, the bound on |fp32 result - them| per element), both [M, 4k] fp64 numpy; the module's
    docstring derives the bound."""
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64)
    a = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    M = d.shape[0]
    d = d.reshape(M, -1, 4)
    w = [float(np.float32(v)) for v in weights]
    u = U32

    def rounded(v, e):                                        # the fp32 rounding of a result whose operands carry e
        return e + u * (np.abs(v) + e)

    def axis(lo, hi, dc, ds, wc, ws):
        size = (hi - lo)[:, None]
        e_size = rounded(size, 0.0)
        ctr = lo[:, None] + 0.5 * size
        e_ctr = rounded(ctr, 0.5 * e_size)
        t = dc / wc
        e_t = rounded(t, 0.0)
        s = ds / ws
        e_s = rounded(s, 0.0)
        s = np.minimum(s, float(SCALE_CLAMP))
        prod = t * size
        e_prod = rounded(prod, np.abs(t) * e_size + np.abs(size) * e_t + e_t * e_size)
        pc = prod + ctr
        e_pc = rounded(pc, e_prod + e_ctr)
        ex = np.exp(s)
        e_ex = ex * np.expm1(e_s)
        e_ex = e_ex + 2 * EXPF_ULP * u * (ex + e_ex)
        p = ex * size
        e_p = rounded(p, ex * e_size + np.abs(size) * e_ex + e_ex * e_size)
        v0, v1 = pc - 0.5 * p, pc + 0.5 * p
        return v0, rounded(v0, e_pc + 0.5 * e_p), v1, rounded(v1, e_pc + 0.5 * e_p)
    x0, ex0, x1, ex1 = axis(a[:, 0], a[:, 2], d[..., 0], d[..., 2], w[0], w[2])
    y0, ey0, y1, ey1 = axis(a[:, 1], a[:, 3], d[..., 1], d[..., 3], w[1], w[3])
    return np.stack((x0, y0, x1, y1), -1).reshape(M, -1), np.stack((ex0, ey0, ex1, ey1), -1).reshape(M, -1)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, the figure the box-decode tests print before they assert it <= 1."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / bound).max())


def decode_boxes(M, seed=0):
    """[M,4] fp32 anchors with fractional corners, widths and heights of 4 .. 400 pixels."""
    g = rng(7 + seed)
    x0, y0 = g.uniform(-50, 1200, M), g.uniform(-50, 700, M)
    return np.stack((x0, y0, x0 + g.uniform(4, 400, M), y0 + g.uniform(4, 400, M)), 1).astype(np.float32)


def decode_deltas(M, k, weights, translation_only, seed=0):
    """[M, 4k] fp32 deltas as the heads produce them times the weights: dx, dy about +-0.5 box sizes, dw, dh about +-1 (or 0)."""
    g = rng(13 + seed)
    d = g.standard_normal((M, k, 4)) * np.asarray([0.5, 0.5, 1.0, 1.0]) * np.asarray(weights, dtype=np.float64)
    if translation_only:
        d[..., 2:] = 0.0
    return d.reshape(M, 4 * k).astype(np.float32)


def delta_for(target, weight):
    """An fp32 delta d with fl(d / weight) == target, an fp32 number (d = target for an infinite one)."""
    target, weight = np.float32(target), np.float32(weight)
    if not np.isfinite(target):
        return target
    d = np.float32(target * weight)
    for _ in range(8):
        q = np.float32(d / weight)
        if q == target:
            return d
        d = np.nextafter(d, np.float32(np.inf) if q < target else np.float32(-np.inf))
    raise AssertionError(f"no fp32 delta gives {target!r} / {weight!r}")


def clamp_neighbours():
    """dw / ww just below, at, just above the clamp, and +inf: fp32 neighbours of (float)log(1000 / 16)."""
    c = SCALE_CLAMP
    return [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)), np.float32(np.inf)]
