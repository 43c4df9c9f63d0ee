"""TEST INFRASTRUCTURE ONLY -- shared by tests/test_preprocess_kernel_host.py (CPU) and tests/test_gpu_preprocess_kernel.py
(-m gpu): vk_preprocess (csrc/preprocess.hip) called directly, with `new_hw` chosen by the test.

contract_reference restates the kernel's contract comment: per axis scale = in / out (an fp32 division), src =
fmaf(scale, dst + 0.5, -0.5) clamped at 0 (formed in float64, where the product and the sum are exact, and rounded to fp32
once), the lower tap floor(src), the upper one a step further unless it is the last, lambda1 = src - floor (exact),
lambda0 = 1 - lambda1 (one fp32 rounding).  With these fp32 weights the interpolation, the subtraction and the division are
float64.

The bound.  u = 2^-24, m = the largest |tap| of the element's four, all of one channel:
  top = fmaf(p01, w1, p00 * w0) and bot likewise: two roundings each (the product, the fma), each of a number <= m (w0 + w1 is
  1 to within u): |top - exact| <= 2 u m.  v = fmaf(bot, h1, top * h0) carries h0 * 2 u m + h1 * 2 u m = 2 u m of that and adds
  two roundings of its own: |v - exact| <= 4 u m.  d = v - mean is one rounding of a number <= m + |mean|; d / std one more.
      |out - ref| <= u (4 m + 2 (m + |mean|)) / |std|  <=  6 u (m + |mean|) / |std|
c = 6: two per fmaf stage, the subtract, the divide.  (1 + 2^-20) covers the second-order terms."""
import ctypes as C

import numpy as np
import torch

from vltk_amd import _lib as L

MEAN = (102.9801, 115.9465, 122.7717)
STD = (57.375, 57.12, 58.395)                 # distinct, no power of two: a wrong index or a multiply changes every value
PAD = -3.5
SENTINEL = 1234.5
C_BOUND = 6
U32 = 2.0 ** -24
GENERAL = (((1, 1), (3, 5)), ((1, 7), (4, 7)), ((7, 1), (7, 4)), ((5, 7), (8, 11)), ((37, 53), (8, 11)), ((20, 40), (33, 65)),
           ((20, 40), (9, 129)))              # (raw h, w), (new h, w)
DYADIC = (((6, 9), (12, 18)), ((12, 18), (6, 9)), ((16, 24), (4, 6)))
IDENTITY = ((5, 7), (9, 70))


def raw_image(h, w, seed, integers=False):
    gen = np.random.Generator(np.random.PCG64(seed))
    return (gen.integers(0, 256, (h, w, 3)) if integers else gen.uniform(0, 255, (h, w, 3))).astype(np.float32)


def axis_taps(size, new):
    """-> (lower tap, upper tap, lambda0, lambda1) of every output index along an axis, the weights as fp32 numbers."""
    f = np.float32
    scale = f(size) / f(new)
    src = (np.float64(scale) * (np.arange(new, dtype=np.float64) + 0.5) - 0.5).astype(f)          # fmaf: one rounding
    src = np.where(src < 0, f(0), src)
    lo = src.astype(np.int64)
    hi = lo + (lo < size - 1)
    l1 = (src - lo.astype(f)).astype(f)
    l0 = (f(1) - l1).astype(f)
    return lo, hi, l0, l1


def contract_reference(raw, new_h, new_w, mean, std):
    """-> (ref, bound), [3, new_h, new_w] float64, for a raw HWC f32 image; mean and std as the kernel receives them (fp32)."""
    H, W, _ = raw.shape
    y0, y1, h0, h1 = axis_taps(H, new_h)
    x0, x1, w0, w1 = axis_taps(W, new_w)
    r = raw.astype(np.float64)
    p00, p01, p10, p11 = r[y0][:, x0], r[y0][:, x1], r[y1][:, x0], r[y1][:, x1]               # [new_h, new_w, 3]
    w0, w1 = w0.astype(np.float64)[None, :, None], w1.astype(np.float64)[None, :, None]
    h0, h1 = h0.astype(np.float64)[:, None, None], h1.astype(np.float64)[:, None, None]
    v = (p01 * w1 + p00 * w0) * h0 + (p11 * w1 + p10 * w0) * h1
    mean = np.asarray(mean, np.float32).astype(np.float64)
    std = np.asarray(std, np.float32).astype(np.float64)
    m = np.maximum(np.maximum(np.abs(p00), np.abs(p01)), np.maximum(np.abs(p10), np.abs(p11)))
    ref = (v - mean) / std
    bound = C_BOUND * U32 * (1 + 2.0 ** -20) * (m + np.abs(mean)) / np.abs(std)
    return ref.transpose(2, 0, 1), bound.transpose(2, 0, 1)


def fma32(a, b, c):
    """fmaf on fp32 arrays through float64 (the product is exact there; the sum's second rounding is far below the bound)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def contract_fp32(raw, new_h, new_w, mean, std):
    """The kernel's arithmetic, operation by operation in fp32 -> [3, new_h, new_w] f32."""
    H, W, _ = raw.shape
    y0, y1, h0, h1 = axis_taps(H, new_h)
    x0, x1, w0, w1 = axis_taps(W, new_w)
    p00, p01, p10, p11 = raw[y0][:, x0], raw[y0][:, x1], raw[y1][:, x0], raw[y1][:, x1]
    w0, w1, h0, h1 = (np.broadcast_to(a, p00.shape) for a in (w0[None, :, None], w1[None, :, None], h0[:, None, None], h1[:, None, None]))
    top, bot = fma32(p01, w1, p00 * w0), fma32(p11, w1, p10 * w0)
    v = fma32(bot, h1, top * h0)
    return ((v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).transpose(2, 0, 1)


def worst_ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


def batch_geometry(N):
    """N distinct pairs of tiny raw and new sizes, 3..9 x 3..11 each."""
    raw_hw = [(3 + i % 7, 3 + (i // 7) % 9) for i in range(N)]
    new_hw = [(3 + (3 * i + 1) % 7, 3 + (5 * i + 2 + i // 63) % 9) for i in range(N)]
    assert len(set(zip(raw_hw, new_hw))) == N
    return raw_hw, new_hw


# ---- the library's entry point (GPU tests only) ---------------------------------------------------------------------------------------
def run_preprocess(raws, new_hw, Hmax, Wmax, mean=MEAN, std=STD, pad=PAD, null_at=None, expect=L.VK_OK):
    """vk_preprocess on numpy HWC images -> [N + 1, 3, Hmax, Wmax] f32 on the CPU: the output is allocated with one more image
    slot, everything filled with SENTINEL before the call.  Returns (status, the whole buffer)."""
    N = len(raws)
    dev = [torch.from_numpy(np.ascontiguousarray(r)).to("cuda:0") for r in raws]
    ptrs = (C.c_void_p * N)(*[d.data_ptr() for d in dev])
    if null_at is not None:
        ptrs[null_at] = None
    raw_hw = np.asarray([r.shape[:2] for r in raws], np.int32)
    new_hw = np.asarray(new_hw, np.int32)
    out = torch.full((N + 1, 3, Hmax, Wmax), SENTINEL, dtype=torch.float32, device="cuda:0")
    status = L.load().vk_preprocess(ptrs, raw_hw.ctypes.data_as(C.c_void_p), new_hw.ctypes.data_as(C.c_void_p), N, Hmax, Wmax,
                                    (C.c_float * 3)(*mean), (C.c_float * 3)(*std), pad, out.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == expect, (status, L.load().vk_last_error())
    return status, out.cpu().numpy()
