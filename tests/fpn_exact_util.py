"""TEST INFRASTRUCTURE ONLY -- shared by tests/test_fpn_exact_host.py (CPU) and tests/test_gpu_fpn_kernels.py (-m gpu): the
case tables of the three forms of vk_roi_align (csrc/fpn.hip), the exact sets they run on, the pyramid, and the per-element
bound of the cases that are not exact.  Builds on roi_align_c4_util (exact_map, exact_rois, roi_align_fp64).

The exact sets.  exact_map's integers in [-8, 8] and exact_rois' boxes (sides 56 .. 896 px, origins on multiples of 4 px) keep
every sample on a short dyadic position at scales 1/4 .. 1/32 with P in {7, 14, 16, 32} and sampling ratio 0, 1, 2 or 4, so
every summation order gives the same fp32 bits; tests/test_fpn_exact_host.py proves it for every (P, ratio, aligned, scale) of
exact_geometries() by comparing the fp32 oracle (oracle/tv_ops.c, per-sample order) with roi_align_fp64 bit for bit.  extra_rois
adds boxes of 3584 or 4096 px (bins of 16 cells and more at 1/16: beyond the separable kernel's tables) and, for `aligned`,
inverted boxes (negative bin sizes: the separable kernel's per-sample loop; with `aligned` off max(size, 1) makes them 1 / P
wide, which is not dyadic, so they stay out).

The bound of a case that is not exact.  ref is roi_align_fp64(geometry=np.float32): the kernel's own fp32 sample positions
and weights l, 1 - l, the products and sums in float64, so it differs from the kernel only by the roundings listed here.
With u = 2^-24, n = gh * gw samples and A = sum |w * x| / count over the samples and taps of the element:

    |out - ref| <= c u / (1 - c u) * A  +  half an ulp of the storage type at |ref| + that first term   (0 for f32)

per-sample forms (scalar, vec, the separable kernel's loop, the oracle): a term w * x is rounded twice (hy * hx, then * x),
passes at most 3 additions inside its sample's four-tap sum and at most n additions into the accumulator, then the division
by count:                                                       c_sample = n + 6
table form: an entry of a per-axis table is a sequential fp32 sum of at most 2 g weights (each sample adds 1 - l and l), so
an addend passes at most 2 g additions: 2 gh + 2 gw for the two axes; wy * wx and * x are one rounding each; the footprint
has T <= min(RA_T^2, 4 gh gw + 4) pixels (the `tables` predicate) and a term passes at most T additions; inv = 1 / count and
acc * inv are one rounding each:                                c_tables = 2 (gh + gw) + T + 4
c of a RoI is c_sample, or the larger of the two where the restated predicate says the separable kernel takes its tables.
The conversions of 16-bit inputs to fp32 are exact.  Nothing here is fitted to what a kernel returns."""
import ctypes as C

import numpy as np
import torch

from vltk_amd import _lib as L

import roi_align_c4_util as U

FORMS = ("sep", "vec", "scalar")                       # VK_RA_FORM_* by value
RA_T, RA_MAXP = 12, 16                                 # csrc/fpn.hip
U32 = 2.0 ** -24
TD = {L.VK_F32: torch.float32, L.VK_F16: torch.float16, L.VK_BF16: torch.bfloat16}
NAME = {L.VK_F32: "f32", L.VK_F16: "f16", L.VK_BF16: "bf16"}
F32, F16, BF16 = L.VK_F32, L.VK_F16, L.VK_BF16
S4, S8, S16, S32 = 1 / 4, 1 / 8, 1 / 16, 1 / 32
SENTINEL = 7.0


def form(C_, P, dt):
    """The kernel vk_roi_align runs on for this launch under the current environment, by name."""
    r = L.load().vk_roi_align_form(C_, P, dt)
    assert r >= 0, (C_, P, dt, r)
    return FORMS[r]


# ---- the case tables: (dtype, C) per form, and the (sampling ratio, aligned, scale) sets each runs --------------------------------
SCALAR_CASES = ((F32, 6), (F32, 70), (F16, 12), (BF16, 12), (F16, 260), (F32, 1028))       # P = 7
SCALAR_GEOMS = ((2, True, S16), (0, False, S16))
SCALAR_SCALE_GEOMS = ((0, True, S4), (2, True, S32))                                        # f32 C = 6 only
SEP_CASES = ((F16, 8), (BF16, 8), (F32, 40), (F32, 256), (F16, 256), (BF16, 256), (F16, 2048), (F32, 1024))      # P = 7 and 14
SEP_GEOMS = ((0, True, S16), (2, True, S16))
SEP_MORE_GEOMS = {7: ((1, True, S16), (4, False, S16), (0, False, S16), (2, False, S16), (0, True, S4), (2, True, S4), (0, True, S8),
                      (2, True, S8), (0, True, S32), (2, True, S32)),
                  14: ((1, True, S16), (4, False, S16), (0, False, S16), (2, False, S16)),
                  16: ((0, True, S16), (2, False, S16))}                                     # f16 C = 256 and f32 C = 40
VEC_P32_GEOMS = ((0, True, S16), (2, True, S16), (2, False, S16))                            # C = 256, three dtypes
VEC_ENV_GEOMS = ((0, True, S16), (2, True, S16), (4, False, S16))                            # P = 7 and 14 under VK_ROIALIGN_TABLES=0


def sep_geometries():
    """Every (P, sr, aligned, scale) the separable kernel runs on the exact sets."""
    out = [(P, *g) for P in (7, 14) for g in SEP_GEOMS]
    out += [(P, *g) for P, gs in SEP_MORE_GEOMS.items() for g in gs]
    return out


def exact_geometries():
    """Every (P, sr, aligned, scale) a GPU test runs bit for bit."""
    out = set(sep_geometries())
    out |= {(7, *g) for g in SCALAR_GEOMS + SCALAR_SCALE_GEOMS}
    out |= {(32, *g) for g in VEC_P32_GEOMS}
    out |= {(P, *g) for P in (7, 14) for g in VEC_ENV_GEOMS}
    return sorted(out)


# ---- the exact sets -------------------------------------------------------------------------------------------------------------
MAP_C = 2048
_CACHE = {}


def exact_map_wide():
    """[2, 2048, 40, 44] f32 of integers in [-8, 8]; a case of C channels reads the first C."""
    if "map" not in _CACHE:
        _CACHE["map"] = U.exact_map(MAP_C, seed=5).numpy()
    return _CACHE["map"]


def extra_rois(aligned, P):
    """Six boxes of 3584 px (P = 7, 14: bins of 32 and 16 cells at 1/16) or 4096 px (P = 16, 32) over the map; inverted ones."""
    side = 3584 if P % 7 == 0 else 4096
    rows = [[b, x0, y0, x0 + side, y0 + side] for b, x0, y0 in ((0, -1792, -1792), (1, -3072, -2048), (0, -512, -256), (1, 64, 32),
                                                                (0, -3264, -3232), (1, -1024, -3200))]
    if aligned:
        rows += [[0, 448, 320, 224, 96], [1, 600, 200, 152, 144], [0, 116, 560, 60, 112], [1, 900, 500, 4, 52],
                 [0, 224, 64, 112, 176], [1, 64, 448, 288, 0]]
    return np.asarray(rows, dtype=np.float32)


def exact_boxes(aligned, P):
    """exact_rois and extra_rois(aligned, P): [K, 5] f32."""
    return np.concatenate([U.exact_rois(), extra_rois(aligned, P)])


def sep_takes_tables(r, P, scale, sr, aligned):
    """The `tables` predicate of roi_align_sep_kernel for one RoI row, in fp32 as the kernel evaluates it."""
    f = np.float32
    sh, sw, bh, bw, gh, gw = U.roi_geometry(r, P, scale, sr, aligned, f)
    nyb = np.floor(bh * f(gh - 1) / f(gh)) + f(3) if gh > 1 else f(2)
    nxb = np.floor(bw * f(gw - 1) / f(gw)) + f(3) if gw > 1 else f(2)
    return bool(bh >= 0 and bw >= 0 and nyb <= f(RA_T) and nxb <= f(RA_T) and nyb * nxb <= f(4) * f(gh) * f(gw) + f(4))


def exact_reference(P, sr, aligned, scale, C_):
    """(rois [K, 5] f32, roi_align_fp64 [K, C_, P, P]) of an exact set on the first C_ channels of exact_map_wide; computed once
    per geometry at the widest C asked so far."""
    key = (P, sr, aligned, scale)
    rois = exact_boxes(aligned, P)
    if key not in _CACHE or _CACHE[key].shape[1] < C_:
        _CACHE[key] = U.roi_align_fp64(exact_map_wide()[:, :C_], rois, P, scale, sr, aligned)
    return rois, _CACHE[key][:, :C_]


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------
PYR_SCALES = (S4, S8, S16, S32)
PYR_HW = ((160, 176), (80, 88), (40, 44), (20, 22))          # a 640 x 704 image
PYR_P, PYR_SR = 7, 2


def pyramid_maps(C_):
    """Four [2, C_, H, W] f32 maps of different integers in [-8, 8] (the first C_ of 256 channels)."""
    if "pyr" not in _CACHE:
        _CACHE["pyr"] = [np.random.Generator(np.random.PCG64(40 + i)).integers(-8, 9, (2, 256, h, w)).astype(np.float32)
                         for i, (h, w) in enumerate(PYR_HW)]
    return [m[:, :C_] for m in _CACHE["pyr"]]


def permuted_levels(levels):
    """Every third box moves one level up (the coarsest wraps to the finest): levels the rule would not choose."""
    lv = np.asarray(levels).copy()
    lv[::3] = (lv[::3] + 1) % len(PYR_SCALES)
    return lv


def pyramid_reference(levels, C_, sr=PYR_SR):
    """Per RoI of exact_rois, roi_align_fp64 on its level's map and scale -> [K, C_, P, P]."""
    rois, maps = U.exact_rois(), pyramid_maps(C_)
    out = np.zeros((len(rois), C_, PYR_P, PYR_P))
    for li, (m, s) in enumerate(zip(maps, PYR_SCALES)):
        idx = np.nonzero(np.asarray(levels) == li)[0]
        if len(idx):
            out[idx] = U.roi_align_fp64(m, rois[idx], PYR_P, s, sr, True)
    return out


# ---- not exact: boxes, reference, bound ----------------------------------------------------------------------------------------------
ROUGH_MAP = (2, 40, 44)


def rough_map(C_, td):
    """[2, C_, 40, 44] standard normal values, rounded to the storage type (f32 numpy)."""
    x = np.random.Generator(np.random.PCG64(77)).standard_normal((ROUGH_MAP[0], 256, *ROUGH_MAP[1:])).astype(np.float32)
    return torch.from_numpy(x[:, :C_]).to(td).float().numpy()


def rough_rois():
    """The random boxes of test_gpu_fpn._rois at scale 1/16 on the 40 x 44 map (outside, empty, larger than the map), inverted
    ones, and boxes with sides below one cell (16 px), where max(size, 1) of `aligned = False` bites."""
    from test_gpu_fpn import _rois
    N, H, W = ROUGH_MAP
    gen = np.random.Generator(np.random.PCG64(78))
    r = _rois(gen, 40, N, W * 16, H * 16)
    inv = np.asarray([[0, 300.5, 200.25, 100.0, 90.0], [1, 90.0, 80.0, 40.0, 20.0], [0, 50.0, 400.0, 350.0, 100.0],
                      [1, 350.0, 100.0, 50.0, 400.0]], np.float32)
    xy = gen.uniform(0, [W * 16 - 16, H * 16 - 16], (12, 2))
    wh = gen.uniform(0.1, 15.0, (12, 2))
    tiny = np.concatenate([gen.integers(0, N, (12, 1)), xy, xy + wh], 1).astype(np.float32)
    return np.concatenate([r, inv, tiny])


ROUGH_GEOMS = {"sep": ((7, 3, True), (7, 0, False), (14, 2, False)), "vec": ((20, 0, True), (20, 3, False)),
               "scalar": ((7, 3, True), (7, 0, False))}
ROUGH_CASES = {"sep": ((F32, 40), (F16, 256), (BF16, 256)), "vec": ((F32, 64), (F16, 256), (BF16, 256)),
               "scalar": ((F32, 6), (F16, 12), (BF16, 12))}


def half_ulp(v, td):
    """Half the spacing of the storage type at |v| (0 for f32, which stores the fp32 result as it is)."""
    if td == torch.float32:
        return np.zeros_like(v)
    bits, emin = (10, -14) if td == torch.float16 else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - bits)


def bound_c(rois, P, scale, sr, aligned):
    """c per RoI, as the module docstring derives it."""
    out = np.zeros(len(rois))
    for k, r in enumerate(rois):
        _, _, _, _, gh, gw = U.roi_geometry(r, P, scale, sr, aligned, np.float32)
        n = max(gh, 0) * max(gw, 0)
        c = n + 6
        if sep_takes_tables(r, P, scale, sr, aligned):
            c = max(c, 2 * (gh + gw) + min(RA_T * RA_T, 4 * gh * gw + 4) + 4)
        out[k] = c
    return out


def rough_reference(x, rois, P, scale, sr, aligned, td):
    """(ref, bound) [K, C, P, P] float64 of a case that is not exact."""
    ref, mag = U.roi_align_fp64(x, rois, P, scale, sr, aligned, geometry=np.float32, magnitude=True)
    c = bound_c(rois, P, scale, sr, aligned)[:, None, None, None]
    b32 = c * U32 / (1 - c * U32) * mag
    return ref, b32 + half_ulp(np.abs(ref) + b32, td)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, an element with bound 0 counting as 0 when it is exact and infinite when not."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max())


# ---- the library's entry point (device tensors; GPU tests only) ---------------------------------------------------------------------
def run_roi_align(maps_nhwc, scales, rois, levels, P, sr, aligned, dt, expect_form):
    """vk_roi_align over device maps [N, H, W, C] -> [K, P, P, C] on the CPU; the form is asserted before the launch, the maps and
    the output are 16-byte aligned, and one sentinel row behind the output must stay untouched."""
    n = len(maps_nhwc)
    N, _, _, C_ = maps_nhwc[0].shape
    K = rois.shape[0]
    assert form(C_, P, dt) == expect_form, f"C={C_} P={P} {NAME[dt]}: runs on {form(C_, P, dt)}, the test expects {expect_form}"
    out = torch.full((K + 1, P, P, C_), SENTINEL, dtype=TD[dt], device=maps_nhwc[0].device)
    assert out.data_ptr() % 16 == 0 and all(m.data_ptr() % 16 == 0 and m.is_contiguous() and m.dtype == TD[dt] for m in maps_nhwc)
    ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in maps_nhwc])
    Hs, Ws = (C.c_int32 * n)(*[m.shape[1] for m in maps_nhwc]), (C.c_int32 * n)(*[m.shape[2] for m in maps_nhwc])
    L.call("vk_roi_align", ptrs, Hs, Ws, (C.c_float * n)(*scales), n, N, C_, C.c_void_p(rois.data_ptr()),
           C.c_void_p(levels.data_ptr()) if levels is not None else None, K, P, sr, int(aligned), C.c_void_p(out.data_ptr()), dt,
           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[K] == SENTINEL).all()), "the row behind the output was written"
    return out[:K]
