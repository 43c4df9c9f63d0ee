"""-m gpu: the memory-bound kernels of the C4 detector (csrc/pool.hip) and vk_box_decode (csrc/rpn.hip) at their edges, through
the C ABI, against the references of tests/pool_util.py.

Every tensor is laid out with torch (`permute(...).contiguous()`), never with the project's own converters, so a misplacement
that both converters share cannot cancel.  Every output buffer is filled with NaN first and is one row longer than the kernel
may write; the row must come back untouched.  Comparisons are bitwise (`assert_same_bits`: -0.0 is not 0.0, a NaN must be a NaN)
except the general box decode, which is held per element to the bound derived in pool_util's docstring.

Grid caps and loops entered here and nowhere else directly: the converters' and the max-pool's grid-stride loop past
4096 workgroups x 256, RoIPool's second pass over `i += blockDim.x` in both types, mean-pool's idle row groups (S < 4) and its
second 64-lane pass, box decode's `m = i / k` across workgroups."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                 # noqa: E402

import gpu_util as G                           # noqa: E402
import pool_util as PU                         # noqa: E402

DTYPES = pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
NAME = {L.VK_F32: "fp32", L.VK_F16: "fp16"}
NAN = float("nan")


def guarded(rows, width, dtype):
    """A NaN-filled device buffer of `rows` rows for the kernel and one more that it must leave alone."""
    return torch.full((rows + 1, width), NAN, dtype=dtype, device=G.DEV)


def result(buf, shape):
    """The kernel's rows of a guarded buffer on the host, after checking that the extra row is still all NaN."""
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool(torch.isnan(host[-1]).all()), "the row after the output was written"
    return host[:-1].reshape(shape)


def nhwc(x, dt):
    """[N,C,H,W] fp32 on the host -> [N,H,W,C] of the kernel's type on the device, laid out by torch."""
    return x.permute(0, 2, 3, 1).contiguous().to(G.TDT[dt]).to(G.DEV)


def nchw32(y):
    """[N,H,W,C] host tensor -> [N,C,H,W] fp32 numpy."""
    return np.ascontiguousarray(y.float().permute(0, 3, 1, 2).numpy())


# ---- layout converters ---------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, dt):
    N, Cc, H, W = x.shape
    xd = x.contiguous().to(G.DEV)
    buf = guarded(N * H * W, Cc, G.TDT[dt])
    L.call("vk_nchw_to_nhwc", G.P(xd), N, Cc, H, W, G.P(buf), dt, G.stream())
    want = x.permute(0, 2, 3, 1).contiguous()
    PU.assert_same_bits(result(buf, (N, H, W, Cc)).numpy(), (want.half() if dt == L.VK_F16 else want).numpy())


def nhwc_to_nchw(x, dt):
    N, Cc, H, W = x.shape
    xd = nhwc(x, dt)
    buf = guarded(N * Cc * H, W, torch.float32)
    L.call("vk_nhwc_to_nchw", G.P(xd), N, Cc, H, W, G.P(buf), dt, G.stream())
    want = xd.cpu().float().permute(0, 3, 1, 2).contiguous()
    PU.assert_same_bits(result(buf, (N, Cc, H, W)).numpy(), want.numpy())


CONVERTERS = pytest.mark.parametrize("convert", [nchw_to_nhwc, nhwc_to_nchw], ids=lambda f: f.__name__)


@DTYPES
@CONVERTERS
@pytest.mark.parametrize("shape", PU.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_each_direction(shape, convert, dt):
    """Each converter alone against torch's permute; an element holds its own linear index, so any misplacement shows."""
    convert(PU.index_tensor(shape), dt)


@DTYPES
@CONVERTERS
def test_layout_special_values(convert, dt):
    """+-inf, NaN, -0.0, an f16 subnormal and +-70000 (inf in f16) keep their place, sign and class."""
    convert(PU.specials_tensor(), dt)


@DTYPES
@CONVERTERS
def test_layout_past_the_grid_cap(convert, dt):
    """1 054 152 elements: more than 4096 workgroups x 256 lanes, so the grid-stride loop takes a second step."""
    assert int(np.prod(PU.LAYOUT_OVER_CAP)) > 4096 * 256
    convert(PU.index_tensor(PU.LAYOUT_OVER_CAP), dt)


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
def maxpool(x, caffe, dt):
    """x [N,C,H,W] fp32 of values the type holds exactly -> the kernel's result against maxpool_ref, bitwise."""
    N, Cc, H, W = x.shape
    ref = PU.maxpool_ref(x, caffe)
    Ho, Wo = ref.shape[2:]
    xd = nhwc(x, dt)
    buf = guarded(N * Ho * Wo, Cc, G.TDT[dt])
    L.call("vk_maxpool3x3s2", G.P(xd), N, H, W, Cc, caffe, G.P(buf), dt, G.stream())
    PU.assert_same_bits(nchw32(result(buf, (N, Ho, Wo, Cc))), ref.numpy())


def negative_map(shape, dt, seed):
    x = torch.from_numpy(PU.rng(seed).standard_normal(shape).astype(np.float32)) - 10.0
    if dt == L.VK_F16:
        x = x.half().float()
    assert bool((x < 0).all())
    return x


@pytest.mark.parametrize("caffe", [1, 0], ids=["caffe", "pad1"])
@pytest.mark.parametrize("dt,Cc", [pytest.param(dt, c, id=f"{NAME[dt]}-C{c}")
                                   for dt, cs in ((L.VK_F16, (8, 24, 64)), (L.VK_F32, (4, 12, 64))) for c in cs])
def test_maxpool_minimum_sizes_all_negative(dt, Cc, caffe):
    """H, W in 3 .. 6 in all 16 pairings, three images, one / three / many 16-byte chunks per pixel, every value negative: a 0
    in place of -inf as the initial value or as the pad = 1 border would win.  (NaN is not fed in: both pool kernels drop NaN
    by design -- fmaxf and `>` keep the other operand -- and the stem raises its non-finite flag at the source instead, see
    the comment in stem_pack_kernel.)"""
    for H in (3, 4, 5, 6):
        for W in (3, 4, 5, 6):
            maxpool(negative_map((3, Cc, H, W), dt, 100 * H + W), caffe, dt)


@DTYPES
@pytest.mark.parametrize("caffe", [1, 0], ids=["caffe", "pad1"])
def test_maxpool_infinite_windows(caffe, dt):
    """A window of nothing but -inf gives -inf (both modes' first window lies inside rows and columns 0 .. 2); +inf wins."""
    Cc = 16
    x = negative_map((2, Cc, 7, 9), dt, 5)
    x[:, :, 0:3, 0:3] = float("-inf")
    x[0, 3, 5, 6] = x[1, 9, 6, 8] = float("inf")
    ref = PU.maxpool_ref(x, caffe)
    assert bool((ref[:, :, 0, 0] == float("-inf")).all()) and int((ref == float("inf")).sum()) >= 2
    maxpool(x, caffe, dt)


def test_maxpool_past_the_grid_cap():
    """fp32, 64 channels, 515 x 515, pad 1: 258 x 258 x 16 work items, more than 4096 workgroups x 256."""
    assert 258 * 258 * 16 > 4096 * 256
    maxpool(negative_map((1, 64, 515, 515), L.VK_F32, 9), 0, L.VK_F32)


# ---- RoIPool -----------------------------------------------------------------------------------------------------------------------
def roi_channels(dt):
    return 320 if dt == L.VK_F16 else 160            # 40 chunks: P * 40 = 280 > 256 lanes at P = 7


@functools.lru_cache(maxsize=None)
def roi_map():
    return PU.roi_feature_map()


@functools.lru_cache(maxsize=None)
def roi_map_dev(dt):
    return nhwc(roi_map()[:, :roi_channels(dt)], dt)


@functools.lru_cache(maxsize=2)
def sweep_reference(P, scale):
    return PU.roi_pool_ref(roi_map(), PU.sweep_rois(scale), P, scale).numpy()


@functools.lru_cache(maxsize=None)
def hand_reference(P, scale):
    return PU.hand_expected(roi_map().numpy(), PU.hand_rois(scale), P, scale)


def roi_pool(xd, rois, P, scale, dt):
    """xd [N,H,W,C] on the device, rois [K,5] numpy -> [K,C,P,P] fp32 numpy."""
    N, H, W, Cc = xd.shape
    K = len(rois)
    rd = torch.from_numpy(np.ascontiguousarray(rois, dtype=np.float32)).to(G.DEV) if K else torch.zeros(5, device=G.DEV)
    buf = guarded(K * P * P, Cc, G.TDT[dt])
    L.call("vk_roi_pool", G.P(xd), N, H, W, Cc, G.P(rd), K, scale, P, G.P(buf), dt, G.stream())
    return nchw32(result(buf, (K, P, P, Cc)))


ROI_GRID = [pytest.mark.parametrize("scale", PU.ROI_SCALES, ids=["s16", "s32", "s1"]), pytest.mark.parametrize("P", PU.ROI_P)]


def roi_grid(f):
    for m in ROI_GRID:
        f = m(f)
    return DTYPES(f)


@roi_grid
def test_roi_pool_geometry_sweep(P, scale, dt):
    """Every integer cell range from two cells outside the map to two cells outside on the other side, as rows and as
    columns, at four output sizes and three scales, three images: 210 RoIs against the oracle.  40 chunks per pixel, so the
    lanes' loop over (pw, chunk) runs a second pass from P = 7 on."""
    assert 7 * roi_channels(dt) // (8 if dt == L.VK_F16 else 4) > 256
    got = roi_pool(roi_map_dev(dt), PU.sweep_rois(scale), P, scale, dt)
    PU.assert_same_bits(got, np.ascontiguousarray(sweep_reference(P, scale)[:, :roi_channels(dt)]))


@roi_grid
def test_roi_pool_hand_built(P, scale, dt):
    """Corners at -0.5, 0.5 and 2.5 cells (roundf goes away from zero: -1, 1, 3), x2 < x1, y2 < y1, a RoI wholly outside on
    each side (every bin empty: 0), one cell, the whole map: against the rule restated by hand, not the oracle's C."""
    got = roi_pool(roi_map_dev(dt), PU.hand_rois(scale), P, scale, dt)
    PU.assert_same_bits(got, np.ascontiguousarray(hand_reference(P, scale)[:, :roi_channels(dt)]))
    outside = [i for i, r in enumerate(PU.HAND_ROIS_CELLS) if r[3] < 0 or r[1] > 16 or r[4] < 0 or r[2] > 16]
    assert len(outside) == 4 and not got[outside].any()


@DTYPES
@pytest.mark.parametrize("P", [1, 2, 4])
def test_roi_pool_non_finite_features(P, dt):
    """The rules of the kernel's comment.  A 4 x 4 map of two 16-byte chunks; channel 1 (in chunk 0) holds, by quadrant: a NaN
    among finite values, nothing but -inf, nothing but NaN, a +inf.  A NaN never wins; a bin of nothing but NaN, or but -inf,
    keeps the initial value, -FLT_MAX in fp32 and -inf in f16 (what -FLT_MAX rounds to); +inf wins; every other channel, the
    second chunk included, is finite and exact."""
    vn = 8 if dt == L.VK_F16 else 4
    x = torch.from_numpy(PU.rng(41).standard_normal((1, 2 * vn, 4, 4)).astype(np.float32)).half().float()
    x[0, 1, 0, 0] = NAN
    x[0, 1, 0:2, 2:4] = float("-inf")
    x[0, 1, 2:4, 0:2] = NAN
    x[0, 1, 3, 3] = float("inf")
    roi = np.asarray([[0, 0, 0, 3, 3]], dtype=np.float32)
    want = PU.roi_pool_by_hand(x.numpy(), roi[0], P, 1.0)[None]
    low = -PU.FLT_MAX
    if dt == L.VK_F16:
        want = torch.from_numpy(want).half().float().numpy()
        low = -np.inf
    quad = {1: [[np.inf]], 2: [[x[0, 1, 0:2, 0:2].nan_to_num(-99.0).max().item(), low], [low, np.inf]]}
    if P in quad:
        np.testing.assert_array_equal(want[0, 1], np.asarray(quad[P], dtype=np.float32))
    else:
        assert want[0, 1, 0, 0] == low and want[0, 1, 3, 3] == np.inf and (want[0, 1, 0:2, 2:4] == low).all()
    got = roi_pool(nhwc(x, dt), roi, P, 1.0, dt)
    PU.assert_same_bits(got, want)
    others = np.delete(got, 1, axis=1)
    assert np.isfinite(others).all() and not np.isnan(got).any()


@DTYPES
def test_roi_pool_no_rois(dt):
    """K = 0 returns VK_OK and writes nothing."""
    assert roi_pool(roi_map_dev(dt), np.zeros((0, 5), np.float32), 7, 1.0 / 16, dt).shape == (0, roi_channels(dt), 7, 7)


# ---- mean-pool ---------------------------------------------------------------------------------------------------------------------
def mean_pool(x, dt):
    K, S, Cc = x.shape
    xd = x.to(G.TDT[dt]).to(G.DEV)
    buf = guarded(K, Cc, torch.float32)
    L.call("vk_mean_pool", G.P(xd), K, S, Cc, G.P(buf), dt, G.stream())
    return result(buf, (K, Cc)).numpy()


@pytest.mark.parametrize("dt,Cc", [pytest.param(dt, c, id=f"{NAME[dt]}-C{c}") for dt in (L.VK_F32, L.VK_F16) for c in PU.MEAN_C[NAME[dt]]])
def test_mean_pool_exact_on_integers(dt, Cc):
    """Integers in [-8, 8]: every partial sum is exact in any order and the one division is correctly rounded, so the result is
    the fp64 mean rounded to fp32, bit for bit (see mean_pool_ref).  S = 1, 2, 3 leave row groups idle; the widths are 1, 63, 64,
    65 and 256 chunks: below, at and one lane into a second 64-lane pass."""
    for K in PU.MEAN_K:
        for S in PU.MEAN_S:
            x = PU.integer_features(K, S, Cc)
            PU.assert_same_bits(mean_pool(x, dt), PU.mean_pool_ref(x).numpy())


@DTYPES
def test_mean_pool_non_finite_stays_in_its_column(dt):
    """A NaN and a +inf planted at known (k, s, c) reach exactly their own (k, c): the NaN sits in the first 64-lane pass where
    the second pass has a lane of the same number, the +inf in that second pass and in row group 0's second row; nothing
    leaks through the LDS partials into another pass, row group or RoI."""
    vn = 8 if dt == L.VK_F16 else 4
    K, S, Cc = 3, 5, 65 * vn
    x = PU.integer_features(K, S, Cc, seed=1)
    planted = {(1, 2, 1): NAN, (2, 4, 64 * vn + 1): float("inf"), (0, 3, 63 * vn): NAN}
    for (k, s, c), v in planted.items():
        x[k, s, c] = v
    got = mean_pool(x, dt)
    PU.assert_same_bits(got, PU.mean_pool_ref(x).numpy())
    assert sorted(zip(*np.nonzero(~np.isfinite(got)))) == sorted((k, c) for k, _, c in planted)
    assert np.isnan(got[1, 1]) and np.isnan(got[0, 63 * vn]) and got[2, 64 * vn + 1] == np.inf


# ---- box decode --------------------------------------------------------------------------------------------------------------------
WEIGHTS = pytest.mark.parametrize("w", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)], ids=["rpn", "roi"])


def box_decode(d, b, w):
    M, k4 = d.shape
    dd = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(G.DEV) if M else torch.zeros(4, device=G.DEV)
    bd = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(G.DEV) if M else torch.zeros(4, device=G.DEV)
    buf = guarded(M, k4, torch.float32)
    L.call("vk_box_decode", G.P(dd), G.P(bd), M, k4 // 4, (C.c_float * 4)(*w), G.P(buf), G.stream())
    return result(buf, (M, k4)).numpy()


@WEIGHTS
@pytest.mark.parametrize("M,k", [(1, 1), (3, 5), (257, 1), (5, 1601)])
def test_box_decode_translation_is_exact(M, k, w):
    """dw = dh = 0: exp(0) = 1, and everything else is one IEEE operation after another in the reference's order (no FMA),
    so the bits are the fp32 reference's.  k = 1601 carries the anchor index m = i / k across many workgroups."""
    d, b = PU.decode_deltas(M, k, w, True, seed=M + k), PU.decode_boxes(M, seed=M)
    PU.assert_same_bits(box_decode(d, b, w), PU.box_decode_ref32(d, b, w).numpy())


@WEIGHTS
def test_box_decode_general_within_bound(w):
    """General deltas: each element within the bound derived from the kernel's rounding points and the device expf's 1 ulp
    (pool_util).  The worst |err| / bound is printed; it is a report, the assertion is <= 1."""
    d, b = PU.decode_deltas(64, 5, w, False), PU.decode_boxes(64)
    ref, bound = PU.box_decode_ref64(d, b, w)
    r = PU.worst_ratio(box_decode(d, b, w), ref, bound)
    print(f"box_decode general {w}: worst |err| / bound = {r:.3f}")
    assert r <= 1.0


@WEIGHTS
@pytest.mark.parametrize("j", [2, 3], ids=["dw", "dh"])
def test_box_decode_scale_clamp(j, w):
    """d / weight just below, at and just above (float)log(1000 / 16), +inf and -inf, on one anchor: everything at or above the
    clamp gives the bits of the value at the clamp, those lie within the general bound, the value below gives a smaller box;
    -inf gives size exactly 0 with both corners on the predicted centre."""
    targets = PU.clamp_neighbours() + [np.float32(-np.inf)]
    d = np.tile(PU.decode_deltas(1, 1, w, False, seed=3), (len(targets), 1))
    d[:, j] = [PU.delta_for(t, w[j]) for t in targets]
    b = np.tile(np.asarray([[10.5, 20.25, 110.5, 84.25]], dtype=np.float32), (len(targets), 1))
    got = box_decode(d, b, w)
    below, at, above, inf, ninf = got
    PU.assert_same_bits(above, at)
    PU.assert_same_bits(inf, at)
    ref, bound = PU.box_decode_ref64(d[:3], b[:3], w)
    r = PU.worst_ratio(got[:3], ref, bound)
    print(f"box_decode clamp {w}: worst |err| / bound = {r:.3f}")
    assert r <= 1.0
    lo, hi = j - 2, j
    assert below[hi] - below[lo] < at[hi] - at[lo]
    assert np.isfinite(got).all()
    centre = PU.box_decode_ref32(d[4:], b[4:], w).numpy()[0]          # exp(-inf) = 0: pcx -+ 0, no exponential's ulp in it
    PU.assert_same_bits(ninf[[lo, hi]], centre[[lo, hi]])
    assert centre[lo] == centre[hi]


@WEIGHTS
@pytest.mark.parametrize("j", [0, 1, 2, 3], ids=["dx", "dy", "dw", "dh"])
def test_box_decode_nan_delta_stays_in_its_box(j, w):
    """A NaN in one delta of one box makes that box's two coordinates of the same axis NaN, as the fp32 reference says, and
    leaves every other box exact."""
    M, k = 3, 5
    d, b = PU.decode_deltas(M, k, w, True, seed=j), PU.decode_boxes(M, seed=2)
    d[1, 4 * 2 + j] = NAN
    want = PU.box_decode_ref32(d, b, w).numpy()
    assert sorted(np.nonzero(np.isnan(want[1]))[0] - 8) == [j % 2, j % 2 + 2] and not np.isnan(want[[0, 2]]).any()
    PU.assert_same_bits(box_decode(d, b, w), want)


@WEIGHTS
def test_box_decode_degenerate_anchors(w):
    """Anchors of zero and of negative width or height, translation only: bit-exact."""
    b = np.asarray([[5.5, 7.25, 5.5, 40.0], [5.5, 7.25, 60.0, 7.25], [3.0, 3.0, 3.0, 3.0], [50.0, 10.0, 20.5, 90.0],
                    [10.0, 90.0, 70.0, 15.5], [80.0, 80.0, -20.0, -30.0]], dtype=np.float32)
    d = PU.decode_deltas(len(b), 3, w, True, seed=5)
    PU.assert_same_bits(box_decode(d, b, w), PU.box_decode_ref32(d, b, w).numpy())


def test_box_decode_no_boxes():
    """M = 0 returns VK_OK with nothing written."""
    assert box_decode(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32), (1.0, 1.0, 1.0, 1.0)).shape == (0, 8)
