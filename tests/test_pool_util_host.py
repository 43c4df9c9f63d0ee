"""CPU (-m "not gpu"): the references of tests/pool_util.py held against each other, so that tests/test_gpu_pool_kernels.py
does not rest on one of them alone, and the argument checks of the pooling entry points that run before any HIP call."""
import os

import numpy as np
import pytest
import torch

from oracle.frcnn_oracle import FRCNNOracle
from vltk_amd import _lib as L

import pool_util as PU

FAKE = 0x1000            # never dereferenced: every check below runs before the device


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "kat_ops.npz"))


# ---- RoIPool: the two references agree on every hand-built RoI ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def roi_map():
    return PU.roi_feature_map()[:, :16].contiguous()         # the GPU file's map; 16 channels are enough on the host


@pytest.mark.parametrize("scale", PU.ROI_SCALES, ids=["s16", "s32", "s1"])
@pytest.mark.parametrize("P", PU.ROI_P)
def test_roi_pool_by_hand_is_the_oracle(roi_map, P, scale):
    rois = PU.hand_rois(scale)
    np.testing.assert_array_equal(PU.hand_expected(roi_map.numpy(), rois, P, scale), PU.roi_pool_ref(roi_map, rois, P, scale).numpy())


def test_roi_pool_by_hand_rounds_half_away_from_zero():
    assert [PU._roundf(v) for v in (-0.5, 0.5, 2.5, -2.5, 1.5, 0.49999997, -0.49999997, 3.0)] == [-1, 1, 3, -3, 2, 0, 0, 3]
    x = np.arange(16 * 16, dtype=np.float32).reshape(1, 1, 16, 16)
    # -0.5 .. 2.5 cells -> cells -1 .. 3: five wide, P = 1 -> the maximum over rows and columns 0 .. 3
    assert PU.roi_pool_by_hand(x, (0, -8.0, -8.0, 40.0, 40.0), 1, 1.0 / 16)[0, 0, 0] == 3 * 16 + 3


def test_roi_pool_by_hand_non_finite_rules():
    x = np.zeros((1, 1, 4, 4), dtype=np.float32)
    x[0, 0, 0, 0], x[0, 0, 0, 1] = np.nan, -3.0                # a NaN never wins
    x[0, 0, 2:, :2] = np.nan                                    # a bin of nothing but NaN
    x[0, 0, :2, 2:] = -np.inf                                   # ... but -inf
    x[0, 0, 3, 3] = np.inf
    got = PU.roi_pool_by_hand(x, (0, 0.0, 0.0, 3.0, 3.0), 2, 1.0)[0]
    np.testing.assert_array_equal(got, np.asarray([[0.0, -PU.FLT_MAX], [-PU.FLT_MAX, np.inf]], dtype=np.float32))


def test_sweep_rois_cover_every_range():
    for scale in PU.ROI_SCALES:
        r = PU.sweep_rois(scale)
        cells = np.float32(scale) * r[:, 1:]
        assert r.shape == (210, 5) and np.array_equal(cells, np.round(cells))
        assert {(int(a), int(b)) for a, b in cells[:, [1, 3]]} == set(PU.cell_ranges())
        assert {(int(a), int(b)) for a, b in cells[:, [0, 2]]} == set(PU.cell_ranges())
        assert sorted(set(r[:, 0].tolist())) == [0.0, 1.0, 2.0]


# ---- box decode ----------------------------------------------------------------------------------------------------------------------
GOLDEN_DECODES = [("deltas_rpn", (1.0, 1.0, 1.0, 1.0)), ("deltas_roi", (10.0, 10.0, 5.0, 5.0))]


@pytest.mark.parametrize("tag,w", GOLDEN_DECODES)
def test_box_decode_ref32_is_the_oracle(kat, tag, w):
    d, b = torch.from_numpy(kat[tag + "/deltas"]), torch.from_numpy(kat[tag + "/boxes"])
    got = PU.box_decode_ref32(d, b, w)
    PU.assert_same_bits(got.numpy(), FRCNNOracle.apply_deltas(d, b, w).numpy())
    PU.assert_same_bits(got.numpy(), kat[tag + "/y"])          # and the reference's own recorded output


def _decode_cases():
    yield from ((tag, w, None) for tag, w in GOLDEN_DECODES)
    for w in ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)):
        yield "general", w, (PU.decode_deltas(64, 5, w, False), PU.decode_boxes(64))
        d = PU.decode_deltas(4, 1, w, False)
        d[:, 2] = [PU.delta_for(t, w[2]) for t in PU.clamp_neighbours()]
        yield "clamp", w, (d[:3], PU.decode_boxes(3))        # the +inf row has no finite bound


@pytest.mark.parametrize("tag,w,data", list(_decode_cases()), ids=lambda v: v if isinstance(v, str) else None)
def test_box_decode_bound_holds_for_a_correct_fp32_evaluation(kat, tag, w, data):
    """torch's CPU exp is good to 1 ulp as well, so a correct fp32 evaluation fits the bound (that the bound is not slack
    enough to pass wrong arithmetic is the next test's)."""
    d, b = data if data is not None else (kat[tag + "/deltas"], kat[tag + "/boxes"])
    ref, bound = PU.box_decode_ref64(d, b, w)
    assert np.isfinite(bound).all() and (bound > 0).all()
    r = PU.worst_ratio(PU.box_decode_ref32(d, b, w).numpy(), ref, bound)
    print(f"box_decode {tag} {w}: fp32 on the CPU, worst |err| / bound = {r:.3f}")
    assert r <= 1.0


def test_box_decode_bound_refuses_wrong_arithmetic():
    """An exponential two parts in a million off (17 ulp) does not fit; nor does a decode with the other head's weights."""
    w = (10.0, 10.0, 5.0, 5.0)
    d, b = PU.decode_deltas(64, 5, w, False), PU.decode_boxes(64)
    ref, bound = PU.box_decode_ref64(d, b, w)
    assert PU.worst_ratio(PU.box_decode_ref32(d, b, w, exp=lambda t: torch.exp(t) * (1 + 2e-6)).numpy(), ref, bound) > 1.0
    assert PU.worst_ratio(PU.box_decode_ref32(d, b, (1.0, 1.0, 1.0, 1.0)).numpy(), ref, bound) > 1.0


def test_clamp_deltas_land_on_the_neighbours():
    below, at, above, inf = PU.clamp_neighbours()
    assert below < at < above < inf and at == np.float32(np.log(1000.0 / 16.0))
    for w in (1.0, 5.0):
        for t in (below, at, above, inf):
            assert np.float32(PU.delta_for(t, w) / np.float32(w)) == t


# ---- mean-pool: the fp64 reference gives the fp32 bits on integers ------------------------------------------------------------------
@pytest.mark.parametrize("S", PU.MEAN_S)
def test_mean_pool_ref_is_the_fp32_mean_on_integers(S):
    for K in PU.MEAN_K:
        for C in sorted(set(PU.MEAN_C["fp16"] + PU.MEAN_C["fp32"])):
            x = PU.integer_features(K, S, C)
            assert float(x.abs().max()) <= 8 and torch.equal(x, x.half().float())
            ref = PU.mean_pool_ref(x)
            PU.assert_same_bits(ref.numpy(), x.mean(1).numpy())
            # the kernel's own order: four interleaved row groups, joined in a fixed order, one division
            part = [x[:, g::4].sum(1) if g < S else torch.zeros(K, C) for g in range(4)]
            PU.assert_same_bits(ref.numpy(), ((((part[0] + part[1]) + part[2]) + part[3]) / np.float32(S)).numpy())


# ---- max-pool reference ----------------------------------------------------------------------------------------------------------------
def test_maxpool_ref_modes():
    x = torch.arange(25, dtype=torch.float32).reshape(1, 1, 5, 5) - 30.0
    assert PU.maxpool_ref(x, 1).shape == (1, 1, 2, 2) and PU.maxpool_ref(x, 0).shape == (1, 1, 3, 3)
    assert PU.maxpool_ref(x, 0)[0, 0, 0, 0] == x[0, 0, 1, 1]                     # the pad-1 border counts as -inf, not 0
    x4 = torch.full((1, 1, 4, 4), -5.0)
    assert PU.maxpool_ref(x4, 1).shape == (1, 1, 2, 2) and bool((PU.maxpool_ref(x4, 1) == -5.0).all())


# ---- the refusals that need no device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C", [(L.VK_F16, 12), (L.VK_F16, 4), (L.VK_F32, 6), (L.VK_F32, 2)])
def test_channel_count_must_fill_16_byte_vectors(lib, dt, C):
    vn = 8 if dt == L.VK_F16 else 4
    with pytest.raises(ValueError, match=f"maxpool: C={C} must be a multiple of {vn}"):
        L.call("vk_maxpool3x3s2", FAKE, 1, 8, 8, C, 0, FAKE, dt, None)
    with pytest.raises(ValueError, match=f"roi_pool: C={C} must be a multiple of {vn}"):
        L.call("vk_roi_pool", FAKE, 1, 8, 8, C, FAKE, 1, 1.0 / 16, 7, FAKE, dt, None)
    with pytest.raises(ValueError, match=f"mean_pool: C={C} must be a multiple of {vn}"):
        L.call("vk_mean_pool", FAKE, 1, 4, C, FAKE, dt, None)


@pytest.mark.parametrize("hw", [(2, 8), (8, 2), (0, 0)])
def test_maxpool_refuses_a_map_below_one_window(lib, hw):
    with pytest.raises(ValueError, match=f"maxpool: input {hw[0]}x{hw[1]} too small"):
        L.call("vk_maxpool3x3s2", FAKE, 1, hw[0], hw[1], 8, 1, FAKE, L.VK_F16, None)


@pytest.mark.parametrize("shape", [(0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)])
def test_layout_converters_refuse_an_empty_tensor(lib, shape):
    with pytest.raises(ValueError, match="nchw_to_nhwc: empty tensor"):
        L.call("vk_nchw_to_nhwc", FAKE, *shape, FAKE, L.VK_F16, None)
    with pytest.raises(ValueError, match="nhwc_to_nchw: empty tensor"):
        L.call("vk_nhwc_to_nchw", FAKE, *shape, FAKE, L.VK_F32, None)


def test_mean_pool_refuses_no_positions(lib):
    for dt in (L.VK_F16, L.VK_F32):
        with pytest.raises(ValueError, match="mean_pool"):
            L.call("vk_mean_pool", FAKE, 1, 0, 8, FAKE, dt, None)
        with pytest.raises(ValueError, match="mean_pool"):
            L.call("vk_mean_pool", FAKE, 0, 0, 8, FAKE, dt, None)       # the S check comes before K == 0 returns


def test_pool_entry_points_refuse_other_types(lib):
    for name, args in (("vk_maxpool3x3s2", (FAKE, 1, 8, 8, 8, 0, FAKE)), ("vk_mean_pool", (FAKE, 1, 4, 8, FAKE))):
        with pytest.raises(ValueError, match="bad dtype"):
            L.call(name, *args, L.VK_BF16, None)
    with pytest.raises(ValueError, match="bad dtype"):
        L.call("vk_roi_pool", FAKE, 1, 8, 8, 8, FAKE, 1, 1.0 / 16, 7, FAKE, L.VK_I32, None)
    with pytest.raises(ValueError, match="roi_pool"):
        L.call("vk_roi_pool", FAKE, 1, 8, 8, 8, FAKE, 1, 1.0 / 16, 0, FAKE, L.VK_F16, None)      # P = 0
    with pytest.raises(ValueError, match="box_decode: bad sizes"):
        L.call("vk_box_decode", FAKE, FAKE, -1, 1, None, FAKE, None)
    with pytest.raises(ValueError, match="box_decode: bad sizes"):
        L.call("vk_box_decode", FAKE, FAKE, 1, 0, None, FAKE, None)
