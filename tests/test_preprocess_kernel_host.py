"""CPU: what tests/test_gpu_preprocess_kernel.py relies on -- the restated contract of csrc/preprocess.hip agrees with
torch's bilinear resize, an fp32 emulation of the contract stays inside the derived bound at every general ratio, the identity
and dyadic cases are exact, and wrong arithmetic (another channel's std, a multiply for the divide) leaves the bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import preprocess_util as PU

MEAN32, STD32 = np.asarray(PU.MEAN, np.float32), np.asarray(PU.STD, np.float32)


@pytest.mark.parametrize("raw_hw,new_hw", PU.GENERAL + PU.DYADIC)
def test_restatement_agrees_with_torch_interpolate(raw_hw, new_hw):
    raw = PU.raw_image(*raw_hw, seed=1)
    ref, _ = PU.contract_reference(raw, *new_hw, PU.MEAN, PU.STD)
    t = F.interpolate(torch.from_numpy(raw).permute(2, 0, 1)[None], new_hw, mode="bilinear", align_corners=False)[0]
    t = (t.double() - torch.tensor(MEAN32).double().view(3, 1, 1)) / torch.tensor(STD32).double().view(3, 1, 1)
    assert np.abs(ref - t.numpy()).max() / np.abs(ref).max() <= 2e-6


@pytest.mark.parametrize("raw_hw,new_hw", PU.GENERAL)
def test_fp32_emulation_stays_inside_the_bound(raw_hw, new_hw):
    raw = PU.raw_image(*raw_hw, seed=2)
    ref, bound = PU.contract_reference(raw, *new_hw, PU.MEAN, PU.STD)
    worst = PU.worst_ratio(PU.contract_fp32(raw, *new_hw, PU.MEAN, PU.STD), ref, bound)
    print(f"\n[fp32 emulation {raw_hw} -> {new_hw}] worst |out - ref| / bound {worst:.3f}")
    assert worst <= 1


def test_wrong_arithmetic_leaves_the_bound():
    raw = PU.raw_image(5, 7, seed=3)
    ref, bound = PU.contract_reference(raw, 8, 11, PU.MEAN, PU.STD)
    wrong_std = PU.contract_fp32(raw, 8, 11, PU.MEAN, (PU.STD[0],) * 3)
    assert PU.worst_ratio(wrong_std[0], ref[0], bound[0]) <= 1 < min(PU.worst_ratio(wrong_std[c], ref[c], bound[c]) for c in (1, 2))
    times = PU.contract_fp32(raw, 8, 11, PU.MEAN, tuple(1 / s for s in PU.STD))       # v * std in place of v / std
    assert PU.worst_ratio(times, ref, bound) > 1
    assert PU.worst_ratio(ref * (1 + 2.0 ** -20), ref, bound) > 1                        # 16 u relative is outside c = 6


@pytest.mark.parametrize("hw", PU.IDENTITY)
def test_identity_is_the_fp32_normalisation(hw):
    """new == raw: the weights are exactly 0 and 1, so the contract gives fp32 (raw - mean) / std."""
    raw = PU.raw_image(*hw, seed=4)
    np.testing.assert_array_equal(PU.contract_fp32(raw, *hw, PU.MEAN, PU.STD), ((raw - MEAN32) / STD32).transpose(2, 0, 1))
    for lo, hi, l0, l1 in (PU.axis_taps(hw[0], hw[0]), PU.axis_taps(hw[1], hw[1])):
        assert lo.tolist() == list(range(len(lo))) and (l0 == 1).all() and (l1 == 0).all()


@pytest.mark.parametrize("raw_hw,new_hw", PU.DYADIC)
def test_dyadic_ratios_are_exact(raw_hw, new_hw):
    """Integer pixels and weights in {0, 1/4, 1/2, 3/4, 1}: the interpolated value is an fp32 number whatever the order."""
    raw = PU.raw_image(*raw_hw, seed=5, integers=True)
    for size, new in zip(raw_hw, new_hw):
        _, _, l0, l1 = PU.axis_taps(size, new)
        assert set(np.concatenate([l0, l1]).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    ref, _ = PU.contract_reference(raw, *new_hw, zero, one)
    np.testing.assert_array_equal(PU.contract_fp32(raw, *new_hw, zero, one).astype(np.float64), ref)
    assert len(np.unique(ref % 1)) >= 4                           # quarters occur: the weights are not all 0 or 1
    mean, std = (100.5, 116.25, 122.0), (1.0, 2.0, 0.5)
    ref, _ = PU.contract_reference(raw, *new_hw, mean, std)
    np.testing.assert_array_equal(PU.contract_fp32(raw, *new_hw, mean, std).astype(np.float64), ref)


def test_batch_geometry():
    for N in (33, 65):
        raw_hw, new_hw = PU.batch_geometry(N)
        assert all(3 <= h <= 9 and 3 <= w <= 11 for h, w in raw_hw + new_hw)
