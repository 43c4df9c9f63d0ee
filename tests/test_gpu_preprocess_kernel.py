"""-m gpu: vk_preprocess (csrc/preprocess.hip) called directly, at sizes the test chooses -- identity and dyadic ratios bit
for bit, general ratios per element under the bound derived in preprocess_util, batches that cross the 32-image chunk of the
launch loop, and refusals that must leave the output untouched.  mean and std are three distinct numbers each and std is no
power of two, the padding value is not the config's, Hmax and Wmax exceed every image, and the output carries one more image
slot of sentinels.  tests/test_preprocess_kernel_host.py proves the references on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                          # noqa: E402

import preprocess_util as PU                            # noqa: E402

MEAN32, STD32 = np.asarray(PU.MEAN, np.float32), np.asarray(PU.STD, np.float32)


def split(out, new_hw):
    """The buffer of run_preprocess -> per image (interior [3, h, w], its padding as a flat array); the sentinel slot is checked."""
    assert (out[-1] == PU.SENTINEL).all(), "the slot behind the last image was written"
    parts = []
    for i, (h, w) in enumerate(new_hw):
        mask = np.zeros(out.shape[2:], bool)
        mask[:h, :w] = True
        parts.append((out[i][:, :h, :w], out[i][:, ~mask]))
    return parts


def assert_padding(pad, value=PU.PAD):
    assert pad.size > 0 and (pad.view(np.uint32) == np.float32(value).view(np.uint32)).all()


@pytest.mark.parametrize("hw", PU.IDENTITY)
def test_identity_is_bit_exact(hw):
    """new == raw: the weights are exactly 0 and 1 under the kernel's operation order, so out = fp32 (raw - mean) / std."""
    raw = PU.raw_image(*hw, seed=10)
    _, out = PU.run_preprocess([raw], [hw], hw[0] + 3, hw[1] + 2)
    (inner, pad), = split(out, [hw])
    np.testing.assert_array_equal(inner, ((raw - MEAN32) / STD32).transpose(2, 0, 1))
    assert_padding(pad)


@pytest.mark.parametrize("raw_hw,new_hw", PU.DYADIC)
def test_dyadic_ratios_are_bit_exact(raw_hw, new_hw):
    """Integer pixels, weights in {0, 1/4, 1/2, 3/4, 1}: the interpolated value is exact, then one fp32 subtract and divide."""
    raw = PU.raw_image(*raw_hw, seed=11, integers=True)
    v, _ = PU.contract_reference(raw, *new_hw, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    _, out = PU.run_preprocess([raw], [new_hw], new_hw[0] + 1, new_hw[1] + 5)
    (inner, pad), = split(out, [new_hw])
    np.testing.assert_array_equal(inner, (v32 - MEAN32[:, None, None]) / STD32[:, None, None])
    assert_padding(pad)
    mean, std = (100.5, 116.25, 122.0), (1.0, 2.0, 0.5)                  # dyadic: the whole result is exact
    ref, _ = PU.contract_reference(raw, *new_hw, mean, std)
    _, out = PU.run_preprocess([raw], [new_hw], new_hw[0] + 1, new_hw[1] + 5, mean=mean, std=std)
    (inner, pad), = split(out, [new_hw])
    np.testing.assert_array_equal(inner.astype(np.float64), ref)
    assert_padding(pad)


@pytest.mark.parametrize("raw_hw,new_hw", PU.GENERAL)
def test_general_ratios_per_element(raw_hw, new_hw):
    raw = PU.raw_image(*raw_hw, seed=12)
    ref, bound = PU.contract_reference(raw, *new_hw, PU.MEAN, PU.STD)
    _, out = PU.run_preprocess([raw], [new_hw], new_hw[0] + 2, new_hw[1] + 3)
    (inner, pad), = split(out, [new_hw])
    worst = PU.worst_ratio(inner, ref, bound)
    print(f"\n[vk_preprocess {raw_hw[0]}x{raw_hw[1]} -> {new_hw[0]}x{new_hw[1]}] worst |out - ref| / bound {worst:.3f}")
    assert worst <= 1
    assert_padding(pad)


@pytest.mark.parametrize("N", [33, 65])
def test_batches_across_the_32_image_chunk(N):
    """A second and a third launch of the chunk loop: image i in slot i, each image checked alone."""
    raw_hw, new_hw = PU.batch_geometry(N)
    raws = [PU.raw_image(h, w, seed=100 + i) for i, (h, w) in enumerate(raw_hw)]
    _, out = PU.run_preprocess(raws, new_hw, 10, 12)
    worst = 0.0
    for i, (inner, pad) in enumerate(split(out, new_hw)):
        ref, bound = PU.contract_reference(raws[i], *new_hw[i], PU.MEAN, PU.STD)
        r = PU.worst_ratio(inner, ref, bound)
        assert r <= 1, f"image {i}: worst |out - ref| / bound {r:.3f}"
        worst = max(worst, r)
        assert_padding(pad)
    print(f"\n[vk_preprocess batch of {N}] worst |out - ref| / bound {worst:.3f}")


@pytest.mark.parametrize("what", ["new_h > Hmax at image 40", "null image at index 33"])
def test_refusals_leave_the_output_untouched(what):
    """Every image is validated before the first launch: a bad image behind the first chunk of 32 writes nothing."""
    raw_hw, new_hw = PU.batch_geometry(48)
    raws = [PU.raw_image(h, w, seed=200 + i) for i, (h, w) in enumerate(raw_hw)]
    null_at = None
    if what.startswith("new_h"):
        new_hw[40] = (11, new_hw[40][1])
    else:
        null_at = 33
    _, out = PU.run_preprocess(raws, new_hw, 10, 12, null_at=null_at, expect=L.VK_EINVAL)
    assert (out == PU.SENTINEL).all()
