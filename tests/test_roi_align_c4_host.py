"""CPU: the RoIAlign box pooler of the C4 model -- the config surface (vk_pooler_check through the library; no GPU is
touched) and the exact set against its fp64 restatement."""
import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import vg_c4_config
from vltk_amd.frcnn import pooler_from_config

import roi_align_c4_util as U


def _cfg(**head):
    return vg_c4_config(overrides=[("roi_box_head", k, v) for k, v in head.items()])


def test_pooler_type_values():
    assert pooler_from_config(_cfg()) == (L.VK_POOLER_ROIPOOL, 0)                       # the key is absent
    assert "pooler_type" not in vg_c4_config().ROI_BOX_HEAD.to_dict()
    assert pooler_from_config(_cfg(pooler_type="ROIPool")) == (L.VK_POOLER_ROIPOOL, 0)
    assert pooler_from_config(_cfg(pooler_type="ROIAlign", pooler_sampling_ratio=0)) == (L.VK_POOLER_ROIALIGN, 0)
    assert pooler_from_config(_cfg(pooler_type="ROIAlignV2", pooler_sampling_ratio=0)) == (L.VK_POOLER_ROIALIGNV2, 0)
    assert pooler_from_config(_cfg(pooler_type="ROIAlignV2")) == (L.VK_POOLER_ROIALIGNV2, 2)   # the build-owned config's ratio
    assert pooler_from_config(_cfg(pooler_type="ROIAlignV2", pooler_sampling_ratio=8)) == (L.VK_POOLER_ROIALIGNV2, 8)


def test_pooler_sampling_ratio_defaults_to_adaptive():
    d = vg_c4_config().to_dict()
    del d["roi_box_head"]["pooler_sampling_ratio"]
    d["roi_box_head"]["pooler_type"] = "ROIAlign"
    from vltk_amd.config import Config
    assert pooler_from_config(Config(d)) == (L.VK_POOLER_ROIALIGN, 0)


@pytest.mark.parametrize("head", [dict(pooler_type="ROIAlignV3"), dict(pooler_type="roialign"), dict(pooler_type=2),
                                  dict(pooler_type="ROIAlignV2", pooler_sampling_ratio=9),
                                  dict(pooler_type="ROIAlign", pooler_sampling_ratio=-1),
                                  dict(pooler_type="ROIAlignV2", pooler_sampling_ratio=2.0),
                                  dict(pooler_type="ROIAlignV2", pooler_sampling_ratio=True)])
def test_bad_pooler_config_is_a_value_error(head):
    with pytest.raises(ValueError):
        pooler_from_config(_cfg(**head))


def test_roipool_ignores_the_sampling_ratio():
    assert pooler_from_config(_cfg(pooler_type="ROIPool", pooler_sampling_ratio=99)) == (L.VK_POOLER_ROIPOOL, 0)


def test_vk_pooler_check():
    lib = L.load()
    for t in (L.VK_POOLER_ROIPOOL, L.VK_POOLER_ROIALIGN, L.VK_POOLER_ROIALIGNV2):
        for r in (0, 2, 8):
            assert lib.vk_pooler_check(t, r) == L.VK_OK
    for t, r in ((3, 0), (-1, 0), (L.VK_POOLER_ROIALIGNV2, 9), (L.VK_POOLER_ROIALIGN, -1)):
        assert lib.vk_pooler_check(t, r) == L.VK_EINVAL
    with pytest.raises(ValueError):
        L.call("vk_pooler_check", 7, 0)


@pytest.mark.parametrize("sr", [0, 2])
def test_align_oracle_is_exact_on_the_exact_set(sr):
    """The oracle's fp32 sums (per-sample order) equal the float64 separable restatement bit for bit: the data are exact,
    so the GPU tests may ask any summation order for the oracle's bits."""
    x, rois = U.exact_map(8), U.exact_rois()
    oracle = U.AlignOracle(_cfg(pooler_type="ROIAlignV2", pooler_sampling_ratio=sr), {})
    boxes = [torch.from_numpy(rois[rois[:, 0] == i, 1:]) for i in range(U.EXACT_MAP[0])]
    order = np.concatenate([np.nonzero(rois[:, 0] == i)[0] for i in range(U.EXACT_MAP[0])])
    got = oracle.pool(x, boxes).numpy()
    ref = U.roi_align_fp64(x.numpy(), rois[order], U.EXACT_P, U.EXACT_SCALE, sr, True)
    assert got.dtype == np.float32 and np.abs(ref).max() > 1
    np.testing.assert_array_equal(got.astype(np.float64), ref)
    # and the exact set is what it says: skipped samples, both clamps, counts that are powers of two
    assert (rois[:, 1:3] < 0).any() and (rois[:, 3] > U.EXACT_MAP[2] * 16).any() and (rois[:, 4] > U.EXACT_MAP[1] * 16).any()
    assert ((rois[:, 1:] % 4) == 0).all()


def test_align_oracle_fp16_emulation_rounds_once():
    x, rois = U.exact_map(4, seed=3) * 0.37, U.exact_rois()[:6]
    cfg = _cfg(pooler_type="ROIAlign", pooler_sampling_ratio=2)
    boxes = [torch.from_numpy(rois[rois[:, 0] == i, 1:]) for i in range(2)]
    a, b = U.AlignOracle(cfg, {}).pool(x, boxes), U.AlignOracle(cfg, {}, emulate="fp16").pool(x, boxes)
    assert torch.equal(a.half().float(), b) and not torch.equal(a, b)
