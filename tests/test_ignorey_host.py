"""CPU (-m "not gpu"): the host side of ignorey= (find_top_rpn_proposals frcnn.py:328-366) -- the test-local restatement
against the reference's own candidates (tests/golden/e2e_ignorey.npz), the packing / validation helper, the C ABI's new
entry points, and extraction with bands through a stand-in model."""
import ctypes as C
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd.frcnn import MAX_IGNOREY, pack_ignorey, pack_proposals
from vltk_amd.parallel import OutputBlock, output_spec

from ignorey_util import band_restatement, scaled_bands


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_ignorey.npz"))


# ---- the restatement against the reference ---------------------------------------------------------------------------
def test_restatement_matches_the_reference_candidates(golden):
    g = golden
    sc = g["scales_yx"]
    seen = set()
    for case in g["cases"].tolist():
        ig = g[f"{case}_ignorey"]
        for j, i in enumerate(g[f"{case}_images"].tolist()):
            bands = scaled_bands(ig[j], float(sc[i, 1]))
            assert bands.dtype == (torch.float64 if ig.dtype == np.float64 else torch.float32)
            pre = torch.from_numpy(g[f"{case}_{j}_pre_boxes"])
            b, keep = band_restatement(pre, bands)
            np.testing.assert_array_equal(keep.numpy(), g[f"{case}_{j}_keep"])
            np.testing.assert_array_equal(b.numpy(), g[f"{case}_{j}_post_boxes"])
            if (~keep).any():
                seen.add("drop")
            if (b[keep, 3] != pre[keep, 3]).any():
                seen.add("top")
            if (b[keep, 1] != pre[keep, 1]).any():
                seen.add("bottom")
    assert seen == {"drop", "top", "bottom"}
    # the band outside the image changes nothing; image 0 of the batched case only trims
    assert g["outside_0_keep"].all() and (g["outside_0_post_boxes"] == g["outside_0_pre_boxes"]).all()
    assert g["batched_0_keep"].all()


def test_pack_scales_like_torch_on_the_cpu():
    sc = np.array([[1.25, 1.5], [2.0, 3.0]], np.float32)
    bands, counts, f64 = pack_ignorey([[[10.0, 20.5], [7, 9]], []], sc, 2)
    assert not f64 and bands.dtype == np.float32 and bands.shape == (2, 2, 2) and counts.tolist() == [2, 0]
    np.testing.assert_array_equal(bands[0], (torch.tensor([[10.0, 20.5], [7, 9]]) * 1 / torch.tensor(sc)[0, 1]).numpy())
    assert (bands[1] == 0).all()
    x = np.array([[[0.1, 1e-3]], [[5.0, 6.0]]], np.float64)
    bands, counts, f64 = pack_ignorey(x, sc, 2)
    assert f64 and bands.dtype == np.float64 and counts.tolist() == [1, 1]
    np.testing.assert_array_equal(bands[0, 0], (torch.from_numpy(x[0, 0]) * 1 / torch.tensor(sc)[0, 1]).numpy())
    assert bands[0, 0, 0] != np.float64(np.float32(0.1) / np.float32(1.5))        # float64 all the way
    assert pack_ignorey([[], np.zeros((0, 2))], sc, 2) is None                      # no band at all


def test_pack_without_scales_warns_and_does_nothing():
    with pytest.warns(UserWarning, match="scales_yx"):
        assert pack_ignorey(np.zeros((1, 1, 2)), None, 1) is None
    with pytest.raises(ValueError):                     # the shape is still checked
        pack_ignorey(np.zeros((1, 1, 3)), None, 1)


@pytest.mark.parametrize("ig,n", [
    (np.zeros((2, 1, 2)), 1),                           # wrong N
    ([np.zeros((1, 2))], 2),
    (np.zeros((1, 2)), 1),                              # not [N, J, 2] (the reference asserts ndim == 3)
    (np.zeros((1, 1, 3)), 1),
    ([np.zeros((1, 3))], 1),
    ([np.zeros((MAX_IGNOREY + 1, 2))], 1),              # J_i > 64
    ([np.array([[0.0, np.inf]])], 1),                   # int() of a non-finite band raises in the reference
    ([np.array([[np.nan, 1.0]])], 1),
    ([np.array([[0.0, 2.0 ** 31]])], 1),                # beyond int32
    ([np.array([[True, False]])], 1),
])
def test_pack_rejects(ig, n):
    with pytest.raises(ValueError):
        pack_ignorey(ig, np.ones((n, 2), np.float32), n)


def test_pack_rejects_a_zero_scale():
    with pytest.raises(ValueError):
        pack_ignorey([[[1.0, 2.0]]], np.array([[1.0, 0.0]], np.float32), 1)


# ---- C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_new_exports_and_argtypes(lib):
    assert L.VK_MAX_IGNOREY == 64 and C.sizeof(L.vk_ignorey) == 24
    for name, old in (("vk_forward_begin_ignorey", "vk_forward_begin"), ("vk_rpn_proposals_ignorey", "vk_rpn_proposals"),
                      ("vk_rpn_proposals_multilevel_ignorey", "vk_rpn_proposals_multilevel")):
        assert hasattr(lib, name), name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[:-1] == L.SIGNATURES[old][1] and args[-1] == C.POINTER(L.vk_ignorey), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vltk_hip.h")).read()
    assert "typedef struct vk_ignorey" in header and "#define VK_MAX_IGNOREY 64" in header


def test_forward_begin_ignorey_checks_before_the_device(lib):
    fake = C.c_void_p(0x1000)
    hw = np.full((1, 2), 64, np.int32)
    rp = L.vk_roi_params()
    out = L.vk_outputs(*([0x1000] * 7))
    t = C.c_int64(-1)
    st = lib.vk_forward_begin_ignorey(None, fake, 1, 64, 64, hw.ctypes.data_as(C.c_void_p), None, C.byref(rp), C.byref(out), None,
                                      C.byref(t), None)
    assert st == L.VK_EINVAL and "null" in lib.vk_last_error().decode() and t.value == -1


def test_rpn_ignorey_rejects_a_bad_table(lib):
    fake = C.c_void_p(0x1000)
    ws = lib.vk_rpn_workspace_bytes(1, 16, 16)
    wts = (C.c_float * 4)(1, 1, 1, 1)
    cnt = np.zeros(1, np.int32)
    for maxj, f64 in ((MAX_IGNOREY + 1, 0), (4, 2)):
        ig = L.vk_ignorey(0x1000, cnt.ctypes.data, maxj, f64)
        st = lib.vk_rpn_proposals_ignorey(fake, 1, fake, 4, 1, 4, 4, 1, fake, 16, 0.0, fake, wts, 0.0, 0.7, 16, 8, fake, fake, fake,
                                          fake, fake, ws, None, C.byref(ig))
        assert st == L.VK_EINVAL and "ignorey" in lib.vk_last_error().decode()


# ---- extraction with bands -------------------------------------------------------------------------------------------
class _StubModel:
    """Detection stand-in of vltk_amd.FRCNN's call surface that records the bands (and scales) it was given."""

    def __init__(self, D, F=8):
        self.roi_outputs = SimpleNamespace(max_detections=D, min_detections=D)
        self.visual_dim, self.F, self.calls = F, F, []
        self.device = torch.device("cpu")

    def __call__(self, images, image_shapes, scales_yx=None, proposals=None, ignorey=None, padding=None, **_):
        assert proposals is None
        N = images.shape[0]
        self.calls.append((None if ignorey is None else [torch.as_tensor(b).reshape(-1, 2).tolist() for b in ignorey],
                           None if scales_yx is None else torch.as_tensor(scales_yx).tolist()))
        blk = OutputBlock(output_spec(N, self.roi_outputs.max_detections, self.F))
        blk.flat.zero_()
        self._blk = blk
        return blk

    def forward_padded(self):
        return self._blk


def _images(root, names, size=(20, 30)):
    from PIL import Image
    d = root / "train"
    d.mkdir()
    for i, n in enumerate(names):
        Image.fromarray(np.full((size[0], size[1], 3), 40 * i, np.uint8)).save(d / f"{n}.jpg")


def test_extract_routes_bands_by_imgid(tmp_path):
    from vltk_amd.adapters import FRCNN as Adapter
    _images(tmp_path, ["a", "b"])
    model = _StubModel(D=2)
    Adapter.extract(str(tmp_path), model=(model, {}), ignorey={"a": [[2.0, 3.5]]}, processor="reference", max_detections=2,
                    visual_dim=8)
    # the reference processor resizes 20x30 to 800x1200: wh_scale = 40; the adapter hands the model processed rows and
    # scales_yx = 1; "b" has no entry: no bands, a plain forward
    assert sorted(model.calls, key=str) == sorted([([[[80.0, 140.0]]], [[1.0, 1.0]]), (None, None)], key=str)


def test_extract_with_bad_bands_writes_nothing(tmp_path):
    from vltk_amd.adapters import FRCNN as Adapter
    _images(tmp_path, ["a"])
    model = _StubModel(D=2)
    with pytest.raises(ValueError, match="64"):
        Adapter.extract(str(tmp_path), model=(model, {}), ignorey={"a": np.zeros((65, 2))}, processor="reference", max_detections=2)
    with pytest.raises(ValueError, match="finite"):
        Adapter.extract(str(tmp_path), model=(model, {}), ignorey={"a": [[0.0, np.nan]]}, processor="reference", max_detections=2)
    with pytest.raises(ValueError, match="boxes"):
        Adapter.extract(str(tmp_path), model=(model, {}), ignorey={"a": [[0.0, 1.0]]}, boxes={"a": [[0, 0, 1, 1]]},
                        processor="reference", max_detections=2)
    assert model.calls == []
    assert not any(f.endswith(".arrow") for _, _, fs in os.walk(tmp_path) for f in fs)


def test_pipeline_routes_bands_by_imgid(tmp_path):
    from vltk_amd.pipeline import ExtractionPipeline

    def prep(raws, ids):
        x = torch.stack([torch.as_tensor(r).float().permute(2, 0, 1) for r in raws])
        n = x.shape[0]
        return ids, x, torch.tensor([[4, 6]] * n), torch.full((n, 2), 2.0)

    items = [(f"img{i}", np.full((4, 6, 3), i, np.uint8)) for i in range(3)]
    bands = {"img0": np.array([[1.0, 2.0]], np.float32), "img2": np.array([[3.0, 4.0], [5.0, 6.0]], np.float32)}
    model = _StubModel(D=3)
    pipe = ExtractionPipeline(model, prep, str(tmp_path / "train.arrow"), batch_size=2, visual_dim=8, ignorey=bands)
    pipe.run(items)
    # batches (img0, img1), (img2, img2 repeated); raw-image rows, the forward's scales_yx take them to the processed image
    assert [c[0] for c in model.calls] == [[[[1.0, 2.0]], []], [[[3.0, 4.0], [5.0, 6.0]]] * 2]
    assert all(c[1] == [[2.0, 2.0]] * 2 for c in model.calls)
