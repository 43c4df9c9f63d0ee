"""CPU (-m "not gpu"): the host side of region features for caller-supplied boxes -- the packing / validation helper,
argument checks of vk_forward_boxes_begin that need no device, and extraction to Arrow with given boxes through a
stand-in model (the reference-processor loop and the pipelined loop)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd.frcnn import MAX_GIVEN_BOXES, check_given_width, pack_proposals
from vltk_amd.parallel import OutputBlock, output_spec


# ---- packing and validation ------------------------------------------------------------------------------------------
def test_pack_ragged_sequence():
    props = [np.arange(12, dtype=np.float64).reshape(3, 4), [], torch.tensor([[1, 2, 3, 4]])]
    boxes, counts = pack_proposals(props, 3)
    assert boxes.dtype == torch.float32 and boxes.shape == (3, 3, 4) and boxes.is_contiguous()
    assert counts.dtype == np.int32 and counts.tolist() == [3, 0, 1]
    np.testing.assert_array_equal(boxes[0].numpy(), np.arange(12, dtype=np.float32).reshape(3, 4))
    assert (boxes[1] == 0).all() and (boxes[2, 1:] == 0).all()
    assert boxes[2, 0].tolist() == [1.0, 2.0, 3.0, 4.0]


def test_pack_dense_and_empty():
    boxes, counts = pack_proposals(torch.ones(2, 5, 4, dtype=torch.float64), 2)
    assert boxes.shape == (2, 5, 4) and boxes.dtype == torch.float32 and counts.tolist() == [5, 5]
    boxes, counts = pack_proposals([[], np.zeros((0, 4))], 2)
    assert boxes.shape == (2, 0, 4) and counts.tolist() == [0, 0]
    # non-finite values pass the host: the device raises the reference's assertion
    boxes, _ = pack_proposals([np.array([[np.nan, 0, 1, 1]])], 1)
    assert torch.isnan(boxes[0, 0, 0])


@pytest.mark.parametrize("props,n", [
    ([np.zeros((3, 4))], 2),                          # wrong N
    (torch.zeros(3, 2, 4), 2),                        # wrong N, dense
    ([np.zeros((3, 5))], 1),                          # wrong last dimension
    (torch.zeros(2, 3, 5), 2),
    (np.zeros((2, 3)), 2),                            # one array that is not [N, K, 4]
    ([np.zeros((2, 2, 4))], 1),                       # an image's boxes that are not [K, 4]
    ([np.zeros((MAX_GIVEN_BOXES + 1, 4))], 1),        # K_i > 1024
    (torch.zeros(1, MAX_GIVEN_BOXES + 1, 4), 1),
])
def test_pack_rejects(props, n):
    with pytest.raises(ValueError):
        pack_proposals(props, n)


def test_given_width_is_never_truncated():
    check_given_width(36, None)
    check_given_width(36, 36)
    with pytest.raises(ValueError):
        check_given_width(36, 35)


def test_empty_output_block():
    blk = OutputBlock(output_spec(3, 0, 2048))
    assert blk["roi_features"].shape == (3, 0, 2048) and blk["preds_per_image"].shape == (3,)


# ---- C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _boxes_begin(lib, h, N=2, B=4, counts=(4, 1), hw=((64, 64), (64, 64))):
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    fake = C.c_void_p(0x1000)                   # never dereferenced: every check below runs before the device
    out = L.vk_outputs(*([0x1000] * 7))
    ticket = C.c_int64(-1)
    st = lib.vk_forward_boxes_begin(h, fake, N, 64, 64, hw.ctypes.data_as(C.c_void_p), None, fake, B,
                                    cnt.ctypes.data_as(C.c_void_p), C.byref(out), None, C.byref(ticket))
    return st, lib.vk_last_error().decode(), ticket.value


def test_forward_boxes_begin_is_exported(lib):
    assert "vk_forward_boxes_begin" in L.SIGNATURES
    assert hasattr(lib, "vk_forward_boxes_begin")


def test_forward_boxes_begin_rejects_without_a_device(lib):
    st, msg, t = _boxes_begin(lib, None)
    assert st == L.VK_EINVAL and "null handle" in msg and t == -1
    for counts, B in (((5, 1), 4), ((-1, 0), 4), ((0, 0), 1025), ((0, 0), -1)):
        st, msg, t = _boxes_begin(lib, None, B=B, counts=counts)
        assert st == L.VK_EINVAL and ("counts" in msg or "B=" in msg), msg
        assert t == -1
    st, msg, _ = _boxes_begin(lib, None, hw=((64, 64), (0, 64)))
    assert st == L.VK_EINVAL and "image_shapes" in msg


# ---- extraction with given boxes -------------------------------------------------------------------------------------
class _StubModel:
    """Given-box stand-in of vltk_amd.FRCNN's call surface: obj id = box index, features = the box."""

    def __init__(self, D, F=8):
        self.roi_outputs = SimpleNamespace(max_detections=D, min_detections=D)
        self.visual_dim, self.F, self.calls = F, F, []
        self.device = torch.device("cpu")

    def __call__(self, images, image_shapes, scales_yx=None, proposals=None, padding=None, max_detections=None, **_):
        assert proposals is not None, "detection was run instead of the given boxes"
        boxes, counts = pack_proposals(proposals, images.shape[0])
        self.calls.append((counts.tolist(), max_detections))
        N, B = boxes.shape[:2]
        W = max_detections if padding == "max_detections" and max_detections is not None else B
        blk = OutputBlock(output_spec(N, W, self.F))
        blk.flat.zero_()
        for n in range(N):
            c = int(counts[n])
            blk["boxes"][n, :c] = boxes[n, :c]          # the frame the boxes came in (scales divided, then multiplied)
            blk["obj_ids"][n, :c] = torch.arange(c)
            blk["attr_ids"][n, :c] = torch.arange(c) + 100
            blk["roi_features"][n, :c, :4] = boxes[n, :c]
            blk["preds_per_image"][n] = c
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


def test_extract_with_boxes_writes_the_given_rows(tmp_path):
    from vltk_amd.adapters import FRCNN as Adapter
    from vltk_amd.extraction import load_extraction
    _images(tmp_path, ["a", "b"])
    given = {"a": [[2.0, 3.0, 10.0, 12.0], [0.0, 0.0, 5.0, 5.0]], "b": np.array([[1.0, 1.0, 4.0, 6.0]])}
    model = _StubModel(D=4)
    # the reference processor resizes 20x30 to 800x1200: wh_scale = 40 both ways
    out = Adapter.extract(str(tmp_path), model=(model, {}), boxes=given, processor="reference", max_detections=4,
                          visual_dim=8)
    assert model.calls == [([2], 4), ([1], 4)]
    table, meta = load_extraction(out["train"].path)
    rows = {r["imgid"]: r for r in table.to_pylist()}
    assert rows["a"]["object_ids"] == [0.0, 1.0, 0.0, 0.0]
    assert rows["a"]["box"][:2] == given["a"]                      # original pixels, rounded
    assert rows["b"]["box"][0] == [1.0, 1.0, 4.0, 6.0]
    assert rows["a"]["box"][2:] == [[0.0] * 4, [0.0] * 4]
    feats = np.asarray(rows["a"]["features"], np.float32)
    assert feats.shape == (4, 8)
    np.testing.assert_allclose(feats[0, :4], np.float32(given["a"][0]) * 40)   # the processed image's pixels
    assert (feats[2:] == 0).all()


def test_extract_with_missing_or_too_many_boxes_writes_nothing(tmp_path):
    from vltk_amd.adapters import FRCNN as Adapter
    _images(tmp_path, ["a", "b", "c"])
    model = _StubModel(D=4)
    with pytest.raises(ValueError, match="'b'"):
        Adapter.extract(str(tmp_path), model=(model, {}), boxes={"a": [[0, 0, 1, 1]], "c": []}, processor="reference",
                        max_detections=4)
    with pytest.raises(ValueError, match="max_detections=4"):
        Adapter.extract(str(tmp_path), model=(model, {}), boxes={"a": np.zeros((5, 4)), "b": [], "c": []},
                        processor="reference", max_detections=4)
    assert model.calls == []
    assert not any(f.endswith(".arrow") for _, _, fs in os.walk(tmp_path) for f in fs)


def test_pipeline_with_boxes_widens_to_the_schema(tmp_path):
    from vltk_amd.extraction import load_extraction
    from vltk_amd.pipeline import ExtractionPipeline

    def prep(raws, ids):
        x = torch.stack([torch.as_tensor(r).float().permute(2, 0, 1) for r in raws])
        n = x.shape[0]
        return ids, x, torch.tensor([[4, 6]] * n), torch.full((n, 2), 2.0)

    items = [(f"img{i}", np.full((4, 6, 3), i, np.uint8)) for i in range(5)]
    given = {f"img{i}": np.array([[i, 1.0, i + 2.0, 3.0]] * (i % 3), np.float32) for i in range(5)}
    model = _StubModel(D=3)
    path = str(tmp_path / "train.arrow")
    pipe = ExtractionPipeline(model, prep, path, batch_size=2, visual_dim=8, boxes=given)
    assert pipe.run(items) == path
    # batches (img0, img1), (img2, img3), (img4, img4 repeated): widths 1, 2, 1 before widening
    assert [c for c, _ in model.calls] == [[0, 1], [2, 0], [1, 1]]
    table, _ = load_extraction(path)
    rows = {r["imgid"]: r for r in table.to_pylist()}
    assert sorted(rows) == [f"img{i}" for i in range(5)]
    for i in range(5):
        r, k = rows[f"img{i}"], i % 3
        assert r["object_ids"] == [float(j) for j in range(k)] + [0.0] * (3 - k)
        assert r["box"][:k] == given[f"img{i}"].tolist()
        assert np.asarray(r["features"]).shape == (3, 8)
