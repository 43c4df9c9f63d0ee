"""-m gpu: grid features, `FRCNN.forward(grid=(Gh, Gw))` (vk_forward_grid_begin, vk_grid_pool).

Pinned four ways: (1) vk_grid_pool bit for bit against the numpy restatement of the contract (tests/grid_util.py) -- one
summation order, fp64, no atomics, so there is no tolerance; (2) Res5 conv2 on integer data at map widths on both sides of
the panel kernel's reach (dil * (W + 1) <= 128), bit-exact, with the route asserted; (3) the model stage-chained: its
roi_features and boxes equal the restatement applied to the device's own "grid_map", exactly, while "grid_map" and the
predictor are held to the oracle at the bounds of tests/test_gpu_given_boxes.py (1e-4 strict, 1e-3 against the fp16-emulating
oracle); (4) the reference's vectors (tests/golden/e2e_grid.npz): strict mode 1e-3 with equal ids and boxes, fp16 mode 1e-3 on
features, 3e-2 on probabilities, ids where the stored margin exceeds 5e-2.
"""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.frcnn_oracle import FRCNNOracle            # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
import grid_util as GU                                 # noqa: E402
from exact_util import Case                            # noqa: E402
from test_gpu_conv_exact import assert_exact, run_case   # noqa: E402

NPDT = {L.VK_F16: np.float16, L.VK_F32: np.float32}


# ---- 1. vk_grid_pool, bit for bit ------------------------------------------------------------------------------------
# (map Hm x Wm, image content sizes, grids): a 5 x 7 map with a full and a partial image; a 16 x 22 map whose second image is one
# pixel (every cell is that map pixel) under a grid with more rows than the map has
POOL_SHAPES = [((5, 7), ((80, 112), (40, 50)), ((1, 1), (2, 3), (5, 7), (7, 3))),
               ((16, 22), ((256, 352), (1, 1)), ((20, 3),))]
SCALES = ((1.25, 1.5), (2.0, 1.75))


def _grid_pool(m, hws, S, grid, scales, dt):
    N, Hm, Wm, Cc = m.shape
    Gn = grid[0] * grid[1]
    md = torch.from_numpy(m).to(G.DEV)
    hw = torch.tensor(hws, dtype=torch.int32, device=G.DEV)
    sc = torch.tensor(scales, dtype=torch.float32, device=G.DEV) if scales is not None else None
    feat = torch.full((N * Gn, Cc), float("nan"), dtype=torch.float32, device=G.DEV)
    boxes = torch.full((N, Gn, 4), float("nan"), dtype=torch.float32, device=G.DEV)
    L.call("vk_grid_pool", G.P(md), N, Hm, Wm, Cc, dt, G.P(hw), G.P(sc), S, grid[0], grid[1], G.P(feat), Cc, G.P(boxes), G.stream())
    torch.cuda.synchronize()
    return feat.view(N, Gn, Cc).cpu().numpy(), boxes.cpu().numpy()


@pytest.mark.parametrize("dt", [L.VK_F16, L.VK_F32], ids=["f16", "f32"])
@pytest.mark.parametrize("Cc", [8, 12, 2048, 2056])       # one lane; the scalar path; 256 lanes x 8; a lane's second round
def test_grid_pool_bit_exact(dt, Cc):
    rng = np.random.default_rng(1000 * dt + Cc)
    for (Hm, Wm), hws, grids in POOL_SHAPES:
        m = (rng.standard_normal((2, Hm, Wm, Cc)) * 3).astype(NPDT[dt])
        for grid in grids:
            want_f = GU.pool(m, hws, 16, grid)
            for scales in (None, SCALES):
                feat, boxes = _grid_pool(m, hws, 16, grid, scales, dt)
                np.testing.assert_array_equal(feat.view(np.uint32), want_f.view(np.uint32), err_msg=f"features {grid} C={Cc}")
                want_b = GU.boxes(hws, Hm, Wm, 16, grid, scales)
                np.testing.assert_array_equal(boxes.view(np.uint32), want_b.view(np.uint32), err_msg=f"boxes {grid} scales={scales}")


def test_grid_pool_stride_32_and_leading_dimension():
    """RES5HALVE's S = 32, and rows written at a pitch wider than C leave the gap alone."""
    rng = np.random.default_rng(7)
    m = rng.standard_normal((1, 4, 6, 16)).astype(np.float16)
    hws, grid = ((100, 170),), (3, 2)                       # extents ceil(100 / 32) = 4, ceil(170 / 32) = 6
    md = torch.from_numpy(m).to(G.DEV)
    hw = torch.tensor(hws, dtype=torch.int32, device=G.DEV)
    feat = torch.full((6, 24), -7.0, dtype=torch.float32, device=G.DEV)
    boxes = torch.zeros((1, 6, 4), dtype=torch.float32, device=G.DEV)
    L.call("vk_grid_pool", G.P(md), 1, 4, 6, 16, L.VK_F16, G.P(hw), None, 32, 3, 2, G.P(feat), 24, G.P(boxes), G.stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(feat[:, :16].cpu().numpy(), GU.pool(m, hws, 32, grid)[0])
    assert bool((feat[:, 16:] == -7.0).all())
    np.testing.assert_array_equal(boxes.cpu().numpy(), GU.boxes(hws, 4, 6, 32, grid))
    assert boxes[0, -1].tolist() == [96.0, 64.0, 170.0, 100.0]


# ---- 2. Res5 conv2 at whole-map widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,expect", [(5, 22, "panel"), (5, 70, "!panel"), (20, 70, "ring")])
def test_res5_conv2_exact_on_a_map(H, W, expect, monkeypatch):
    """512 -> 512, 3x3, pad = dilation = 2, fp16 on a [1, H, W] map: W = 22 is the small models' route (the panel kernel);
    W = 70 is past its reach (2 * (W + 1) > 128), on the generic kernel at 5 rows and, from a few tiles of rows on, on the
    route an 800 x 1333 input's 50 x 84 map takes (the 256 x 256 ring kernel)."""
    c = Case(f"grid/res5_conv2_{H}x{W}", "panel", "conv", 1, H, W, 512, 512, 3, 1, 2, 2, relu=1)
    route = G.conv_route(**c.route_geometry())
    assert route != "panel" if expect == "!panel" else route == expect, route
    assert G.conv_route(32, 50, 84, 512, 512, k=3, pad=2, dil=2, relu=1) == "ring"
    c = dataclasses.replace(c, route=route)
    got, want = run_case(c, monkeypatch)
    assert_exact(c, got, want)


# ---- 3. the model ----------------------------------------------------------------------------------------------------
def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_grid.npz"))


@pytest.fixture(scope="module")
def setup(golden):
    g = golden
    n, h, w = g["nhw"].tolist()
    cfg = vg_c4_config(depth=int(g["depth"]), post_nms_topk=30, detections=12)
    sd = make_state_dict(cfg, seed=int(g["weights_seed"]))
    x = synthetic_images(n, h, w, seed=int(g["images_seed"]))
    shapes = g["shapes"].tolist()
    for i, (hh, ww) in enumerate(shapes):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    return cfg, sd, torch.from_numpy(x), shapes


@pytest.fixture(scope="module")
def models(setup):
    cfg, sd, _, _ = setup
    return {p: FRCNN(cfg, precision=p).load_state_dict(sd).eval() for p in ("fp32", "fp16")}


def stack(out, k):
    return torch.stack([t.cpu() for t in out[k]], 0).numpy()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("grid", [(1, 1), (2, 3), (4, 5), (20, 3)])
def test_forward_is_the_restatement_of_its_own_map(setup, models, precision, grid):
    """Stage-chained and exact: roi_features = the contract's pooling of the device's "grid_map"; boxes = the cell boxes.
    (1, 1) at N = 2 is the sizing case: 2 x 196 RoI rows would not hold the 2 x 16 x 22 map."""
    cfg, sd, x, shapes = setup
    m = models[precision]
    Gn = grid[0] * grid[1]
    scales = np.asarray(SCALES, np.float32)
    for sc in (None, scales):
        out = m(x, torch.tensor(shapes), grid=grid, scales_yx=None if sc is None else torch.from_numpy(sc))
        assert out["preds_per_image"].tolist() == [Gn, Gn]
        gm = m.get_stage("grid_map")
        assert tuple(gm.shape) == (2, 16, 22, 2048) and gm.dtype == (torch.float16 if precision == "fp16" else torch.float32)
        gm = gm.cpu().numpy()
        np.testing.assert_array_equal(stack(out, "roi_features"), GU.pool(gm, shapes, 16, grid))
        np.testing.assert_array_equal(stack(out, "boxes"), GU.boxes(shapes, 16, 22, 16, grid, sc))
        np.testing.assert_array_equal(m.get_stage("proposal_boxes").cpu().numpy(), GU.boxes(shapes, 16, 22, 16, grid))
        np.testing.assert_array_equal(m.get_stage("feature_pooled").cpu().numpy().reshape(2, Gn, -1), stack(out, "roi_features"))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_map_and_predictor_vs_oracle(setup, models, precision):
    """"grid_map" against the oracle's bottlenecks, the predictor against the oracle on the device's own feature rows: 1e-4
    strict, 1e-3 against the fp16-emulating oracle (the bounds of tests/test_gpu_given_boxes.py).

    Stage-chained, as every fp16 stage of this suite is (tests/test_gpu_e2e.py): each Res5 block's output ("grid_res5_0",
    "grid_res5_1", "grid_map") against the oracle's bottleneck on the DEVICE's own input of that block.  Free-running through
    all three blocks from res4 the strict mode is held element by element too (measured 1.6e-6); in fp16 a summation-order
    difference flips single f16 roundings (one ulp is up to 9.8e-4 of the value) which then propagate through ten
    convolutions, so element by element the free-running map measured 1.27e-3 of its maximum on an MI355X -- printed here,
    and held at 1e-3 where the given-box file holds its free-running Res5 too: on the pooled feature rows."""
    cfg, sd, x, shapes = setup
    m = models[precision]
    tol = 1e-3 if precision == "fp16" else 1e-4
    oracle = FRCNNOracle(cfg, sd, emulate="fp16" if precision == "fp16" else None)
    out = m(x, torch.tensor(shapes), grid=(4, 5))
    chain = [nchw(m.get_stage(k)) for k in ("res4", "grid_res5_0", "grid_res5_1", "grid_map")]
    with torch.no_grad():
        e_blocks = [G.rel_err(chain[b + 1], oracle.bottleneck(chain[b], f"roi_heads.res5.{b}", 1, dilation=2)) for b in range(3)]
        ref_map = oracle.res5(chain[0])
    e_map = G.rel_err(chain[3], ref_map)
    e_free = G.rel_err(stack(out, "roi_features"), GU.pool(ref_map.permute(0, 2, 3, 1).numpy(), shapes, 16, (4, 5)))
    print(f"\n[{precision} grid vs oracle] Res5 blocks on their own inputs {['%.2e' % e for e in e_blocks]}; free-running from res4: "
          f"grid_map {e_map:.2e}, pooled rows {e_free:.2e}")
    assert max(e_blocks) <= tol, e_blocks
    assert e_free <= tol
    if precision == "fp32":
        assert e_map <= tol
    feat = stack(out, "roi_features").reshape(40, -1)
    Cn = cfg.ROI_HEADS.NUM_CLASSES
    pred = GU.predict(oracle, feat, Cn)
    s = m.get_stage("obj_logits").cpu().numpy()[:, :pred["obj_logits"].shape[1]]
    a = m.get_stage("attr_logits").cpu().numpy()[:, :pred["attr_logits"].shape[1]]
    e_s, e_a = G.rel_err(s, pred["obj_logits"]), G.rel_err(a, pred["attr_logits"])
    print(f"[{precision} grid vs oracle] obj_logits {e_s:.2e} attr_logits {e_a:.2e}")
    assert e_s <= tol, (e_s, e_a)
    np.testing.assert_array_equal(stack(out, "obj_ids").reshape(-1), pred["obj_ids"])
    assert G.rel_err(stack(out, "obj_probs").reshape(-1), pred["obj_probs"]) <= tol
    same = s.argmax(-1) == pred["obj_logits"].argmax(-1)            # the attribute branch embeds the raw arg-max class
    assert same.sum() > 0 and G.rel_err(a[same], pred["attr_logits"][same]) <= tol
    np.testing.assert_array_equal(stack(out, "attr_ids").reshape(-1)[same], pred["attr_ids"][same])
    assert G.rel_err(stack(out, "attr_probs").reshape(-1)[same], pred["attr_probs"][same]) <= tol


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("grid", [(2, 3), (4, 5)])
def test_reference_vectors(setup, golden, models, precision, grid):
    """The reference's modules on the same input (tests/golden/e2e_grid.npz)."""
    cfg, sd, x, shapes = setup
    g, m, tag = golden, models[precision], f"{grid[0]}x{grid[1]}"
    out = m(x, torch.tensor(shapes), grid=grid, scales_yx=torch.from_numpy(g["scales_yx"]))
    e_f = G.rel_err(stack(out, "roi_features"), g[f"roi_features_{tag}"])
    e_o = G.rel_err(stack(out, "obj_probs"), g[f"obj_probs_{tag}"])
    e_a = G.rel_err(stack(out, "attr_probs"), g[f"attr_probs_{tag}"])
    print(f"\n[{precision} grid {tag} vs reference] features {e_f:.2e} obj_probs {e_o:.2e} attr_probs {e_a:.2e}")
    assert e_f <= 1e-3
    tol_p = 1e-3 if precision == "fp32" else 3e-2
    assert e_o <= tol_p and e_a <= tol_p
    np.testing.assert_array_equal(stack(out, "boxes"), g[f"boxes_scaled_{tag}"])
    if precision == "fp32":
        np.testing.assert_array_equal(stack(out, "obj_ids"), g[f"obj_ids_{tag}"])
        np.testing.assert_array_equal(stack(out, "attr_ids"), g[f"attr_ids_{tag}"])
    else:      # the fp16 arg-max must agree wherever the stored margin exceeds the fp16 error by far
        sure = g[f"cls_margin_{tag}"].reshape(2, -1) > 5e-2
        assert sure.sum() > 0
        np.testing.assert_array_equal(stack(out, "obj_ids")[sure], g[f"obj_ids_{tag}"][sure])


# ---- 4. the call surface ---------------------------------------------------------------------------------------------
def test_call_surface(setup, models):
    cfg, sd, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    lists = m(x, hw, grid=(2, 3))
    assert [t.shape for t in lists["roi_features"]] == [(6, 2048), (6, 2048)] and lists["boxes"][0].is_cuda
    pad = m.forward_padded()
    assert pad["roi_features"].shape == (2, 6, 2048) and pad["boxes"].shape == (2, 6, 4) and pad["preds_per_image"].tolist() == [6, 6]
    t = m(x, hw, grid=(2, 3), return_tensors="pt", padding="max_detections", max_detections=8, location="cpu")
    assert t["roi_features"].shape == (2, 8, 2048) and not t["roi_features"].is_cuda and t["preds_per_image"].tolist() == [6, 6]
    assert bool((t["roi_features"][:, 6:] == 0).all()) and torch.equal(t["roi_features"][:, :6], pad["roi_features"].cpu())
    n = m(x, hw, grid=(2, 3), return_tensors="np", padding="max_batch")
    assert isinstance(n["boxes"], np.ndarray) and n["boxes"].shape == (2, 6, 4) and n["obj_ids"].shape == (2, 6)
    # image 1 (240 x 320: a 15 x 20 extent), cell (1, 2): rows 7..15, columns 13..20
    np.testing.assert_array_equal(n["boxes"][1, -1], np.float32([208, 112, 320, 240]))
    np.testing.assert_array_equal(n["normalized_boxes"][1, -1],
                                  np.float32([208, 112, 320, 240]) / np.float32([320, 240, 320, 240]))
    with pytest.raises(ValueError, match="max_detections=5"):
        m(x, hw, grid=(2, 3), padding="max_detections", max_detections=5)
    with pytest.raises(ValueError, match="max_detections=5"):
        m.forward_async(x, hw, grid=(2, 3)).wait(padding="max_detections", max_detections=5)
    assert m._open == []


# ---- 5. detection is untouched ---------------------------------------------------------------------------------------
def _launches(m):
    return {k: v["launches"] for k, v in m.kernel_timing(reset=True).items()}


def test_detection_is_untouched_by_grid_forwards(setup, models):
    """The same bits from a detection forward before and after grid forwards, and the same launches kernel by kernel."""
    cfg, sd, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    m.enable_kernel_timing(True)
    try:
        m.kernel_timing(reset=True)
        before = {k: v.clone() for k, v in m.forward_async(x, hw).wait_raw().items()}
        n_before = _launches(m)
        for grid in ((1, 1), (4, 5), (32, 32)):
            m(x, hw, grid=grid)
        n_grid = _launches(m)
        after = m.forward_async(x, hw).wait_raw()
        n_after = _launches(m)
    finally:
        m.enable_kernel_timing(False)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert n_before == n_after and sum(n_before.values()) > 0
    assert sum(n_grid.values()) > 0


@pytest.mark.parametrize("lanes", [1, 2])
def test_grid_and_detection_in_flight_together(setup, models, lanes):
    cfg, sd, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    m.set_option("forward_lanes", lanes)
    try:
        det_alone = {k: v.clone() for k, v in m.forward_async(x, hw).wait_raw().items()}
        grid_alone = {k: v.clone() for k, v in m.forward_async(x, hw, grid=(4, 5)).wait_raw().items()}
        p1 = m.forward_async(x, hw, grid=(4, 5))
        p2 = m.forward_async(x, hw)
        p3 = m.forward_async(x, hw, grid=(4, 5))
        p4 = m.forward_async(x, hw)
        b1, b2, b3, b4 = p1.wait_raw(), p2.wait_raw(), p3.wait_raw(), p4.wait_raw()
    finally:
        m.set_option("forward_lanes", 2)
    for k in det_alone:
        assert torch.equal(b2[k], det_alone[k]) and torch.equal(b4[k], det_alone[k]), k
        assert torch.equal(b1[k], grid_alone[k]) and torch.equal(b3[k], grid_alone[k]), k
    assert b1["preds_per_image"].tolist() == [20, 20]


# ---- 6. the extraction loop ------------------------------------------------------------------------------------------
def test_pipeline_writes_grid_rows(setup, models, tmp_path):
    """Three small raw images through ExtractionPipeline(grid=(2, 2)): 4 rows per image, widened to the schema's 12."""
    from vltk_amd.config import Config, vg_c4_config_dict
    from vltk_amd.extraction import load_extraction
    from vltk_amd.pipeline import ExtractionPipeline
    from vltk_amd.preprocess import Preprocess
    cfg, sd, _, _ = setup
    m = models["fp16"]
    d = vg_c4_config_dict(post_nms_topk=30, detections=12)
    d["input"]["min_size_test"], d["input"]["max_size_test"] = 96, 160
    rng = np.random.Generator(np.random.PCG64(5))
    items = [(f"id{i}", rng.integers(0, 256, s + (3,), dtype=np.uint8)) for i, s in enumerate(((60, 80), (48, 100), (75, 55)))]
    path = str(tmp_path / "train.arrow")
    try:
        pipe = ExtractionPipeline(m, Preprocess(Config(d)), path, batch_size=2, dataset="synthetic", grid=(2, 2))
        assert pipe.run(items) == path
    finally:
        m.set_option("forward_lanes", 2)
    table, _ = load_extraction(path)
    rows = {r["imgid"]: r for r in table.to_pylist()}
    assert sorted(rows) == ["id0", "id1", "id2"]
    for i, (h, w) in enumerate(((60, 80), (48, 100), (75, 55))):
        r = rows[f"id{i}"]
        f, b = np.asarray(r["features"], np.float32), np.asarray(r["box"], np.float32)
        assert f.shape == (12, 2048) and b.shape == (12, 4)
        assert np.isfinite(f).all() and (np.abs(f[:4]).sum(1) > 0).all() and (f[4:] == 0).all()
        assert (b[4:] == 0).all() and b[0, 0] == 0 and b[0, 1] == 0
        assert abs(b[3, 2] - w) <= 1 and abs(b[3, 3] - h) <= 1          # the last cell ends at the raw image's corner (rounded)
        assert len(r["object_ids"]) == 12 and r["object_ids"][4:] == [0.0] * 8
