"""-m gpu: region features for caller-supplied boxes, `FRCNN.forward(proposals=...)` (vk_forward_boxes_begin).

Pinned three ways: (1) the reference's own vectors -- its RPN's proposals fed back as given boxes must give its RoI
features and predictions; (2) the detection path -- the same boxes through both entry points give bit-identical head
stages; (3) the oracle, run on the GPU's own res4, for ragged, degenerate and scaled boxes.

Tolerances: fp32 strict mode 1e-3 against the reference's vectors (about 1e-5 expected) and 1e-4 against the oracle
stage by stage (as test_gpu_e2e.py); fp16 fast mode 1e-3 on RoI features against the fp32 reference and 3e-2 on the
soft-max probabilities (the bounds of smoke() and test_gpu_e2e.py), 1e-3 stage by stage against the fp16-emulating oracle.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.frcnn_oracle import FRCNNOracle            # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402

import gpu_util as G                                   # noqa: E402


def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_r101_small.npz"))


@pytest.fixture(scope="module")
def setup(golden):
    g = golden
    n, h, w = g["nhw"].tolist()
    cfg = vg_c4_config(depth=int(g["depth"]), post_nms_topk=int(g["post_topk"]), detections=int(g["det"]))
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


def cat(out, k):
    return torch.cat([t.cpu() for t in out[k]], 0)


def softmax_np(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def expected_boxes(props, shapes, scales=None):
    """_clip_box of the boxes divided by the scales (f32 IEEE), and that box times the scales: (network, returned)."""
    net, ret = [], []
    for i, b in enumerate(props):
        b = np.asarray(b, np.float32).reshape(-1, 4).copy()
        if scales is not None:
            sy, sx = np.float32(scales[i][0]), np.float32(scales[i][1])
            b[:, 0::2] /= sx
            b[:, 1::2] /= sy
        h, w = np.float32(shapes[i][0]), np.float32(shapes[i][1])
        b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], np.float32(0)), w)
        b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], np.float32(0)), h)
        r = b.copy()
        if scales is not None:
            r[:, 0::2] *= sx
            r[:, 1::2] *= sy
        net.append(b)
        ret.append(r)
    return net, ret


# ---- 1. the reference's own vectors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_reference_proposals_give_reference_features(setup, golden, models, precision):
    """The reference's RPN proposals (30 per image, network pixels) as given boxes: its feature_pooled, and the class /
    attribute arg-max and probabilities of its own logits (golden cls_margin >= 4.8e-3 keeps the arg-max stable)."""
    cfg, sd, x, shapes = setup
    g = golden
    m = models[precision]
    props = [g["proposal_boxes_0"], g["proposal_boxes_1"]]
    out = m(x, torch.tensor(shapes), proposals=props)
    assert out["preds_per_image"].tolist() == [30, 30]
    C = cfg.ROI_HEADS.NUM_CLASSES
    obj_p = softmax_np(g["obj_logits"].astype(np.float64))[:, :C]
    attr_p = softmax_np(g["attr_logits"][:, :-1].astype(np.float64))
    feat = cat(out, "roi_features")
    e_feat = G.rel_err(feat, g["feature_pooled"])
    e_obj = G.rel_err(cat(out, "obj_probs"), obj_p.max(-1))
    e_attr = G.rel_err(cat(out, "attr_probs"), attr_p.max(-1))
    print(f"\n[{precision} given boxes vs reference] feature {e_feat:.2e} obj_probs {e_obj:.2e} attr_probs {e_attr:.2e}")
    assert e_feat <= 1e-3
    tol_p = 1e-3 if precision == "fp32" else 3e-2
    assert e_obj <= tol_p and e_attr <= tol_p
    if precision == "fp32":
        np.testing.assert_array_equal(cat(out, "obj_ids").numpy(), obj_p.argmax(-1))
        np.testing.assert_array_equal(cat(out, "attr_ids").numpy(), attr_p.argmax(-1))
    else:      # the fp16 arg-max must agree wherever the golden margin exceeds the fp16 logit error by far
        sure = g["cls_margin"] > 5e-2
        assert sure.sum() > 0
        np.testing.assert_array_equal(cat(out, "obj_ids").numpy()[sure], obj_p.argmax(-1)[sure])
    # boxes: the given ones (already inside the image), unchanged; no regression
    np.testing.assert_array_equal(cat(out, "boxes").numpy(), np.concatenate(props))


# ---- 2. bit-identity with the detection path ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("chunk", [0, 17])
def test_detection_proposals_fed_back_are_bit_identical(setup, models, precision, chunk):
    cfg, sd, x, shapes = setup
    m = models[precision]
    m.set_option("head_chunk", chunk)
    try:
        m(x, torch.tensor(shapes))
        det = {k: m.get_stage(k) for k in ("proposal_boxes", "proposal_counts", "feature_pooled", "obj_logits", "attr_logits")}
        R = cfg.RPN.POST_NMS_TOPK_TEST
        assert det["proposal_boxes"].shape[1] == R
        # the whole [N, R, 4] block (rows beyond a count are the zero box the detection path pools too): B = R
        out = m(x, torch.tensor(shapes), proposals=det["proposal_boxes"])
        assert out["preds_per_image"].tolist() == [R] * len(shapes)
        for k in ("feature_pooled", "obj_logits", "attr_logits"):
            assert torch.equal(m.get_stage(k), det[k]), k
        assert torch.equal(m.get_stage("proposal_boxes"), det["proposal_boxes"])
    finally:
        m.set_option("head_chunk", 9600)


# ---- 3. against the oracle on the GPU's own res4 --------------------------------------------------------------------
def _oracle_check(m, oracle, out, props_net, tol, C):
    res4 = nchw(m.get_stage("res4"))
    nonempty = [torch.from_numpy(b) for b in props_net]
    feat = cat(out, "roi_features")
    feat_ref = oracle.res5(oracle.pool(res4, nonempty)).mean(dim=[2, 3])
    assert G.rel_err(feat, feat_ref) <= tol
    s_ref, a_ref, _ = oracle.predictor(feat)
    counts = [len(b) for b in props_net]
    B = max(counts)
    rows = np.concatenate([np.arange(c) + i * B for i, c in enumerate(counts)])
    s = m.get_stage("obj_logits").cpu()[rows][:, :s_ref.shape[1]]
    assert G.rel_err(s, s_ref) <= tol
    p = torch.softmax(s_ref.double(), -1)[:, :C]
    np.testing.assert_array_equal(cat(out, "obj_ids").numpy(), p.argmax(-1).numpy())
    assert G.rel_err(cat(out, "obj_probs"), p.max(-1).values) <= tol
    same = s.argmax(-1) == s_ref.argmax(-1)            # the attribute branch embeds the raw arg-max class
    ap = torch.softmax(a_ref[:, :-1].double(), -1)
    np.testing.assert_array_equal(cat(out, "attr_ids").numpy()[same.numpy()], ap.argmax(-1).numpy()[same.numpy()])
    assert G.rel_err(cat(out, "attr_probs")[same], ap.max(-1).values[same]) <= tol
    return feat


def test_ragged_degenerate_scaled_boxes_vs_oracle(setup, models):
    cfg, sd, _, _ = setup
    m = models["fp32"]
    x = torch.from_numpy(synthetic_images(3, 160, 224, seed=77))
    shapes = [[160, 224], [144, 200], [150, 210]]
    scales = [[1.5, 2.0], [1.0, 1.0], [0.8, 1.25]]          # (y, x): original = network * scale
    props = [np.array([[10.0, 12.0, 200.0, 150.0],          # inside
                       [-40.0, -30.0, 120.0, 90.0],         # partly outside (top-left)
                       [300.0, 100.0, 600.0, 400.0],        # partly outside (bottom-right)
                       [50.0, 60.0, 50.0, 120.0],           # zero width
                       [180.0, 90.0, 40.0, 20.0],           # x1 < x0, y1 < y0
                       [77.0, 33.0, 78.0, 34.0],            # one pixel
                       [-500.0, -500.0, 900.0, 900.0]], np.float32),  # the whole image and beyond
             np.zeros((0, 4), np.float32),
             np.array([[20.5, 30.25, 90.75, 110.0]], np.float32)]
    out = m(x, torch.tensor(shapes), proposals=props, scales_yx=torch.tensor(scales))
    assert out["preds_per_image"].tolist() == [7, 0, 1]
    net, ret = expected_boxes(props, shapes, scales)
    for i in range(3):
        np.testing.assert_array_equal(out["boxes"][i].cpu().numpy(), ret[i])
    pb = m.get_stage("proposal_boxes").cpu().numpy()
    for i in range(3):
        np.testing.assert_array_equal(pb[i, :len(net[i])], net[i])
        assert (pb[i, len(net[i]):] == 0).all()
    _oracle_check(m, FRCNNOracle(cfg, sd), out, net, 1e-4, cfg.ROI_HEADS.NUM_CLASSES)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_single_box_vs_oracle(setup, models, precision):
    """K = N * B = 1: the smallest head the plan can be asked for (196 Res5 rows)."""
    cfg, sd, x, shapes = setup
    m = models[precision]
    props = [np.array([[8.0, 6.0, 120.0, 100.0]], np.float32)]
    out = m(x[:1], torch.tensor(shapes[:1]), proposals=props)
    assert out["preds_per_image"].tolist() == [1]
    assert out["roi_features"][0].shape == (1, 2048)
    oracle = FRCNNOracle(cfg, sd, emulate="fp16" if precision == "fp16" else None)
    _oracle_check(m, oracle, out, expected_boxes(props, shapes[:1])[0], 1e-3 if precision == "fp16" else 1e-4,
                  cfg.ROI_HEADS.NUM_CLASSES)


# ---- 4. scales round trip and image order ---------------------------------------------------------------------------
def test_scales_round_trip_and_image_order(setup, models):
    cfg, sd, x, shapes = setup
    m = models["fp32"]
    scales = [[1.7, 1.3], [0.9, 2.2]]
    rng = np.random.default_rng(5)
    props = []
    for (h, w), (sy, sx) in zip(shapes, scales):
        x0 = rng.uniform(0, w * sx * 0.5, 9)
        y0 = rng.uniform(0, h * sy * 0.5, 9)
        x1 = x0 + rng.uniform(1, w * sx * 0.5, 9)
        y1 = y0 + rng.uniform(1, h * sy * 0.5, 9)
        props.append(np.stack([x0, y0, x1, y1], 1).astype(np.float32))
    out = m(x, torch.tensor(shapes), proposals=props, scales_yx=torch.tensor(scales), return_tensors="pt",
            padding="max_batch")
    for i in range(2):
        assert G.rel_err(out["boxes"][i].cpu(), props[i]) <= 1e-6
    flip = m(x[[1, 0]], torch.tensor(shapes[::-1]), proposals=props[::-1], scales_yx=torch.tensor(scales[::-1]),
             return_tensors="pt", padding="max_batch")
    for k in ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "roi_features"):
        assert torch.equal(flip[k][[1, 0]], out[k]), k


# ---- 5. detection and given-box forwards in flight together ---------------------------------------------------------
def test_mixed_forwards_in_flight(setup, models):
    cfg, sd, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    props = [np.array([[5.0, 5.0, 80.0, 60.0], [30.0, 20.0, 150.0, 120.0]], np.float32),
             np.array([[0.0, 0.0, 100.0, 100.0]], np.float32)]
    det_alone = {k: v.clone() for k, v in m.forward_async(x, hw).wait_raw().items()}
    given_alone = {k: v.clone() for k, v in m.forward_async(x, hw, proposals=props).wait_raw().items()}
    p1 = m.forward_async(x, hw)
    p2 = m.forward_async(x, hw, proposals=props)
    p3 = m.forward_async(x, hw)
    b1, b2, b3 = p1.wait_raw(), p2.wait_raw(), p3.wait_raw()
    for k in det_alone:
        assert torch.equal(b1[k], det_alone[k]), k
        assert torch.equal(b3[k], det_alone[k]), k
        assert torch.equal(b2[k], given_alone[k]), k
    assert b2["preds_per_image"].tolist() == [2, 1]


# ---- 6. full size ---------------------------------------------------------------------------------------------------
def test_full_size_36_boxes_fp16_vs_emulating_oracle():
    cfg = vg_c4_config(post_nms_topk=300, detections=100)
    sd = make_state_dict(cfg, seed=1234)
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    x = torch.from_numpy(synthetic_images(2, 800, 1333, seed=0x36B))
    shapes = [[800, 1333], [760, 1200]]
    rng = np.random.default_rng(36)
    props = []
    for h, w in shapes:
        x0, y0 = rng.uniform(-20, w - 40, 36), rng.uniform(-20, h - 40, 36)
        props.append(np.stack([x0, y0, x0 + rng.uniform(8, 500, 36), y0 + rng.uniform(8, 400, 36)], 1).astype(np.float32))
    out = m(x, torch.tensor(shapes), proposals=props)
    assert out["preds_per_image"].tolist() == [36, 36]
    torch.set_num_threads(16)
    _oracle_check(m, FRCNNOracle(cfg, sd, emulate="fp16"), out, expected_boxes(props, shapes)[0], 1e-3,
                  cfg.ROI_HEADS.NUM_CLASSES)


# ---- 7. errors ------------------------------------------------------------------------------------------------------
def test_errors_raise_before_anything_is_enqueued(setup, models):
    cfg, sd, x, shapes = setup
    m = models["fp32"]
    hw = torch.tensor(shapes)
    good = [np.zeros((3, 4), np.float32), np.zeros((2, 4), np.float32)]
    bad = [[good[0]],                                                    # N wrong
           [np.zeros((3, 5), np.float32), good[1]],                      # last dimension
           torch.zeros(2, 3),                                            # not [N, K, 4]
           [np.zeros((1025, 4), np.float32), good[1]],                   # K_i > 1024
           torch.zeros(2, 1025, 4)]
    for p in bad:
        with pytest.raises(ValueError):
            m(x, hw, proposals=p)
        assert m._open == []
    with pytest.raises(ValueError):
        m(x, hw, proposals=good, padding="max_detections", max_detections=2)
    assert m._open == []
    nan = [np.array([[1.0, 2.0, float("nan"), 4.0]], np.float32), good[1]]
    with pytest.raises(AssertionError, match="infinite or NaN"):
        m(x, hw, proposals=nan)
    inf = [good[0], np.array([[1.0, 2.0, 30.0, 40.0]], np.float32)]
    with pytest.raises(AssertionError, match="infinite or NaN"):        # a zero scale makes the box infinite
        m(x, hw, proposals=inf, scales_yx=torch.tensor([[1.0, 1.0], [0.0, 1.0]]))
    # the handle is fine afterwards
    out = m(x, hw, proposals=good)
    assert out["preds_per_image"].tolist() == [3, 2]


# ---- 8. every image empty -------------------------------------------------------------------------------------------
def test_all_images_empty(setup, models):
    cfg, sd, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    out = m(x, hw, proposals=[[], np.zeros((0, 4), np.float32)])
    assert out["preds_per_image"].tolist() == [0, 0]
    for i in range(2):
        assert out["boxes"][i].shape == (0, 4) and out["roi_features"][i].shape == (0, 2048)
        assert out["obj_ids"][i].shape == (0,)
    t = m(x, hw, proposals=torch.zeros(2, 0, 4), return_tensors="pt", padding="max_batch")
    assert t["roi_features"].shape == (2, 0, 2048) and t["boxes"].shape == (2, 0, 4)
    assert t["preds_per_image"].tolist() == [0, 0]
    # and the next detection forward is untouched by it
    det = m(x, hw)
    assert int(det["preds_per_image"].sum()) > 0
