"""-m gpu: region features for caller-supplied boxes on the FPN detector, `FRCNNFPN.forward(proposals=...)`.

The reference has no FPN model, so there is no golden file.  Pinned instead to (1) the FPN detection path -- its own
proposals fed back as given boxes give bit-identical head stages; (2) vk_assign_levels -- the ingest's levels are
bit-equal to it on the RoI rows the ingest wrote; (3) oracle/fpn_oracle.py FPNDetectorOracle, run on the GPU's own
p2..p5, for ragged, degenerate, out-of-image and scaled boxes on every pyramid level.

Tolerances as test_gpu_fpn_detector.py: strict fp32 1e-4 and fast fp16 1e-3 stage by stage, 3e-2 on soft-max
probabilities."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.fpn_oracle import FPNDetectorOracle        # noqa: E402
from vltk_amd import FRCNN, _lib as L, adapters, fpn_config, make_state_dict, synthetic_images   # noqa: E402
from vltk_amd.config import Config, fpn_config_dict    # noqa: E402
from vltk_amd.frcnn_fpn import FRCNNFPN                # noqa: E402

import gpu_util as G                                   # noqa: E402

HEAD_STAGES = ("pooled", "levels", "box_features", "obj_logits", "attr_logits")


def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def build(precision, depth=50, seed=3):
    cfg = fpn_config(depth=depth, post_nms_topk=200, pre_nms_topk=300, detections=10,
                     overrides=[("anchor_generator", "sizes", [[64], [128], [256], [512], [1024]])])
    sd = make_state_dict(cfg, seed=seed)
    m = FRCNN(cfg, precision=precision).load_state_dict(sd).eval()
    assert isinstance(m, FRCNNFPN)
    return cfg, sd, m


@pytest.fixture(scope="module")
def models():
    out = {}
    for p in ("fp32", "fp16"):
        cfg, sd, m = build(p)
        out[p] = m
    return cfg, sd, out


def inputs(n=2, h=512, w=640, shapes=((512, 640), (480, 600))):
    x = synthetic_images(n, h, w, seed=5)
    shapes = [list(s) for s in shapes][:n]
    for i, (hh, ww) in enumerate(shapes):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    return torch.from_numpy(x), shapes


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


def softmax_argmax(logits, n_softmax, n_argmax):
    """the detection path's own kernel (vk_softmax_argmax) on [K, ld] f32 device logits -> (prob, cls) on the host."""
    K = logits.shape[0]
    prob = torch.empty(K, dtype=torch.float32, device=logits.device)
    cls = torch.empty(K, dtype=torch.int32, device=logits.device)
    L.call("vk_softmax_argmax", G.P(logits), logits.shape[1], K, n_softmax, n_argmax, G.P(prob), G.P(cls), None, G.stream())
    torch.cuda.synchronize()
    return prob.cpu(), cls.cpu()


# ---- 1. detection's proposals fed back ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_detection_proposals_fed_back_are_bit_identical(models, precision):
    cfg, sd, ms = models
    m = ms[precision]
    x, shapes = inputs()
    hw = torch.tensor(shapes)
    m(x, hw)
    det = {k: m.get_stage(k).clone() for k in HEAD_STAGES + ("proposal_boxes",)}
    N, R = det["proposal_boxes"].shape[:2]
    out = m(x, hw, proposals=det["proposal_boxes"], padding="max_detections", return_tensors="pt")   # B = R: K = N * R
    assert out["preds_per_image"].tolist() == [R] * N
    assert torch.equal(m.get_stage("proposal_boxes"), det["proposal_boxes"])
    for k in HEAD_STAGES:
        assert torch.equal(m.get_stage(k), det[k]), k
    for k in ("rpn_out2", "proposal_logits", "chosen_deltas", "keep_ids", "p6"):
        with pytest.raises(KeyError):
            m.get_stage(k)
    Cn, At = cfg.ROI_HEADS.NUM_CLASSES, cfg.ROI_BOX_HEAD.NUM_ATTRS
    p, c = softmax_argmax(det["obj_logits"], Cn + 1, Cn)
    assert torch.equal(out["obj_probs"].cpu().reshape(-1), p) and torch.equal(out["obj_ids"].cpu().reshape(-1), c.long())
    p, c = softmax_argmax(det["attr_logits"], At, At)
    assert torch.equal(out["attr_probs"].cpu().reshape(-1), p) and torch.equal(out["attr_ids"].cpu().reshape(-1), c.long())
    F = det["box_features"].shape[1]
    assert torch.equal(out["roi_features"].cpu().reshape(-1, F), det["box_features"].cpu())
    assert torch.equal(out["boxes"].cpu(), det["proposal_boxes"].cpu())


# ---- 2. levels ------------------------------------------------------------------------------------------------------
def level_boxes(rng, n):
    """squares and rectangles with sqrt(area) at, and one ulp either side of, 112 / 224 / 448; random sizes; zero-area,
    inverted and out-of-image boxes."""
    out = []
    for s in (56.0, 112.0, 224.0, 448.0, 896.0):
        for side in (np.nextafter(np.float32(s), np.float32(0)), np.float32(s), np.nextafter(np.float32(s), np.float32(1e9))):
            x0, y0 = np.float32(rng.integers(0, 200)), np.float32(rng.integers(0, 200))
            out.append([x0, y0, x0 + side, y0 + side])
            out.append([x0, y0, x0 + side * np.float32(2), y0 + side / np.float32(2)])       # same area, 2:1
    for _ in range(n - len(out) - 40):
        x0, y0 = rng.uniform(-100, 1100, 2)
        w, h = np.exp(rng.uniform(np.log(1.0), np.log(1200.0), 2))
        out.append([x0, y0, x0 + w, y0 + h])
    for _ in range(10):
        x0, y0 = rng.uniform(0, 900, 2)
        out += [[x0, y0, x0, y0 + 50], [x0, y0, x0 + 50, y0], [x0, y0, x0, y0]]            # zero area
        out.append([x0 + 60, y0, x0, y0 + 80])                                              # inverted in x
    return np.asarray(out, np.float32)


def test_ingest_levels_equal_assign_levels():
    rng = np.random.default_rng(2024)
    N, B = 3, 1000
    boxes = np.stack([level_boxes(rng, B) for _ in range(N)])
    counts = np.array([B, B - 37, 500], np.int32)
    hw = np.array([[1100, 1100], [1000, 1300], [800, 1333]], np.int32)
    dev = G.DEV
    bx, cnt, hwd = (torch.from_numpy(a).to(dev) for a in (boxes, counts, hw))
    K = N * B
    pb = torch.empty((N, B, 4), device=dev)
    rois = torch.empty((K, 5), device=dev)
    lv = torch.full((K,), -7, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("vk_given_boxes_ingest", G.P(bx), G.P(cnt), G.P(hwd), None, N, B, G.P(pb), G.P(rois), G.P(lv), 2, 5, 224.0, 4,
           G.P(flag), G.stream())
    ref = torch.full((K,), -9, dtype=torch.int32, device=dev)
    L.call("vk_assign_levels", rois.data_ptr() + 4, 5, K, 2, 5, 224.0, 4, G.P(ref), G.stream())
    torch.cuda.synchronize()
    assert int(flag.cpu()) == 0
    assert torch.equal(lv, ref)
    lv = lv.cpu()
    assert int(lv.min()) == 0 and int(lv.max()) == 3 and len(torch.unique(lv)) == 4
    # the RoI rows: (n, clipped box), padding rows zero-size at the origin
    net, _ = expected_boxes([boxes[i, :counts[i]] for i in range(N)], hw.tolist())
    r = rois.cpu().view(N, B, 5)
    for i in range(N):
        assert (r[i, :, 0] == i).all()
        np.testing.assert_array_equal(r[i, :counts[i], 1:].numpy(), net[i])
        assert (r[i, counts[i]:, 1:] == 0).all() and (lv.view(N, B)[i, counts[i]:] == 0).all()
        np.testing.assert_array_equal(pb.cpu()[i, :counts[i]].numpy(), net[i])


# ---- 3. against the oracle ------------------------------------------------------------------------------------------
def oracle_boxes(rng, shapes):
    """per image: whole-image, per-level, zero-area and out-of-image boxes (network pixels)."""
    out = []
    for h, w in shapes:
        b = [[0, 0, w, h], [-30, -20, w + 50, h + 40], [0, 0, w / 2, h / 2]]
        for s in (24, 48, 90, 150, 260, 420):                   # sqrt(area) on every level 2..5
            x0, y0 = rng.uniform(0, max(w - s, 1)), rng.uniform(0, max(h - s, 1))
            b.append([x0, y0, x0 + s * 1.3, y0 + s / 1.3])
        b += [[10, 20, 10, 80], [30, 40, 90, 40], [50, 50, 50, 50]]                      # zero area
        b += [[w - 20, h - 30, w + 100, h + 100], [-80, -60, -10, -5], [w + 5, 10, w + 60, 50]]   # partly / fully outside
        for _ in range(20):
            x0, y0 = rng.uniform(-40, w), rng.uniform(-40, h)
            b.append([x0, y0, x0 + rng.uniform(2, w), y0 + rng.uniform(2, h)])
        out.append(np.asarray(b, np.float32))
    return out


def oracle_check(m, o, out, net, tol, C):
    """stages of the last given-box forward against the oracle on the GPU's own upstream tensors, and the outputs."""
    N = len(net)
    B = max(len(b) for b in net)
    counts = [len(b) for b in net]
    rows = np.concatenate([np.arange(c) + i * B for i, c in enumerate(counts)]).astype(np.int64)
    pb = m.get_stage("proposal_boxes").cpu()
    for i in range(N):
        np.testing.assert_array_equal(pb[i, :counts[i]].numpy(), net[i])
    pyr = [nchw(m.get_stage(f"p{i}")) for i in range(2, 6)]
    pooled_ref, lv_ref = o.box_pool(pyr, [torch.from_numpy(b) for b in net])
    np.testing.assert_array_equal(m.get_stage("levels").cpu().numpy()[rows], lv_ref.numpy())
    pooled = m.get_stage("pooled").float().permute(0, 3, 1, 2).cpu()[rows]
    assert G.rel_err(pooled, pooled_ref) <= (2e-3 if o.emulate else 1e-5)
    feat = m.get_stage("box_features").cpu()[rows]
    assert G.rel_err(feat, o.box_head(pooled)) <= tol
    s_ref, a_ref, _ = o.predictor(feat)
    C1, A1 = s_ref.shape[1], a_ref.shape[1]
    s = m.get_stage("obj_logits").cpu()[rows][:, :C1]
    assert G.rel_err(s, s_ref) <= tol
    same = (s.argmax(-1) == s_ref.argmax(-1)).numpy()
    a = m.get_stage("attr_logits").cpu()[rows][:, :A1]
    assert G.rel_err(a[same], a_ref[same]) <= tol
    # outputs: ids are the arg-max of the GPU's own logits, probabilities the oracle's soft-max
    sp = torch.softmax(s_ref, -1)[:, :C]
    ap = torch.softmax(a_ref, -1)
    cat = lambda k: torch.cat([out[k][i].cpu() for i in range(N)], 0)                 # noqa: E731
    np.testing.assert_array_equal(cat("obj_ids").numpy(), s[:, :C].argmax(-1).numpy())
    np.testing.assert_array_equal(cat("attr_ids").numpy(), a.argmax(-1).numpy())
    assert G.rel_err(cat("obj_probs"), sp.max(-1).values) <= 3e-2
    assert G.rel_err(cat("attr_probs")[same], ap.max(-1).values[same]) <= 3e-2
    assert torch.equal(cat("roi_features"), feat)
    assert out["preds_per_image"].tolist() == counts


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("fp16", 1e-3)])
@pytest.mark.parametrize("scaled", [False, True])
def test_ragged_degenerate_scaled_boxes_vs_oracle(models, precision, tol, scaled):
    cfg, sd, ms = models
    m = ms[precision]
    x, shapes = inputs(3, shapes=((512, 640), (480, 600), (512, 520)))
    rng = np.random.default_rng(7)
    net_in = oracle_boxes(rng, shapes)
    net_in[1] = np.zeros((0, 4), np.float32)                                         # one image without boxes
    net_in[2] = net_in[2][:5]
    scales = [[1.25, 0.8], [2.0, 2.0], [0.5, 1.5]] if scaled else None
    props = [b * np.float32([scales[i][1], scales[i][0]] * 2) for i, b in enumerate(net_in)] if scaled else net_in
    out = m(x, torch.tensor(shapes), proposals=props, scales_yx=torch.tensor(scales) if scaled else None)
    net, ret = expected_boxes(props, shapes, scales)
    o = FPNDetectorOracle(cfg, sd, emulate=None if precision == "fp32" else "fp16")
    oracle_check(m, o, out, net, tol, cfg.ROI_HEADS.NUM_CLASSES)
    lv = m.get_stage("levels").cpu()[:len(net[0])]
    assert len(torch.unique(lv)) == 4, lv.bincount()                                # every level is used
    for i in range(3):
        np.testing.assert_array_equal(out["boxes"][i].cpu().numpy(), ret[i])
    # the padded block: width max K_i, rows beyond K_i zero
    blk = m.forward_padded()
    B = max(len(b) for b in props)
    assert blk["roi_features"].shape == (3, B, 1024) and blk["obj_ids"].shape == (3, B)
    for i in range(3):
        for k in ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "roi_features"):
            assert (blk[k][i, len(props[i]):] == 0).all(), (k, i)


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("fp16", 1e-3)])
def test_single_box_vs_oracle(models, precision, tol):
    cfg, sd, ms = models
    m = ms[precision]
    x, shapes = inputs()
    props = [np.array([[33.5, 40.25, 300.0, 260.0]], np.float32), np.zeros((0, 4), np.float32)]
    out = m(x, torch.tensor(shapes), proposals=props)
    assert out["preds_per_image"].tolist() == [1, 0]
    o = FPNDetectorOracle(cfg, sd, emulate=None if precision == "fp32" else "fp16")
    oracle_check(m, o, out, expected_boxes(props, shapes)[0], tol, cfg.ROI_HEADS.NUM_CLASSES)


# ---- 4. edges -------------------------------------------------------------------------------------------------------
def test_nonfinite_empty_errors_and_detection_after(models):
    cfg, sd, ms = models
    m = ms["fp16"]
    x, shapes = inputs()
    hw = torch.tensor(shapes)
    m(x, hw)
    det = {k: v.clone() for k, v in m.forward_padded().items()}
    good = [np.array([[10, 20, 200, 220], [0, 0, 640, 512]], np.float32), np.array([[5, 5, 90, 60]], np.float32)]
    m(x, hw, proposals=good)
    ref = {k: v.clone() for k, v in m.forward_padded().items()}
    nan = [good[0], np.array([[1.0, 2.0, float("inf"), 4.0]], np.float32)]
    with pytest.raises(AssertionError, match="infinite or NaN"):
        m(x, hw, proposals=nan)
    with pytest.raises(AssertionError, match="infinite or NaN"):                    # a zero scale makes the box infinite
        m(x, hw, proposals=good, scales_yx=torch.tensor([[1.0, 1.0], [0.0, 1.0]]))
    m(x, hw, proposals=good)                                                          # the model is fine afterwards
    for k, v in ref.items():
        assert torch.equal(m.forward_padded()[k], v), k
    # every image empty: nothing runs, zero counts
    out = m(x, hw, proposals=[[], np.zeros((0, 4), np.float32)])
    assert out["preds_per_image"].tolist() == [0, 0]
    assert out["roi_features"][0].shape == (0, 1024) and out["boxes"][1].shape == (0, 4)
    t = m(x, hw, proposals=torch.zeros(2, 0, 4), return_tensors="pt", padding="max_batch")
    assert t["roi_features"].shape == (2, 0, 1024) and t["preds_per_image"].tolist() == [0, 0]
    # errors before anything is enqueued
    with pytest.raises(ValueError):
        m(x, hw, proposals=good, ignorey=[np.zeros((1, 2))] * 2, scales_yx=torch.ones(2, 2))
    for bad in ([good[0]], [np.zeros((3, 5), np.float32), good[1]], torch.zeros(2, 3),
                [np.zeros((1025, 4), np.float32), good[1]], torch.zeros(2, 1025, 4)):
        with pytest.raises(ValueError):
            m(x, hw, proposals=bad)
    with pytest.raises(ValueError):
        m(x, hw, proposals=good, padding="max_detections", max_detections=1)
    with pytest.raises(ValueError):
        m.forward_async(x, hw, proposals=good).wait(max_detections=1)
    with pytest.raises(NotImplementedError):
        m.train()(x, hw, proposals=good)
    m.eval()
    # detection after all of it: its earlier outputs bit for bit
    m(x, hw)
    for k, v in det.items():
        assert torch.equal(m.forward_padded()[k], v), k


def test_stage_timing_slots(models):
    cfg, sd, ms = models
    m = ms["fp16"]
    x, shapes = inputs()
    m.enable_stage_timing(True)
    try:
        m(x, torch.tensor(shapes), proposals=[np.array([[10, 20, 200, 220]], np.float32)] * 2)
        t = m.stage_timing_ms()
    finally:
        m.enable_stage_timing(False)
    assert set(t) == {"backbone", "neck", "rpn_head", "proposals", "box_head", "predictor_outputs", "total"}
    assert t["rpn_head"] < 0.05 and t["backbone"] > 0


# ---- 5. full size ---------------------------------------------------------------------------------------------------
def test_full_size_36_boxes_fp16_images_independent():
    cfg = fpn_config(post_nms_topk=1000, detections=36)
    sd = make_state_dict(cfg, seed=1234)
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    N, H, W = 32, 800, 1333
    x = torch.from_numpy(synthetic_images(N, H, W, seed=0x36B))
    rng = np.random.default_rng(36)
    props = []
    for _ in range(N):
        x0, y0 = rng.uniform(-20, W - 40, 36), rng.uniform(-20, H - 40, 36)
        props.append(np.stack([x0, y0, x0 + rng.uniform(8, 700, 36), y0 + rng.uniform(8, 600, 36)], 1).astype(np.float32))
    hw = torch.tensor([[H, W]] * N)
    out = m(x, hw, proposals=props, padding="max_detections", return_tensors="pt")
    assert out["preds_per_image"].tolist() == [36] * N
    assert out["roi_features"].shape == (N, 36, 1024)
    for k in ("roi_features", "obj_probs", "attr_probs", "boxes"):
        assert torch.isfinite(out[k]).all(), k
    net, ret = expected_boxes(props, [[H, W]] * N)
    np.testing.assert_array_equal(out["boxes"].cpu().numpy(), np.stack(ret))
    # images are independent: a batch of one gives the same rows (to the fp16 tolerance: the convolutions of a batch of
    # one may take other kernels than those of a batch of 32)
    for i in (0, 13, N - 1):
        one = m(x[i:i + 1], hw[i:i + 1], proposals=props[i:i + 1], padding="max_detections", return_tensors="pt")
        assert torch.equal(one["boxes"][0], out["boxes"][i])
        assert G.rel_err(one["roi_features"][0].cpu(), out["roi_features"][i].cpu()) <= 1e-3, i
        assert G.rel_err(one["obj_probs"][0].cpu(), out["obj_probs"][i].cpu()) <= 3e-2, i
        assert (one["obj_ids"][0] == out["obj_ids"][i]).float().mean() >= 0.9, i


# ---- 6. adapter and extraction --------------------------------------------------------------------------------------
def small_fpn_cfg():
    d = fpn_config_dict(depth=50, post_nms_topk=64, pre_nms_topk=128, detections=8)
    d["input"]["min_size_test"], d["input"]["max_size_test"] = 96, 160
    return Config(d)


def write_images(root, dataset, spec):
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(17))
    for split, files in spec.items():
        os.makedirs(os.path.join(root, dataset, split), exist_ok=True)
        for name, (h, w), ext in files:
            a = g.uniform(0, 255, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
            Image.fromarray(a).resize((w, h), Image.BICUBIC).save(os.path.join(root, dataset, split, f"{name}.{ext}"))


def test_extract_and_adapter_with_boxes_on_fpn(tmp_path):
    from vltk_amd.preprocess import Preprocess
    cfg = small_fpn_cfg()
    sd = make_state_dict(cfg, seed=99)
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    assert isinstance(m, FRCNNFPN) and m.visual_dim == 1024
    root = str(tmp_path)
    spec = {"train": [("100", (120, 150), "jpg"), ("101", (200, 140), "jpg"), ("102", (90, 160), "png"), ("103", (130, 130), "jpg")]}
    write_images(root, "coco2014", spec)
    rng = np.random.default_rng(3)
    given = {}
    for name, (h, w), _ in spec["train"]:
        k = int(rng.integers(1, 7))
        x0, y0 = rng.uniform(-10, w - 10, k), rng.uniform(-10, h - 10, k)
        given[name] = np.stack([x0, y0, x0 + rng.uniform(3, w, k), y0 + rng.uniform(3, h, k)], 1).astype(np.float32)
    res = adapters.Adapters().get("frcnn").extract(root, dataset="coco2014", model=(m, cfg), batch_size=2, max_detections=8,
                                                   boxes=given)
    tr = res["train"]
    assert sorted(tr.imgids) == ["100", "101", "102", "103"]
    pre = Preprocess(cfg)
    files = sorted(spec["train"])
    for lo in range(0, len(files), 2):
        grp = files[lo:lo + 2]
        raws = [torch.from_numpy(adapters.decode_image_bgr(os.path.join(root, "coco2014", "train", f"{n}.{e}"))) for n, _, e in grp]
        _, images, sizes, scales_yx = pre(raws, [n for n, _, _ in grp])
        out = m(images, sizes, scales_yx=scales_yx, proposals=[given[n] for n, _, _ in grp], padding="max_detections",
                max_detections=8, return_tensors="pt", location="cpu")
        for i, (name, _, _) in enumerate(grp):
            row = tr.get(name)
            k = len(given[name])
            feats = np.asarray(row["features"], np.float32)
            assert feats.shape == (8, 1024) and (feats[k:] == 0).all()
            np.testing.assert_array_equal(feats, out["roi_features"][i].numpy())
            np.testing.assert_array_equal(np.asarray(row["box"], np.float32), torch.round(out["boxes"][i]).numpy())
            np.testing.assert_array_equal(np.asarray(row["object_ids"], np.float32), out["obj_ids"][i].float().numpy())
            np.testing.assert_array_equal(np.asarray(row["attr_ids"], np.float32), out["attr_ids"][i].float().numpy())
            # boxes come back clipped to the image, in original pixels
            h, w = [v for n, v, _ in spec["train"] if n == name][0]
            b = np.asarray(row["box"], np.float32)[:k]
            assert (b >= 0).all() and (b[:, 0::2] <= w + 1).all() and (b[:, 1::2] <= h + 1).all()
    # the adapter's per-entry forward routes entry["boxes"] to the given-box path
    raw = torch.from_numpy(adapters.decode_image_bgr(os.path.join(root, "coco2014", "train", "100.jpg")))
    _, images, sizes, scales_yx = pre([raw], ["100"])
    entry = {adapters.IMG: images[0], adapters.SIZE: sizes[0].tolist(), adapters.SCALE: [1.0, 1.0],
             adapters.BOXES: given["100"] / np.float32([scales_yx[0, 1], scales_yx[0, 0]] * 2)}
    row = adapters.FRCNN.forward(m, entry)
    assert len(row["object_ids"][0]) == 8 and sum(1 for _ in row["features"][0]) == 8
    assert m.get_stage("proposal_counts").tolist() == [len(given["100"])]
    both = adapters.FRCNN.forward_batch(m, [entry, entry])
    assert both["object_ids"][0] == both["object_ids"][1]
