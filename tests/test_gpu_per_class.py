"""-m gpu: roi_outputs.selection = "per_class" on the GPU (vltk_amd/csrc/per_class.hip).

Kernel level: vk_per_class_select against the tests' restatement of the contract (tests/per_class_util.py) on identical
crafted inputs, everything bit-exact.  The crafted size deltas are zero: exp(0) is exact on both sides, so every decoded box --
and with it every IoU and every suppression -- is the same IEEE arithmetic on the device and on the host.
Model level: the restatement fed the forward's own stages (stage chaining, as test_gpu_e2e.py), both precisions; the strict
mode against the vectors made from the reference's own pieces (tests/golden/e2e_per_class.npz); the default selection
untouched; ignorey composed with the mode.

The model-level stage chain is exact too.  Real deltas put exp(dw) into the decode, and the device's expf and the host's exp
may differ in the last bit, so the chain hands the restatement the device's own R*C boxes (vk_class_boxes over the forward's
box_deltas and proposal_boxes: the bits the NMS kernel holds) and the forward's own per-row attribute probabilities (stage
"attr_prob"); those two device stages are held to the host's decode and soft-max at 2e-6 beside it, the bound
test_gpu_e2e.py's stage chain holds the same decode to."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
import per_class_util as PC                            # noqa: E402

WEIGHTS = (10.0, 10.0, 5.0, 5.0)
IMG_HW = (400, 600)


# ---- kernel level ---------------------------------------------------------------------------------------------------
def craft(N, R, C, seed, agnostic=False, ties=False, counts=None, F=8):
    """Proposals in a few clusters (so that NMS has work), class-specific shifts with zero size deltas, soft-max scores."""
    g = torch.Generator().manual_seed(seed)
    K = N * R
    ctr = torch.rand((N, 6, 2), generator=g) * torch.tensor([IMG_HW[1] * 0.8, IMG_HW[0] * 0.8]) + 30
    which = torch.randint(0, 6, (N, R), generator=g)
    c = ctr[torch.arange(N)[:, None], which] + torch.randn((N, R, 2), generator=g) * 25
    wh = torch.rand((N, R, 2), generator=g) * 110 + 20
    props = torch.cat([c - wh / 2, c + wh / 2], -1).float()
    nb = 1 if agnostic else C
    deltas = torch.zeros((K, nb, 4))
    deltas[:, :, :2] = torch.randn((K, nb, 2), generator=g) * 2.0           # / 10 -> shifts of ~0.2 of the box size
    scores = torch.softmax(torch.randn((K, C + 1), generator=g) * 3.0, -1)
    if ties:
        scores = torch.round(scores * 64) / 64                               # many exact ties, zeros included
    deltas = deltas.reshape(K, nb * 4)
    if ties and R >= 8:
        for n in range(N):                                                   # duplicate boxes: rows 1 and 5 copy rows 0 and 4
            for src, dst in ((0, 1), (4, 5)):
                props[n, dst] = props[n, src]
                deltas[n * R + dst] = deltas[n * R + src]
                scores[n * R + dst] = scores[n * R + src]
    feats = torch.randn((K, F), generator=g)
    cnt = np.full(N, R, np.int32) if counts is None else np.asarray(counts, np.int32)
    return dict(N=N, R=R, C=C, props=props.contiguous(), deltas=deltas.contiguous(), scores=scores.contiguous(), feats=feats,
                counts=cnt, agnostic=agnostic, hw=np.asarray([IMG_HW] * N, np.int32))


def gpu_select(d, t, score, lo, hi, scales=None, attr_logits=None):
    N, R, Cn, F = d["N"], d["R"], d["C"], d["feats"].shape[1]
    dev = G.DEV
    sc, dl, pr, ft = (d[k].to(dev) for k in ("scores", "deltas", "props", "feats"))
    cn, hw = torch.from_numpy(d["counts"]).to(dev), torch.from_numpy(d["hw"]).to(dev)
    scd = torch.as_tensor(scales, dtype=torch.float32).to(dev) if scales is not None else None
    al = attr_logits.to(dev) if attr_logits is not None else None
    o = dict(obj_ids=torch.full((N, hi), -7, dtype=torch.int64, device=dev), obj_probs=torch.full((N, hi), -7.0, device=dev),
             attr_ids=torch.full((N, hi), -7, dtype=torch.int64, device=dev), attr_probs=torch.full((N, hi), -7.0, device=dev),
             boxes=torch.full((N, hi, 4), -7.0, device=dev), preds_per_image=torch.full((N,), -7, dtype=torch.int64, device=dev),
             roi_features=torch.full((N, hi, F), -7.0, device=dev))
    keep = torch.full((N, hi), -7, dtype=torch.int64, device=dev)
    conf = torch.full((N, R), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = L.vk_outputs(*[o[k].data_ptr() for k in ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "preds_per_image",
                                                    "roi_features")])
    sp = L.vk_select_params()
    sp.mode, sp.score_thresh = L.VK_SELECT_PER_CLASS, score
    sp.roi.num_nms_thresh, sp.roi.min_detections, sp.roi.max_detections = 1, lo, hi
    sp.roi.nms_thresh[0] = t
    w = (C.c_float * 4)(*WEIGHTS)
    L.call("vk_per_class_select", G.P(sc), sc.shape[1], G.P(al), al.shape[1] if al is not None else 0, G.P(dl), dl.shape[1],
           int(d["agnostic"]), G.P(pr), G.P(cn), G.P(ft), F, N, R, Cn, al.shape[1] - 1 if al is not None else 0, G.P(hw), G.P(scd), w,
           C.byref(sp), C.byref(out), G.P(keep), G.P(conf), G.P(flag), G.stream())
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in o.items()}
    res.update(keep_ids=keep.cpu(), max_conf=conf.cpu(), flag=int(flag.cpu()))
    return res


def check_exact(d, got, t, score, lo, hi, scales=None):
    """Every output of the device call against the restatement, bit for bit.  -> per image (n_ge, n_out)."""
    N, R = d["N"], d["R"]
    regimes = []
    for n in range(N):
        c = int(d["counts"][n])
        rows = slice(n * R, n * R + c)
        ref = PC.select_image(d["scores"][rows], d["deltas"][rows], d["props"][n, :c], d["hw"][n], WEIGHTS, t, score, lo, hi,
                              None if scales is None else scales[n])
        if d["agnostic"]:
            assert d["deltas"].shape[1] == 4
        k = len(ref["ids"])
        assert int(got["preds_per_image"][n]) == k, (n, int(got["preds_per_image"][n]), k)
        np.testing.assert_array_equal(got["keep_ids"][n, :k].numpy(), ref["ids"].numpy())
        np.testing.assert_array_equal(got["obj_ids"][n, :k].numpy(), ref["classes"].numpy())
        np.testing.assert_array_equal(got["obj_probs"][n, :k].numpy(), ref["probs"].numpy())
        np.testing.assert_array_equal(got["boxes"][n, :k].numpy(), ref["boxes"].numpy())
        np.testing.assert_array_equal(got["roi_features"][n, :k].numpy(), d["feats"][rows][ref["ids"]].numpy())
        np.testing.assert_array_equal(got["max_conf"][n, :c].numpy(), ref["max_conf"].numpy())
        assert (got["max_conf"][n, c:] == 0).all()
        for key in ("keep_ids", "obj_ids", "obj_probs", "boxes", "roi_features", "attr_ids", "attr_probs"):
            assert (got[key][n, k:] == 0).all(), (key, n)       # rows beyond preds_per_image are zero
        regimes.append((int((ref["max_conf"].double() >= score).sum()), k, ref))
    assert got["flag"] == 0
    return regimes


CASES = [   # N, R, C, keyword arguments of craft
    (2, 1, 5, {}), (2, 37, 5, {}), (2, 300, 5, {}), (1, 1024, 5, {}),
    (2, 1, 1600, {}), (1, 37, 1600, {}), (2, 300, 1600, {}), (1, 1024, 1600, {}),
    (2, 37, 5, dict(agnostic=True)), (1, 300, 1600, dict(agnostic=True)),
    (2, 37, 5, dict(ties=True)), (2, 300, 5, dict(ties=True)), (1, 300, 1600, dict(ties=True)),
    (3, 37, 5, dict(counts=[37, 0, 11])), (2, 300, 1600, dict(counts=[123, 300])),
    (1, 2, 5, {}), (2, 64, 5, {}), (2, 65, 5, {}),      # the shared sort at n == T (one wavefront), the sweep's stride at 64 / 65 rows
]


@pytest.mark.parametrize("N,R,Cn,kw", CASES, ids=[f"N{n}-R{r}-C{c}" + "".join(f"-{k}" for k in kw) for n, r, c, kw in CASES])
def test_kernel_matches_restatement(N, R, Cn, kw):
    d = craft(N, R, Cn, seed=R * 7 + Cn + N, **kw)
    hi = max(1, min(R, 20))
    lo = min(5, hi)
    got = check_exact(d, gpu_select(d, 0.3, 0.2, lo, hi), 0.3, 0.2, lo, hi)
    assert got
    scales = [[1.25, 1.5], [2.0, 1.75], [0.5, 0.75]][:N]
    check_exact(d, gpu_select(d, 0.5, 0.05, lo, hi, scales=scales), 0.5, 0.05, lo, hi, scales=scales)


def test_kernel_count_regimes_and_min_above_R():
    d = craft(2, 37, 5, seed=11)
    # below the minimum -> min_detections; inside the bounds; above the maximum -> max_detections
    ref = [PC.select_image(d["scores"][n * 37:(n + 1) * 37], d["deltas"][n * 37:(n + 1) * 37], d["props"][n], IMG_HW, WEIGHTS, 0.3, 0.0, 0, 37)
           for n in range(2)]
    inside = float(np.sort(ref[0]["max_conf"].numpy())[::-1][11])           # 12 boxes of image 0 at or above it
    for score, want in ((0.999, "min"), (inside, "inside"), (0.0, "max")):
        reg = check_exact(d, gpu_select(d, 0.3, score, 5, 20), 0.3, score, 5, 20)
        n_ge, k, _ = reg[0]
        assert {"min": n_ge < 5 and k == 5, "inside": 5 < n_ge < 20 and k == n_ge, "max": n_ge > 20 and k == 20}[want], (want, n_ge, k)
    # min_detections above an image's own proposal count: every proposal of that image, ranked, and no more
    d1 = craft(2, 37, 5, seed=12, counts=[3, 37])
    reg = check_exact(d1, gpu_select(d1, 0.3, 0.999, 5, 20), 0.3, 0.999, 5, 20)
    assert [k for _, k, _ in reg] == [3, 5]
    # ... and min_detections = max_detections = R with almost nothing above the threshold: every row of both images comes out
    # (the library rejects max_detections > R, so R is the largest minimum that can reach the kernel)
    reg = check_exact(d, gpu_select(d, 0.3, 0.999, 37, 37), 0.3, 0.999, 37, 37)
    assert all(k == 37 for _, k, _ in reg)


def test_kernel_tie_rules_and_a_box_suppressed_everywhere():
    """Row 1 duplicates row 0 (box, deltas, scores): the lower row wins every class, row 1 survives in none (confidence 0,
    class 0, ranked last among ties by row).  Equal scores across classes: the smaller class."""
    d = craft(1, 12, 5, seed=5)
    d["props"][0, 1] = d["props"][0, 0]
    d["deltas"][1] = d["deltas"][0]
    d["scores"][1] = d["scores"][0]
    d["scores"][2, :5] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0])              # the image's best score, twice: class 0, not 2
    d["scores"][3] = d["scores"][2]                                           # and the same confidence on two rows: row 2 first
    d["props"][0, 2] = torch.tensor([5.0, 300.0, 45.0, 340.0])                # both far from everything else
    d["props"][0, 3] = torch.tensor([500.0, 5.0, 560.0, 45.0])
    d["deltas"][2:4] = 0
    got = gpu_select(d, 0.3, 0.0, 12, 12)
    reg = check_exact(d, got, 0.3, 0.0, 12, 12)
    ref = reg[0][2]
    assert float(got["max_conf"][0, 1]) == 0.0 and float(ref["max_conf"][1]) == 0.0 and float(ref["max_conf"][0]) > 0
    ids = got["keep_ids"][0].tolist()
    assert int(got["obj_ids"][0, ids.index(1)]) == 0 and float(got["obj_probs"][0, ids.index(1)]) == 0.0
    assert ids[:2] == [2, 3] and got["obj_ids"][0, :2].tolist() == [0, 0] and got["obj_probs"][0, :2].tolist() == [1.0, 1.0]


def test_kernel_zero_proposals():
    d = craft(2, 16, 5, seed=9, counts=[0, 0])
    got = gpu_select(d, 0.3, 0.2, 4, 8)
    check_exact(d, got, 0.3, 0.2, 4, 8)
    assert got["preds_per_image"].tolist() == [0, 0]


def test_kernel_attributes_are_the_rows_own():
    d = craft(2, 37, 5, seed=21)
    al = torch.randn((2 * 37, 9), generator=torch.Generator().manual_seed(4)) * 2
    got = gpu_select(d, 0.3, 0.2, 5, 20, attr_logits=al)
    ap, ai = PC.attrs_per_row(al)
    for n in range(2):
        k = int(got["preds_per_image"][n])
        ids = got["keep_ids"][n, :k] + n * 37
        np.testing.assert_array_equal(got["attr_ids"][n, :k].numpy(), ai[ids].numpy())
        assert G.rel_err(got["attr_probs"][n, :k], ap[ids]) <= 2e-6
        assert (got["attr_ids"][n, k:] == 0).all() and (got["attr_probs"][n, k:] == 0).all()


@pytest.mark.parametrize("Cn", [5, 1600])
def test_kernel_flags_a_nonfinite_box_of_an_unselected_class(Cn):
    """_clip_box runs on all R*C boxes (do_nms frcnn.py:121): a non-finite delta raises even in a class whose scores are so
    small that no box takes it as its confidence class."""
    d = craft(1, 37, Cn, seed=2)
    c = Cn - 1
    d["scores"][:, c] = 1e-30
    assert int(gpu_select(d, 0.3, 0.2, 5, 20)["flag"]) == 0
    d["deltas"][17, 4 * c + 1] = float("inf")
    assert int(gpu_select(d, 0.3, 0.2, 5, 20)["flag"]) == 1
    with pytest.raises(AssertionError, match="infinite or NaN"):
        PC.select_image(d["scores"], d["deltas"], d["props"][0], IMG_HW, WEIGHTS, 0.3, 0.2, 5, 20)
    d["deltas"][17, 4 * c + 1] = float("nan")
    assert int(gpu_select(d, 0.3, 0.2, 5, 20)["flag"]) == 1
    # a row beyond the image's count is not a box: its deltas are never decoded
    d["deltas"][17, 4 * c + 1] = 0.0
    d["deltas"][36, 0] = float("inf")
    d["counts"] = np.asarray([36], np.int32)
    assert int(gpu_select(d, 0.3, 0.2, 5, 20)["flag"]) == 0


def test_class_probs_against_softmax():
    x = torch.randn((67, 1601), generator=torch.Generator().manual_seed(8)) * 4
    xd = torch.zeros((67, 1608), device=G.DEV)
    xd[:, :1601] = x.to(G.DEV)
    out = torch.full((67, 1608), -7.0, device=G.DEV)
    L.call("vk_class_probs", G.P(xd), 1608, 67, 1601, G.P(out), 1608, G.stream())
    torch.cuda.synchronize()
    assert G.rel_err(out.cpu()[:, :1601], torch.softmax(x, -1)) <= 2e-6
    assert (out.cpu()[:, 1601:] == -7.0).all()
    # column of the arg-max over the classes == what vk_softmax_argmax reports, bit for bit
    prob = torch.zeros(67, device=G.DEV)
    cls = torch.zeros(67, dtype=torch.int32, device=G.DEV)
    L.call("vk_softmax_argmax", G.P(xd), 1608, 67, 1601, 1600, G.P(prob), G.P(cls), None, G.stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu()[torch.arange(67), cls.cpu().long()].numpy(), prob.cpu().numpy())


@pytest.mark.parametrize("agnostic", [False, True], ids=["per-class-deltas", "agnostic"])
def test_class_boxes_are_the_restatements(agnostic):
    """vk_class_boxes on crafted inputs (zero size deltas: exp(0) is exact) == class_boxes of the restatement, bit for bit;
    rows beyond an image's count are zero and a non-finite box raises the flag."""
    d = craft(2, 37, 5, seed=31, agnostic=agnostic, counts=[37, 20])
    dev = G.DEV
    dl, pr = d["deltas"].to(dev), d["props"].to(dev)
    cn, hw = torch.from_numpy(d["counts"]).to(dev), torch.from_numpy(d["hw"]).to(dev)
    out = torch.full((2 * 37, 5, 4), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (dl.shape[1], int(agnostic), G.P(pr), G.P(cn), 2, 37, 5, G.P(hw), (C.c_float * 4)(*WEIGHTS), G.P(out), G.P(flag), G.stream())
    L.call("vk_class_boxes", G.P(dl), *args)
    torch.cuda.synchronize()
    got = out.cpu()
    for n, c in enumerate(d["counts"]):
        rows = slice(n * 37, n * 37 + int(c))
        want = PC.class_boxes(d["deltas"][rows], d["props"][n, :c], IMG_HW, WEIGHTS, 5)
        np.testing.assert_array_equal(got[rows].numpy(), want.contiguous().numpy())
        assert (got[n * 37 + int(c):(n + 1) * 37] == 0).all()
    assert int(flag.cpu()) == 0
    dl[3, 1] = float("nan")
    L.call("vk_class_boxes", G.P(dl), *args)
    torch.cuda.synchronize()
    assert int(flag.cpu()) == 1


# ---- model level ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_per_class.npz"))


@pytest.fixture(scope="module")
def setup(golden):
    g = golden
    n, h, w = g["nhw"].tolist()
    cfg = vg_c4_config(depth=int(g["depth"]), post_nms_topk=int(g["post_topk"]), detections=int(g["max_detections"]))
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


def set_per_class(m, g, score):
    ro = m.roi_outputs
    ro.selection, ro.nms_thresh, ro.score_thresh = "per_class", [float(g["nms_thresh"])], score
    ro.min_detections, ro.max_detections = int(g["min_detections"]), int(g["max_detections"])


def device_class_boxes(m, bd, pb, pc, shapes):
    """vk_class_boxes over the forward's own box_deltas / proposal_boxes stages -> [N*R, C, 4] on the host."""
    cfg = m.config
    R, Cn = cfg.RPN.POST_NMS_TOPK_TEST, cfg.ROI_HEADS.NUM_CLASSES
    N = len(shapes)
    bdd, pbd, pcd = bd.contiguous(), pb.contiguous(), pc.to(torch.int32).contiguous()
    hw = torch.tensor(shapes, dtype=torch.int32, device=bdd.device)
    out = torch.full((N * R, Cn, 4), -7.0, device=bdd.device)
    flag = torch.zeros(1, dtype=torch.int32, device=bdd.device)
    L.call("vk_class_boxes", G.P(bdd), bdd.shape[1], int(bool(cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG)), G.P(pbd), G.P(pcd), N, R, Cn,
           G.P(hw), (C.c_float * 4)(*cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS), G.P(out), G.P(flag), G.stream())
    torch.cuda.synchronize()
    assert int(flag.cpu()) == 0
    return out.cpu()


def chain_check(m, out, shapes, scales=None):
    """The restatement fed the forward's own obj_scores, box_deltas (decoded by the device: see the module docstring),
    proposal_boxes, feature_pooled and attr_prob: every output exactly."""
    cfg, ro = m.config, m.roi_outputs
    R, Cn, An = cfg.RPN.POST_NMS_TOPK_TEST, cfg.ROI_HEADS.NUM_CLASSES, cfg.ROI_BOX_HEAD.NUM_ATTRS
    nb = 1 if cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG else Cn
    sc, bd = m.get_stage("obj_scores").cpu()[:, :Cn + 1], m.get_stage("box_deltas").cpu()[:, :4 * nb]
    pb, pc = m.get_stage("proposal_boxes").cpu(), m.get_stage("proposal_counts").cpu()
    feat, kid, conf = m.get_stage("feature_pooled").cpu(), m.get_stage("keep_ids").cpu(), m.get_stage("max_conf").cpu()
    dev_boxes = device_class_boxes(m, m.get_stage("box_deltas"), m.get_stage("proposal_boxes"), m.get_stage("proposal_counts"), shapes)
    dev_ap = m.get_stage("attr_prob").cpu()
    ap, ai = PC.attrs_per_row(m.get_stage("attr_logits").cpu()[:, :An + 1])
    worst = 0.0
    for i in range(len(shapes)):
        c = int(pc[i])
        rows = slice(i * R, i * R + c)
        ref = PC.select_image(sc[rows], bd[rows], pb[i, :c], shapes[i], cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS, ro.nms_thresh[0],
                              ro.score_thresh, ro.min_detections, ro.max_detections, None if scales is None else scales[i],
                              boxes=dev_boxes[rows])
        k = len(ref["ids"])
        assert int(out["preds_per_image"][i]) == k, (i, int(out["preds_per_image"][i]), k)
        np.testing.assert_array_equal(kid[i, :k].numpy(), ref["ids"].numpy())
        assert (kid[i, k:] == 0).all()
        np.testing.assert_array_equal(out["obj_ids"][i].cpu().numpy(), ref["classes"].numpy())
        np.testing.assert_array_equal(out["obj_probs"][i].cpu().numpy(), ref["probs"].numpy())
        np.testing.assert_array_equal(conf[i, :c].numpy(), ref["max_conf"].numpy())
        np.testing.assert_array_equal(out["boxes"][i].cpu().numpy(), ref["boxes"].numpy())
        np.testing.assert_array_equal(out["attr_ids"][i].cpu().numpy(), ai[rows][ref["ids"]].numpy())
        np.testing.assert_array_equal(out["attr_probs"][i].cpu().numpy(), dev_ap[rows][ref["ids"]].numpy())
        np.testing.assert_array_equal(out["roi_features"][i].cpu().numpy(), feat[rows][ref["ids"]].numpy())
        # the two device stages the chain starts from, against the host's arithmetic
        assert G.rel_err(dev_ap[rows], ap[rows]) <= 2e-6
        if c:
            e = G.rel_err(dev_boxes[rows], PC.class_boxes(bd[rows], pb[i, :c], shapes[i], cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS, Cn))
            worst = max(worst, e)
            assert e <= 2e-6, (i, e)
        assert (dev_boxes[i * R + c:(i + 1) * R] == 0).all()
    print(f"[per_class stage chain] every output exact; device R*C boxes vs host decode rel err {worst:.2e}")
    return pb, pc


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_stage_chained(golden, setup, models, precision):
    _, _, x, shapes = setup
    m = models[precision]
    for score in golden["score_thresh"].tolist():
        set_per_class(m, golden, score)
        out = m(x, torch.tensor(shapes))
        chain_check(m, out, shapes)
    sc = torch.from_numpy(golden["scales_yx"])
    set_per_class(m, golden, 0.4)
    out = m(x, torch.tensor(shapes), scales_yx=sc)
    chain_check(m, out, shapes, scales=sc)
    Cn = m.config.ROI_HEADS.NUM_CLASSES
    logits = m.get_stage("obj_logits").cpu()[:, :Cn + 1]
    e = G.rel_err(m.get_stage("obj_scores").cpu()[:, :Cn + 1], torch.softmax(logits, -1))
    print(f"[per_class {precision}] obj_scores vs softmax(obj_logits) rel err {e:.2e}")
    assert e <= 2e-6
    with pytest.raises(ValueError, match="chosen_deltas"):
        m.get_stage("chosen_deltas")                            # the arg-max class's rows alone are not computed in this mode


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales_yx"])
def test_strict_fp32_against_the_fixture(golden, setup, models, scaled):
    """Identical ids, classes and counts at all four thresholds; values at test_gpu_e2e.py's 1e-3."""
    g = golden
    _, _, x, shapes = setup
    m = models["fp32"]
    sc = torch.from_numpy(g["scales_yx"]) if scaled else None
    for ti, score in enumerate(g["score_thresh"].tolist()):
        set_per_class(m, g, score)
        out = m(x, torch.tensor(shapes), scales_yx=sc)
        kid = m.get_stage("keep_ids").cpu()
        np.testing.assert_array_equal(out["preds_per_image"].numpy(), g["counts"][ti])
        for i in range(len(shapes)):
            k = int(g["counts"][ti][i])
            assert int(m.get_stage("proposal_counts")[i]) == len(g[f"proposal_boxes_{i}"])
            pb = m.get_stage("proposal_boxes").cpu()[i, :len(g[f"proposal_boxes_{i}"])]
            assert G.rel_err(pb, g[f"proposal_boxes_{i}"]) <= 1e-3
            np.testing.assert_array_equal(kid[i, :k].numpy(), g[f"keep_ids_{i}"][:k])
            np.testing.assert_array_equal(out["obj_ids"][i].cpu().numpy(), g[f"obj_ids_{i}"][:k])
            np.testing.assert_array_equal(out["attr_ids"][i].cpu().numpy(), g[f"attr_ids_{i}"][:k])
            for key in ("roi_features", "boxes", "obj_probs", "attr_probs"):
                want = g["boxes_scaled_%d" % i if key == "boxes" and scaled else f"{key}_{i}"][:k]
                e = G.rel_err(out[key][i].cpu(), want)
                assert e <= 1e-3, (score, i, key, e)
    deltas = m.get_stage("box_deltas").cpu()
    R = m.config.RPN.POST_NMS_TOPK_TEST
    for i in range(len(shapes)):
        c = len(g[f"deltas_rowsum_{i}"])
        cols = torch.from_numpy(g[f"class_cols_{i}"])
        rows = deltas[i * R:i * R + c, :4 * m.config.ROI_HEADS.NUM_CLASSES]
        assert G.rel_err(rows.view(c, -1, 4)[:, cols].reshape(c, -1), g[f"deltas_cols_{i}"]) <= 1e-3
        assert G.rel_err(rows.double().sum(1).float(), g[f"deltas_rowsum_{i}"]) <= 1e-3


def _raw(m, x, hw, **kw):
    blk = m.forward_async(x, hw, **kw).wait_raw()
    return {k: blk[k].clone() for k in blk}


def test_default_mode_is_untouched(golden, setup):
    """selection = "class_max": the outputs and the kernel_timing() launch counts of a forward equal those of a model whose
    roi_outputs never had the attribute; a class-max forward after a per-class one gives bit-identical outputs."""
    cfg, sd, x, shapes = setup
    hw = torch.tensor(shapes)
    old = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    del old.roi_outputs.selection
    new = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    assert new.roi_outputs.selection == "class_max"
    for m in (old, new):
        m.roi_outputs.nms_thresh, m.roi_outputs.score_thresh = [0.5, 1.0, 0.1], 0.2       # tests/frcnn_test.py:16-19
        m.enable_kernel_timing(True)
    a, b = _raw(old, x, hw), _raw(new, x, hw)
    ta, tb = old.kernel_timing(reset=True), new.kernel_timing(reset=True)
    assert {k: v["launches"] for k, v in ta.items()} == {k: v["launches"] for k, v in tb.items()}
    assert sum(v["launches"] for v in ta.values()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    saved = (new.roi_outputs.nms_thresh, new.roi_outputs.min_detections, new.roi_outputs.max_detections)
    set_per_class(new, golden, 0.4)
    pc = _raw(new, x, hw)
    assert not torch.equal(pc["obj_probs"], b["obj_probs"])
    new.roi_outputs.selection = "class_max"
    new.roi_outputs.nms_thresh, new.roi_outputs.min_detections, new.roi_outputs.max_detections = saved
    new.kernel_timing(reset=True)
    again = _raw(new, x, hw)
    assert {k: v["launches"] for k, v in new.kernel_timing().items()} == {k: v["launches"] for k, v in ta.items()}
    for k in a:
        assert torch.equal(a[k], again[k]), k
    assert new.get_stage("chosen_deltas").shape[1] == 4          # the class-max stages are back


def test_ignorey_composes_with_per_class(golden, setup, models):
    """ignorey acts on the proposals, before the selection: the forward equals the restatement on the filtered proposals."""
    _, _, x, shapes = setup
    m = models["fp32"]
    hw, sc = torch.tensor(shapes), torch.from_numpy(golden["scales_yx"])
    set_per_class(m, golden, 0.4)
    out0 = m(x, hw, scales_yx=sc)
    pb0, pc0 = chain_check(m, out0, shapes, scales=sc)
    # image 0: a band inside proposal 0 removes it; image 1: a band across the top of proposal 1 trims or removes boxes there
    b0, b1 = pb0[0, 0], pb0[1, 1]
    ig = [[[(float(b0[1]) + 3.3) * float(sc[0, 1]), (float(b0[3]) - 3.3) * float(sc[0, 1])]],
          [[(float(b1[1]) - 2.3) * float(sc[1, 1]), (float(b1[1]) + 4.6) * float(sc[1, 1])]]]
    out = m(x, hw, scales_yx=sc, ignorey=ig)
    pb, pc = chain_check(m, out, shapes, scales=sc)
    for i in range(2):
        c0, c = int(pc0[i]), int(pc[i])
        assert c != c0 or not torch.equal(pb[i, :c], pb0[i, :c0]), f"image {i}: the band changed no proposal"


def test_per_class_raises_on_a_nonfinite_box(golden, setup, models):
    """The reference's AssertionError through the non-finite flag and vk_forward_end: NaN pixels poison every box."""
    _, _, x, shapes = setup
    m = models["fp32"]
    set_per_class(m, golden, 0.4)
    bad = x.clone()
    bad[0, 0, 8, 8] = float("nan")
    with pytest.raises(AssertionError, match="infinite or NaN"):
        m(bad, torch.tensor(shapes))
    out = m(x, torch.tensor(shapes))                            # and the model is usable afterwards
    chain_check(m, out, shapes)


@pytest.mark.parametrize("overrides", [(("roi_heads", "num_classes", 5),), (("roi_box_head", "cls_agnostic_bbox_reg", True),)],
                         ids=["C5", "agnostic"])
def test_model_with_a_padded_bbox_pred(golden, setup, overrides):
    """bbox_pred with 4C = 20 rows, and the class-agnostic head's 4: neither is a whole tile of the linear path, so the first
    per-class forward makes the zero-padded copy of the weights.  Stage-chained like the 1600-class model, both precisions,
    twice (the second forward reuses the copy)."""
    _, _, x, shapes = setup
    cfg = vg_c4_config(overrides=overrides, depth=int(golden["depth"]), post_nms_topk=int(golden["post_topk"]),
                       detections=int(golden["max_detections"]))
    sd = make_state_dict(cfg, seed=int(golden["weights_seed"]), calibrated=False)      # the calibration file is the 1600-class head's
    for precision in ("fp32", "fp16"):
        m = FRCNN(cfg, precision=precision).load_state_dict(sd).eval()
        for score in (0.4, 0.05):
            set_per_class(m, golden, score)
            out = m(x, torch.tensor(shapes))
            chain_check(m, out, shapes)
            assert int(out["preds_per_image"].min()) >= min(int(golden["min_detections"]), int(m.get_stage("proposal_counts").min()))
        nb = 1 if cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG else cfg.ROI_HEADS.NUM_CLASSES
        bd = m.get_stage("box_deltas").cpu()
        assert bd.shape[1] >= 4 * nb and float(bd[:, :4 * nb].abs().max()) > 0
        # the all-class deltas are the class-max mode's chosen rows: the same weights through the other path
        m.roi_outputs.selection, m.roi_outputs.nms_thresh = "class_max", [0.3]
        m(x, torch.tensor(shapes))
        chosen = m.get_stage("chosen_deltas").cpu()
        logits = m.get_stage("obj_logits").cpu()[:, :cfg.ROI_HEADS.NUM_CLASSES]
        arg = logits.argmax(1) if nb > 1 else torch.zeros(len(logits), dtype=torch.int64)
        want = bd[:, :4 * nb].view(len(bd), nb, 4)[torch.arange(len(bd)), arg]
        pc = m.get_stage("proposal_counts").cpu()
        R = cfg.RPN.POST_NMS_TOPK_TEST
        for i in range(len(shapes)):
            rows = slice(i * R, i * R + int(pc[i]))
            e = G.rel_err(want[rows], chosen[rows])
            print(f"[per_class {precision} {'agnostic' if nb == 1 else 'C5'}] box_deltas vs chosen_deltas rel err {e:.2e}")
            assert e <= 1e-3
