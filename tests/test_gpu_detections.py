"""-m gpu: roi_outputs.selection = "detections" on the GPU (vltk_amd/csrc/detections.hip).

Kernel level: vk_detections_select against the tests' restatement of the contract (tests/detections_util.py) on the crafted
inputs of test_gpu_per_class.py, everything bit for bit.  The crafted size deltas are zero: exp(0) is exact on both sides, so
every decoded box -- and with it every IoU and every suppression -- is the same IEEE arithmetic on the device and on the
host.  The restatement runs NMS over all rows of a class and filters afterwards; the device sweeps the candidates alone.
Model level: the restatement fed the forward's own stages (the device's R*C boxes and per-row attribute probabilities, as in
test_gpu_per_class.py), both precisions; the relation to the per-class fixture that test_detections_host.py holds the
restatement to; the two other selections untouched; ignorey composed with the mode; the non-finite assertion."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import FRCNN                             # noqa: E402
from vltk_amd import _lib as L                         # noqa: E402

import detections_util as DT                           # noqa: E402
import gpu_util as G                                   # noqa: E402
import per_class_util as PC                            # noqa: E402
import test_detections_host as TH                      # noqa: E402
import test_gpu_per_class as TP                        # noqa: E402

WEIGHTS, IMG_HW, craft = TP.WEIGHTS, TP.IMG_HW, TP.craft
golden, setup, models = TP.golden, TP.setup, TP.models          # the small fixture model of test_gpu_per_class.py
OUT_KEYS = ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "preds_per_image", "roi_features")


def lds_keys():
    return int(L.load().vk_detections_lds_keys())


# ---- kernel level ---------------------------------------------------------------------------------------------------
def gpu_select(d, t, score, D, scales=None, attr_logits=None):
    N, R, Cn, F = d["N"], d["R"], d["C"], d["feats"].shape[1]
    dev = G.DEV
    sc, dl, pr, ft = (d[k].to(dev) for k in ("scores", "deltas", "props", "feats"))
    cn, hw = torch.from_numpy(d["counts"]).to(dev), torch.from_numpy(d["hw"]).to(dev)
    scd = torch.as_tensor(scales, dtype=torch.float32).to(dev) if scales is not None else None
    al = attr_logits.to(dev) if attr_logits is not None else None
    o = dict(obj_ids=torch.full((N, D), -7, dtype=torch.int64, device=dev), obj_probs=torch.full((N, D), -7.0, device=dev),
             attr_ids=torch.full((N, D), -7, dtype=torch.int64, device=dev), attr_probs=torch.full((N, D), -7.0, device=dev),
             boxes=torch.full((N, D, 4), -7.0, device=dev), preds_per_image=torch.full((N,), -7, dtype=torch.int64, device=dev),
             roi_features=torch.full((N, D, F), -7.0, device=dev))
    keep = torch.full((N, D), -7, dtype=torch.int64, device=dev)
    nsurv = torch.full((N,), -7, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = L.vk_outputs(*[o[k].data_ptr() for k in OUT_KEYS])
    sp = L.vk_select_params()
    sp.mode, sp.score_thresh = L.VK_SELECT_DETECTIONS, score
    sp.roi.num_nms_thresh, sp.roi.min_detections, sp.roi.max_detections = 1, 0, D
    sp.roi.nms_thresh[0] = t
    w = (C.c_float * 4)(*WEIGHTS)
    L.call("vk_detections_select", G.P(sc), sc.shape[1], G.P(al), al.shape[1] if al is not None else 0, G.P(dl), dl.shape[1],
           int(d["agnostic"]), G.P(pr), G.P(cn), G.P(ft), F, N, R, Cn, al.shape[1] - 1 if al is not None else 0, G.P(hw), G.P(scd), w,
           C.byref(sp), C.byref(out), G.P(keep), G.P(nsurv), G.P(flag), G.stream())
    torch.cuda.synchronize()                        # the call itself does not synchronise
    res = {k: v.cpu() for k, v in o.items()}
    res.update(keep_ids=keep.cpu(), n_survivors=nsurv.cpu(), flag=int(flag.cpu()))
    return res


def restate(d, t, score, D, scales=None):
    N, R = d["N"], d["R"]
    refs = []
    for n in range(N):
        c = int(d["counts"][n])
        rows = slice(n * R, n * R + c)
        refs.append(DT.select_image(d["scores"][rows], d["deltas"][rows], d["props"][n, :c], d["hw"][n], WEIGHTS, t, score, D,
                                    None if scales is None else scales[n]))
    return refs


def check_exact(d, got, refs, D):
    """Every output of the device call against the restatement, bit for bit.  `refs` may come from a larger max_detections:
    the first D of a ranking are the ranking at D."""
    R = d["R"]
    for n, ref in enumerate(refs):
        k = min(len(ref["ids"]), D)
        rows = slice(n * R, n * R + int(d["counts"][n]))
        assert int(got["n_survivors"][n]) == ref["n_survivors"], (n, int(got["n_survivors"][n]), ref["n_survivors"])
        assert int(got["preds_per_image"][n]) == k == min(ref["n_survivors"], D), (n, int(got["preds_per_image"][n]), k)
        np.testing.assert_array_equal(got["keep_ids"][n, :k].numpy(), ref["ids"][:k].numpy())
        np.testing.assert_array_equal(got["obj_ids"][n, :k].numpy(), ref["classes"][:k].numpy())
        np.testing.assert_array_equal(got["obj_probs"][n, :k].numpy(), ref["probs"][:k].numpy())
        np.testing.assert_array_equal(got["boxes"][n, :k].numpy(), ref["boxes"][:k].numpy())
        np.testing.assert_array_equal(got["roi_features"][n, :k].numpy(), d["feats"][rows][ref["ids"][:k]].numpy())
        for key in ("keep_ids", "obj_ids", "obj_probs", "boxes", "roi_features", "attr_ids", "attr_probs"):
            assert (got[key][n, k:] == 0).all(), (key, n)       # rows beyond preds_per_image are zero
    assert got["flag"] == 0


CASES = [   # N, R, C, keyword arguments of craft, max_detections
    (1, 1, 5, {}, 3), (3, 37, 5, dict(counts=[37, 0, 11]), 20), (1, 1024, 5, {}, 20), (2, 300, 1600, dict(counts=[123, 300]), 100),
    (2, 37, 5, dict(agnostic=True), 20), (2, 37, 5, dict(ties=True), 20), (1, 300, 5, dict(ties=True), 100),
    (1, 2, 5, {}, 3), (2, 64, 5, {}, 20), (2, 65, 5, {}, 20),      # the rows of test_gpu_per_class.py's CASES at the shared code's edges
]


@pytest.mark.parametrize("N,R,Cn,kw,D", CASES, ids=[f"N{n}-R{r}-C{c}" + "".join(f"-{k}" for k in kw) for n, r, c, kw, _ in CASES])
def test_kernel_matches_restatement(N, R, Cn, kw, D):
    d = craft(N, R, Cn, seed=R * 7 + Cn + N, **kw)
    check_exact(d, gpu_select(d, 0.3, 0.2, D), restate(d, 0.3, 0.2, D), D)
    scales = [[1.25, 1.5], [2.0, 1.75], [0.5, 0.75]][:N]
    refs = restate(d, 0.5, 0.05, D, scales=scales)
    check_exact(d, gpu_select(d, 0.5, 0.05, D, scales=scales), refs, D)
    assert max(r["n_survivors"] for r in refs) <= lds_keys()     # the in-LDS sort


def test_kernel_survivor_counts_around_max_detections():
    """#survivors = 0 (threshold 1.0), 1, D - 1, D, D + 1."""
    d = craft(2, 37, 5, seed=11)
    got = gpu_select(d, 0.3, 1.0, 20)
    check_exact(d, got, restate(d, 0.3, 1.0, 20), 20)
    assert got["preds_per_image"].tolist() == [0, 0] and got["n_survivors"].tolist() == [0, 0]
    top = np.sort(d["scores"][:37, :5].numpy().ravel())[::-1]
    assert top[0] > top[1]
    one = (float(top[0]) + float(top[1])) / 2                    # only image 0's best pair is above it
    refs = restate(d, 0.3, one, 20)
    assert refs[0]["n_survivors"] == 1
    check_exact(d, gpu_select(d, 0.3, one, 20), refs, 20)
    refs = restate(d, 0.3, 0.05, 1024)
    ns = refs[0]["n_survivors"]
    assert 3 <= ns <= 1023
    for D in (ns + 1, ns, ns - 1):
        got = gpu_select(d, 0.3, 0.05, D)
        check_exact(d, got, refs, D)
        assert int(got["preds_per_image"][0]) == min(ns, D)


def test_kernel_radix_path_above_the_lds_capacity():
    """More survivors in an image than the final kernel sorts in LDS.  At an NMS threshold of 1.0 nothing is suppressed
    (an IoU is never above 1), so every positive score of 1024 x 5 survives: 5120 keys, cut at 1, 100 and 1024; and the general
    case, 300 x 1600 at a zero threshold, with exact ties and duplicate boxes."""
    cap = lds_keys()
    d = craft(1, 1024, 5, seed=3)
    refs = restate(d, 1.0, 0.0, 1024)
    assert refs[0]["n_survivors"] > cap, (refs[0]["n_survivors"], cap)
    for D in (1, 100, 1024):
        check_exact(d, gpu_select(d, 1.0, 0.0, D), refs, D)
    d = craft(1, 300, 1600, seed=4, ties=True)
    refs = restate(d, 0.3, 0.0, 1024)
    assert refs[0]["n_survivors"] > cap, (refs[0]["n_survivors"], cap)
    a = gpu_select(d, 0.3, 0.0, 1024)
    check_exact(d, a, refs, 1024)
    b = gpu_select(d, 0.3, 0.0, 1024)                            # run to run: identical bytes
    for k in a:
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k


def test_kernel_max_detections_above_R():
    d = craft(1, 37, 5, seed=17)
    refs = restate(d, 0.3, 0.0, 100)
    got = gpu_select(d, 0.3, 0.0, 100)
    check_exact(d, got, refs, 100)
    k = int(got["preds_per_image"][0])
    assert 37 < k <= 100, k                                      # more outputs than proposals: some come out under several classes
    assert len(set(got["keep_ids"][0, :k].tolist())) < k


def test_kernel_tie_rules():
    """Equal scores across rows of one class, across classes of one row, and duplicate boxes pin the key order: score, then
    the lower row, then the lower class."""
    d = craft(1, 12, 5, seed=5)
    d["props"][0, 1] = d["props"][0, 0]                          # row 1 duplicates row 0: suppressed in every class
    d["deltas"][1] = d["deltas"][0]
    d["scores"][1] = d["scores"][0]
    d["scores"][2, :5] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0])  # the image's best score in classes 0 and 2 of a row ...
    d["scores"][3] = d["scores"][2]                               # ... and on two rows
    d["props"][0, 2] = torch.tensor([5.0, 300.0, 45.0, 340.0])    # both far from everything else
    d["props"][0, 3] = torch.tensor([500.0, 5.0, 560.0, 45.0])
    d["deltas"][2:4] = 0
    refs = restate(d, 0.3, 0.0, 60)
    got = gpu_select(d, 0.3, 0.0, 60)
    check_exact(d, got, refs, 60)
    k = int(got["preds_per_image"][0])
    pairs = list(zip(got["keep_ids"][0, :k].tolist(), got["obj_ids"][0, :k].tolist()))
    assert pairs[:4] == [(2, 0), (2, 2), (3, 0), (3, 2)], pairs[:4]
    assert 1 not in got["keep_ids"][0, :k].tolist() and 0 in got["keep_ids"][0, :k].tolist()
    assert (got["obj_probs"][0, :k] > 0).all()                   # a zero score is never a candidate, even at threshold 0


def test_kernel_zero_proposals_and_attributes():
    d = craft(2, 16, 5, seed=9, counts=[0, 0])
    got = gpu_select(d, 0.3, 0.0, 8)
    check_exact(d, got, restate(d, 0.3, 0.0, 8), 8)
    assert got["preds_per_image"].tolist() == [0, 0]
    d = craft(2, 37, 5, seed=21)
    al = torch.randn((2 * 37, 9), generator=torch.Generator().manual_seed(4)) * 2
    got = gpu_select(d, 0.3, 0.1, 50, attr_logits=al)
    ap, ai = PC.attrs_per_row(al)
    for n in range(2):
        k = int(got["preds_per_image"][n])
        assert k > 0
        ids = got["keep_ids"][n, :k] + n * 37
        np.testing.assert_array_equal(got["attr_ids"][n, :k].numpy(), ai[ids].numpy())
        assert G.rel_err(got["attr_probs"][n, :k], ap[ids]) <= 2e-6
        assert (got["attr_ids"][n, k:] == 0).all() and (got["attr_probs"][n, k:] == 0).all()


@pytest.mark.parametrize("Cn", [5, 1600])
def test_kernel_flags_a_nonfinite_box_that_is_no_candidate(Cn):
    """_clip_box runs on all R*C boxes (do_nms frcnn.py:121): a non-finite delta raises even in a pair far below the threshold."""
    d = craft(1, 37, Cn, seed=2)
    c = Cn - 1
    d["scores"][:, c] = 1e-30
    assert int(gpu_select(d, 0.3, 0.05, 20)["flag"]) == 0
    d["deltas"][17, 4 * c + 1] = float("inf")
    assert int(gpu_select(d, 0.3, 0.05, 20)["flag"]) == 1
    with pytest.raises(AssertionError, match="infinite or NaN"):
        DT.select_image(d["scores"], d["deltas"], d["props"][0], IMG_HW, WEIGHTS, 0.3, 0.05, 20)
    d["deltas"][17, 4 * c + 1] = float("nan")
    assert int(gpu_select(d, 0.3, 0.05, 20)["flag"]) == 1
    d["deltas"][17, 4 * c + 1] = 0.0                             # a row beyond the image's count is not a box
    d["deltas"][36, 0] = float("inf")
    d["counts"] = np.asarray([36], np.int32)
    assert int(gpu_select(d, 0.3, 0.05, 20)["flag"]) == 0


def test_kernel_run_to_run_and_cross_mode_invariant():
    """The same call twice gives identical bytes.  At a zero threshold with strictly positive scores and D >= #survivors, a
    row's best detection is what the per-class mode reports as its (max_conf, cls): (score bits, class), every row."""
    d = craft(2, 37, 5, seed=23)
    assert (d["scores"][:, :5] > 0).all()
    a, b = gpu_select(d, 0.3, 0.0, 1024), gpu_select(d, 0.3, 0.0, 1024)
    for k in a:
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
    pc = TP.gpu_select(d, 0.3, 0.0, 37, 37)                      # every row comes out: its class and confidence
    for n in range(2):
        k = int(a["preds_per_image"][n])
        assert k == int(a["n_survivors"][n]) <= 1024
        best = {}
        for r, c, p in zip(a["keep_ids"][n, :k].tolist(), a["obj_ids"][n, :k].tolist(), a["obj_probs"][n, :k].numpy()):
            best.setdefault(r, (c, p.tobytes()))
        assert int(pc["preds_per_image"][n]) == 37
        for r, c, p in zip(pc["keep_ids"][n].tolist(), pc["obj_ids"][n].tolist(), pc["obj_probs"][n].numpy()):
            if r in best:
                assert best[r] == (c, p.tobytes()), (n, r)
            else:
                assert float(p) == 0.0 and c == 0, (n, r)        # survives in no class
        np.testing.assert_array_equal(pc["max_conf"][n].numpy()[sorted(best)], np.asarray(
            [np.frombuffer(best[r][1], np.float32)[0] for r in sorted(best)]))


# ---- model level ----------------------------------------------------------------------------------------------------
def set_detections(m, g, score, D):
    ro = m.roi_outputs
    ro.selection, ro.nms_thresh, ro.score_thresh = "detections", [float(g["nms_thresh"])], score
    ro.min_detections, ro.max_detections = 0, D


def chain_check(m, out, shapes, scales=None):
    """The restatement fed the forward's own obj_scores, the device's R*C boxes, proposal_boxes, feature_pooled and attr_prob:
    every output exactly.  -> (proposal boxes, counts, per image n_survivors)."""
    cfg, ro = m.config, m.roi_outputs
    R, Cn, An = cfg.RPN.POST_NMS_TOPK_TEST, cfg.ROI_HEADS.NUM_CLASSES, cfg.ROI_BOX_HEAD.NUM_ATTRS
    nb = 1 if cfg.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG else Cn
    sc, bd = m.get_stage("obj_scores").cpu()[:, :Cn + 1], m.get_stage("box_deltas").cpu()[:, :4 * nb]
    pb, pc = m.get_stage("proposal_boxes").cpu(), m.get_stage("proposal_counts").cpu()
    feat, kid, ns = m.get_stage("feature_pooled").cpu(), m.get_stage("keep_ids").cpu(), m.get_stage("n_survivors").cpu()
    assert kid.shape == (len(shapes), ro.max_detections)
    dev_boxes = TP.device_class_boxes(m, m.get_stage("box_deltas"), m.get_stage("proposal_boxes"), m.get_stage("proposal_counts"), shapes)
    dev_ap = m.get_stage("attr_prob").cpu()
    _, ai = PC.attrs_per_row(m.get_stage("attr_logits").cpu()[:, :An + 1])
    for i in range(len(shapes)):
        c = int(pc[i])
        rows = slice(i * R, i * R + c)
        ref = DT.select_image(sc[rows], bd[rows], pb[i, :c], shapes[i], cfg.ROI_BOX_HEAD.BBOX_REG_WEIGHTS, ro.nms_thresh[0],
                              ro.score_thresh, ro.max_detections, None if scales is None else scales[i], boxes=dev_boxes[rows])
        k = len(ref["ids"])
        assert int(out["preds_per_image"][i]) == k and int(ns[i]) == ref["n_survivors"], (i, int(out["preds_per_image"][i]), k)
        np.testing.assert_array_equal(kid[i, :k].numpy(), ref["ids"].numpy())
        assert (kid[i, k:] == 0).all()
        np.testing.assert_array_equal(out["obj_ids"][i].cpu().numpy(), ref["classes"].numpy())
        np.testing.assert_array_equal(out["obj_probs"][i].cpu().numpy(), ref["probs"].numpy())
        np.testing.assert_array_equal(out["boxes"][i].cpu().numpy(), ref["boxes"].numpy())
        np.testing.assert_array_equal(out["attr_ids"][i].cpu().numpy(), ai[rows][ref["ids"]].numpy())
        np.testing.assert_array_equal(out["attr_probs"][i].cpu().numpy(), dev_ap[rows][ref["ids"]].numpy())
        np.testing.assert_array_equal(out["roi_features"][i].cpu().numpy(), feat[rows][ref["ids"]].numpy())
    return pb, pc, ns.tolist()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_stage_chained(golden, setup, models, precision):
    _, _, x, shapes = setup
    m = models[precision]
    R = m.config.RPN.POST_NMS_TOPK_TEST
    seen = []
    for score, D in ((0.05, 16), (0.2, 100), (0.0, 1024), (1.0, 16)):
        set_detections(m, golden, score, D)
        out = m(x, torch.tensor(shapes))
        ns = chain_check(m, out, shapes)[2]
        seen.append((D, ns))
    assert seen[3][1] == [0, 0]                                  # nothing is above 1.0: an empty image is a valid answer
    assert max(seen[0][1]) > 16 and max(seen[1][1]) < 100 and max(seen[2][1]) > max(R, 1024)     # cut, not cut, cut above R
    sc = torch.from_numpy(golden["scales_yx"])
    set_detections(m, golden, 0.05, 100)
    out = m(x, torch.tensor(shapes), scales_yx=sc)
    chain_check(m, out, shapes, scales=sc)
    assert int(out["preds_per_image"].max()) > R                 # more outputs than proposals
    for stage in ("chosen_deltas", "max_conf"):                  # the other modes' stages are not produced
        with pytest.raises(ValueError, match=stage):
            m.get_stage(stage)


def test_strict_fp32_against_the_fixture(golden, setup, models):
    """What the per-class fixture (the reference's own methods) pins of this mode, at test_gpu_e2e.py's 1e-3."""
    g = golden
    _, _, x, shapes = setup
    m = models["fp32"]
    for score in g["score_thresh"].tolist():
        set_detections(m, g, score, 1024)
        out = m(x, torch.tensor(shapes))
        kid = m.get_stage("keep_ids").cpu()
        for i in range(len(shapes)):
            k = int(out["preds_per_image"][i])
            res = dict(ids=kid[i, :k].numpy(), classes=out["obj_ids"][i].cpu().numpy(), probs=out["obj_probs"][i].cpu().numpy(),
                       boxes=out["boxes"][i].cpu().numpy())
            TH.fixture_relation(g, i, score, res, lambda c: c)


def _raw(m, x, hw, **kw):
    blk = m.forward_async(x, hw, **kw).wait_raw()
    return {k: blk[k].clone() for k in blk}


def _launches(m):
    return {k: v["launches"] for k, v in m.kernel_timing(reset=True).items()}


def test_other_modes_are_untouched_by_the_mode(golden, setup):
    """With the new code present, class_max and per_class forwards on a handle that has run the detections mode give the
    outputs and the kernel_timing() launch counts they gave before the mode was ever used on it."""
    cfg, sd, x, shapes = setup
    hw = torch.tensor(shapes)
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    m.enable_kernel_timing(True)
    ro = m.roi_outputs
    class_max = dict(selection="class_max", nms_thresh=[0.5, 1.0, 0.1], score_thresh=0.2, min_detections=ro.min_detections,
                     max_detections=ro.max_detections)
    per_class = dict(selection="per_class", nms_thresh=[float(golden["nms_thresh"])], score_thresh=0.4,
                     min_detections=int(golden["min_detections"]), max_detections=int(golden["max_detections"]))

    def run(knobs):
        for k, v in knobs.items():
            setattr(ro, k, v)
        m.kernel_timing(reset=True)
        out = _raw(m, x, hw)
        return out, _launches(m)
    before = [run(class_max), run(per_class)]
    assert sum(before[0][1].values()) > 0
    set_detections(m, golden, 0.05, 100)
    det = _raw(m, x, hw)
    assert int(det["preds_per_image"].max()) > 0
    after = [run(class_max), run(per_class)]
    for (a, la), (b, lb) in zip(before, after):
        assert la == lb
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert m.get_stage("max_conf").shape == (len(shapes), cfg.RPN.POST_NMS_TOPK_TEST)      # the per-class stages are back


def test_ignorey_composes_with_detections(golden, setup, models):
    """ignorey acts on the proposals, before the selection: the forward equals the restatement on the filtered proposals."""
    _, _, x, shapes = setup
    m = models["fp32"]
    hw, sc = torch.tensor(shapes), torch.from_numpy(golden["scales_yx"])
    set_detections(m, golden, 0.2, 100)
    out0 = m(x, hw, scales_yx=sc)
    pb0, pc0, _ = chain_check(m, out0, shapes, scales=sc)
    b0, b1 = pb0[0, 0], pb0[1, 1]
    ig = [[[(float(b0[1]) + 3.3) * float(sc[0, 1]), (float(b0[3]) - 3.3) * float(sc[0, 1])]],
          [[(float(b1[1]) - 2.3) * float(sc[1, 1]), (float(b1[1]) + 4.6) * float(sc[1, 1])]]]
    out = m(x, hw, scales_yx=sc, ignorey=ig)
    pb, pc, _ = chain_check(m, out, shapes, scales=sc)
    for i in range(2):
        c0, c = int(pc0[i]), int(pc[i])
        assert c != c0 or not torch.equal(pb[i, :c], pb0[i, :c0]), f"image {i}: the band changed no proposal"


def test_detections_raises_on_a_nonfinite_box(golden, setup, models):
    """The reference's AssertionError through the non-finite flag and vk_forward_end: NaN pixels poison every box."""
    _, _, x, shapes = setup
    m = models["fp32"]
    set_detections(m, golden, 0.2, 100)
    bad = x.clone()
    bad[0, 0, 8, 8] = float("nan")
    with pytest.raises(AssertionError, match="infinite or NaN"):
        m(bad, torch.tensor(shapes))
    out = m(x, torch.tensor(shapes))                            # and the model is usable afterwards
    chain_check(m, out, shapes)
