"""-m gpu: the RoIAlign box pooler of the C4 model (ROI_BOX_HEAD.POOLER_TYPE) -- the handle path at the model level, and
vk_roi_align on one level at the C4 head's shape (C = 1024, P = 14).  The rule is torchvision's / detectron2's (the reference holds only RoIPool): PARITY
UNPINNED, held to oracle/fpn_oracle.py::roi_align exactly as tests/test_gpu_fpn.py holds the pyramid kernel.

Stage level: the exact set (roi_align_c4_util: dyadic data on which every summation order gives the oracle's bits) bit for
bit against the oracle.  Model level: the e2e_r101_small fixture model through stage_chain_check with
AlignOracle (fp32 1e-4; fp16 1e-3 against the fp16-emulating oracle, the chain's own tolerances)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fpn_oracle as fo                     # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                          # noqa: E402

import gpu_util as G                                    # noqa: E402
import roi_align_c4_util as U                           # noqa: E402
from test_gpu_e2e import nchw, stage_chain_check        # noqa: E402

TD = {L.VK_F32: torch.float32, L.VK_F16: torch.float16}


def nhwc(x, td):
    return x.permute(0, 2, 3, 1).contiguous().to(td).to(G.DEV)


# ---- stage level: the kernel the handle pools through, at the C4 head's shape ---------------------------------------------
_EXACT = {}


def exact_reference(sr):
    """(map [N,1024,H,W] f32, rois [K,5], the oracle's [K,1024,P,P]) of the exact set, computed once per sampling ratio."""
    if sr not in _EXACT:
        x, rois = U.exact_map(1024), U.exact_rois()
        _EXACT[sr] = (x, rois, fo.roi_align(x, rois, U.EXACT_P, U.EXACT_SCALE, sr, True))
    return _EXACT[sr]


@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["fp32", "fp16"])
def test_exact_set_one_level_c1024_bit_identical_to_oracle(dt, sr):
    """vk_roi_align on one level with C = 1024, P = 14 (two bins in flight per workgroup: the shape the C4 handle gives it,
    which the FPN tests never do) on the exact set: the oracle's bits, in fp16 the oracle's fp32 result rounded once."""
    x, rois, ref = exact_reference(sr)
    out = U.align_pyramid_one_level(L, nhwc(x, TD[dt]), torch.from_numpy(rois).to(G.DEV), U.EXACT_P, U.EXACT_SCALE, sr, True, dt)
    expect = ref.to(TD[dt]) if dt == L.VK_F16 else ref
    got = out.permute(0, 3, 1, 2).cpu()
    bad = (got != expect).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"RoIs {bad} differ from the oracle"


# ---- model level ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(golden_dir):
    g = np.load(os.path.join(golden_dir, "e2e_r101_small.npz"))
    n, h, w = g["nhw"].tolist()
    kw = dict(depth=int(g["depth"]), post_nms_topk=int(g["post_topk"]), detections=int(g["det"]))
    x = synthetic_images(n, h, w, seed=int(g["images_seed"]))
    shapes = g["shapes"].tolist()
    for i, (hh, ww) in enumerate(shapes):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    return kw, int(g["weights_seed"]), torch.from_numpy(x), shapes


def align_cfg(kw, kind="ROIAlignV2", sr=0, extra=()):
    return vg_c4_config(overrides=[("roi_box_head", "pooler_type", kind), ("roi_box_head", "pooler_sampling_ratio", sr)] + list(extra),
                        **kw)


_SD = {}


def state_dict(cfg, seed, key="plain"):
    if key not in _SD:
        _SD[key] = make_state_dict(cfg, seed=seed)
    return _SD[key]


def build(cfg, sd, precision, **options):
    m = FRCNN(cfg, precision=precision).load_state_dict(sd).eval()
    m.set_option("head_chunk", 0)
    for k, v in options.items():
        m.set_option(k, v)
    return m


def pooled_vs_oracle(m, oracle, shapes):
    """The "pooled" stage against the oracle's pool on the GPU's own res4 and proposals."""
    R = m.config.RPN.POST_NMS_TOPK_TEST
    pb, pc = m.get_stage("proposal_boxes").cpu(), m.get_stage("proposal_counts").cpu()
    boxes = [pb[i, :int(pc[i])] for i in range(len(shapes))]
    rows = np.concatenate([np.arange(int(pc[i])) + i * R for i in range(len(shapes))])
    ref = oracle.pool(nchw(m.get_stage("res4")), boxes)
    return G.rel_err(nchw(m.get_stage("pooled"))[rows], ref)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("sr", [0, 2])
def test_model_roialignv2_chain_vs_align_oracle(setup, sr, precision):
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", sr)
    sd = state_dict(cfg, seed)
    m = build(cfg, sd, precision)
    assert m.pooler == (L.VK_POOLER_ROIALIGNV2, sr)
    out = m(x, torch.tensor(shapes))
    oracle = U.AlignOracle(cfg, sd, emulate="fp16" if precision == "fp16" else None)
    stage_chain_check(m, out, oracle, shapes, tol=1e-3 if precision == "fp16" else 1e-4)
    if precision == "fp32":
        e = pooled_vs_oracle(m, oracle, shapes)
        print(f"\n[ROIAlignV2 sr={sr}] pooled rel err {e:.3e}")
        assert e <= 1e-5


def test_model_roialign_unaligned_chain(setup):
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlign", 2)
    sd = state_dict(cfg, seed)
    m = build(cfg, sd, "fp32")
    out = m(x, torch.tensor(shapes))
    oracle = U.AlignOracle(cfg, sd)
    stage_chain_check(m, out, oracle, shapes, tol=1e-4)
    assert pooled_vs_oracle(m, oracle, shapes) <= 1e-5
    # aligned and unaligned are different rules: the pooled tensors must differ
    m2 = build(align_cfg(kw, "ROIAlignV2", 2), sd, "fp32")
    m2(x, torch.tensor(shapes))
    assert not torch.equal(m.get_stage("pooled"), m2.get_stage("pooled"))


def test_model_detectron2_layout_chain(setup):
    """RES5HALVE = true, the stride in the 3x3, ROIAlignV2 with adaptive sampling: detectron2's own C4 layout."""
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", 0, extra=[("roi_box_head", "res5halve", True), ("resnets", "stride_in_1x1", False)])
    sd = state_dict(cfg, seed, key="d2")
    m = build(cfg, sd, "fp32")
    out = m(x, torch.tensor(shapes))
    stage_chain_check(m, out, U.AlignOracle(cfg, sd), shapes, tol=1e-4)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_model_given_boxes_vs_align_oracle(setup, precision):
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", 0)
    sd = state_dict(cfg, seed)
    m = build(cfg, sd, precision)
    props = [np.array([[10.0, 12.0, 200.0, 150.0], [-40.0, -30.0, 120.0, 90.0], [50.0, 60.0, 50.0, 120.0], [77.0, 33.0, 78.0, 34.0],
                       [-500.0, -500.0, 900.0, 900.0]], np.float32),
             np.array([[20.5, 30.25, 90.75, 110.0], [180.0, 90.0, 40.0, 20.0]], np.float32)][:len(shapes)]
    out = m(x[:len(props)], torch.tensor(shapes[:len(props)]), proposals=props)
    assert out["preds_per_image"].tolist() == [len(p) for p in props]
    pb = m.get_stage("proposal_boxes").cpu()                 # the clipped boxes, network pixels
    boxes = [pb[i, :len(p)] for i, p in enumerate(props)]
    oracle = U.AlignOracle(cfg, sd, emulate="fp16" if precision == "fp16" else None)
    ref = oracle.res5(oracle.pool(nchw(m.get_stage("res4")), boxes)).mean(dim=[2, 3])
    feat = torch.cat([out["roi_features"][i].cpu() for i in range(len(props))])
    e = G.rel_err(feat, ref)
    print(f"\n[given boxes, ROIAlignV2, {precision}] roi_features rel err {e:.3e}")
    assert e <= (1e-3 if precision == "fp16" else 1e-4)


def test_model_every_selection_pools_through_roialign(setup):
    """per_class and detections run the same head: their feature rows are the class_max forward's bytes, and every output
    row is its proposal's feature row."""
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", 0)
    sd = state_dict(cfg, seed)
    m = build(cfg, sd, "fp16")
    R = cfg.RPN.POST_NMS_TOPK_TEST
    m(x, torch.tensor(shapes))
    feat0 = m.get_stage("feature_pooled")
    for sel in ("per_class", "detections"):
        m.roi_outputs.selection = sel
        m.roi_outputs.nms_thresh = [0.3]
        if sel == "detections":
            m.roi_outputs.min_detections = 0
        out = m(x, torch.tensor(shapes))
        feat = m.get_stage("feature_pooled")
        assert torch.equal(feat, feat0)
        kid = m.get_stage("keep_ids").cpu()
        for i in range(len(shapes)):
            k = int(out["preds_per_image"][i])
            assert torch.equal(out["roi_features"][i].cpu(), feat.cpu()[kid[i, :k] + i * R])


def test_model_chunks_and_head_streams_give_identical_bytes(setup):
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", 0)
    sd = state_dict(cfg, seed)
    K = len(shapes) * cfg.RPN.POST_NMS_TOPK_TEST
    ref_m = build(cfg, sd, "fp16")
    ref = ref_m(x, torch.tensor(shapes), return_tensors="pt", padding="max_detections")
    ref_feat = ref_m.get_stage("feature_pooled")
    for options in (dict(head_chunk=17), dict(head_chunk=K - 1), dict(head_streams=2, head_split_min_rois=2),
                    dict(head_chunk=23, head_streams=2, head_split_min_rois=2)):
        assert options.get("head_chunk", K) <= K
        m = build(cfg, sd, "fp16", **options)
        out = m(x, torch.tensor(shapes), return_tensors="pt", padding="max_detections")
        assert torch.equal(m.get_stage("feature_pooled"), ref_feat), options
        for k in ref:
            assert torch.equal(out[k], ref[k]), (options, k)


def test_default_path_is_untouched(setup, monkeypatch):
    # the fixture model's 60 RoIs are fewer tiles than conv_gemm4 takes by default; the dedupe path needs it (re-read per launch)
    monkeypatch.setenv("VK_CONV_GEMM4", "2")
    kw, seed, x, shapes = setup
    cfg_absent = vg_c4_config(**kw)
    assert "pooler_type" not in cfg_absent.ROI_BOX_HEAD.to_dict()
    cfg_pool = vg_c4_config(overrides=[("roi_box_head", "pooler_type", "ROIPool")], **kw)
    sd = state_dict(cfg_absent, seed)
    outs = []
    for cfg in (cfg_absent, cfg_pool):
        m = build(cfg, sd, "fp16")
        assert m.pooler == (L.VK_POOLER_ROIPOOL, 0)
        outs.append(m(x, torch.tensor(shapes), return_tensors="pt", padding="max_detections"))
        assert int(m.get_stage("head_windows").sum()) > 0          # the dedupe path ran: distinct RoIPool windows per chunk
        assert m.get_option("dedupe_chunks") == 1
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    ma = build(align_cfg(kw), sd, "fp16")
    out_a = ma(x, torch.tensor(shapes), return_tensors="pt", padding="max_detections")
    with pytest.raises(ValueError):
        ma.get_stage("head_windows")
    assert ma.get_option("dedupe_chunks") == 0
    assert not torch.equal(out_a["roi_features"], outs[0]["roi_features"])       # another pooler, other features
    # the pooler is fixed once the handle has run a forward
    lib = L.load()
    assert lib.vk_set_pooler(ma._h, L.VK_POOLER_ROIPOOL, 0) == L.VK_EINVAL
    t, r = C.c_int(-1), C.c_int(-1)
    L.call("vk_get_pooler", ma._h, C.byref(t), C.byref(r))
    assert (t.value, r.value) == (L.VK_POOLER_ROIALIGNV2, 0)
    fresh = FRCNN(cfg_absent, precision="fp16")
    assert lib.vk_set_pooler(fresh._h, L.VK_POOLER_ROIALIGN, 3) == L.VK_OK
    assert lib.vk_set_pooler(fresh._h, L.VK_POOLER_ROIALIGN, 9) == L.VK_EINVAL
    with pytest.raises(ValueError):
        FRCNN(vg_c4_config(overrides=[("roi_box_head", "pooler_type", "ROIAlignV3")], **kw), precision="fp16")


def test_nan_box_raises_the_reference_assertion(setup):
    """Last on purpose.  A NaN coordinate in a caller-supplied box: the ingest flags it and clips it to the image (fminf / fmaxf
    drop the NaN), so the pooler sees a finite box inside the map; the forward ends in the reference's AssertionError
    (frcnn.py:148), and the process goes on."""
    kw, seed, x, shapes = setup
    cfg = align_cfg(kw, "ROIAlignV2", 0)
    m = build(cfg, state_dict(cfg, seed), "fp16")
    props = [np.array([[10.0, 12.0, 100.0, 90.0], [float("nan"), 12.0, 100.0, 90.0]], np.float32),
             np.array([[20.0, 30.0, 90.0, 110.0]], np.float32)][:len(shapes)]
    with pytest.raises(AssertionError):
        m(x[:len(props)], torch.tensor(shapes[:len(props)]), proposals=props)
    ok = [p[:1] for p in props]
    out = m(x[:len(props)], torch.tensor(shapes[:len(props)]), proposals=ok)          # the handle is still good
    assert out["preds_per_image"].tolist() == [1] * len(props)
    assert all(torch.isfinite(f).all() for f in out["roi_features"])
