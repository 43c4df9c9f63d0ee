"""-m gpu: Res5 block 0 over the distinct RoIPool windows (csrc/roi_windows.hip, the DD form of csrc/conv_gemm4.hip, option
"head_dedupe").  Nothing here has a tolerance: the window table is held to the numpy restatement (tests/roi_dedupe_util.py,
itself held to the oracle's RoIPool by tests/test_roi_windows_host.py), every tensor to the plain kernels' bits, and the
model with head_dedupe = 1 to the same model with head_dedupe = 0."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, P, pack_conv, launch, stream   # noqa: E402
from roi_dedupe_util import SCALE, crafted_boxes, distinct_boxes, window_table   # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L   # noqa: E402

PP = 14
MAPS = [(6, 9), (13, 21)]


@pytest.fixture(autouse=True)
def small_grids(monkeypatch):
    monkeypatch.setenv("VK_CONV_GEMM4", "2")        # conv_gemm4 also at the few tiles of these shapes (re-read per launch)


def roi_set(hw, R, kind):
    """R RoIs over two images of map hw.  kind: "ragged" (a third on image 0), "empty0" (image 0 has none), "distinct" (every
    window distinct: boxes of P x P cells on disjoint cells, as many as the maps hold, at most R)."""
    if kind == "distinct":
        return distinct_boxes([hw, hw], (R + 1) // 2, P=6)
    base = crafted_boxes([hw])                       # 16 crafted boxes; further copies shifted by whole and half cells
    rows = np.concatenate([base + np.float32([0, 24.0 * j, 8.0 * j, 24.0 * j, 8.0 * j]) for j in range((R + 15) // 16)])[:R]
    rows[:, 0] = 1
    if kind == "ragged":
        rows[: R // 3, 0] = 0
    return rows


def run_table(rois, N, H, W, Pn):
    K = len(rois)
    rows = K * Pn * Pn
    ws_bytes = L.load().vk_roi_windows_workspace_bytes(N, H, W)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    r = torch.from_numpy(np.ascontiguousarray(rois)).to(DEV)
    idx = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    win = torch.full((rows, 5), -1, dtype=torch.int32, device=DEV)
    u = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.call("vk_roi_windows", P(r), K, N, H, W, Pn, SCALE, P(idx), P(win), P(u), P(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    return r, idx, win, u


@pytest.mark.parametrize("kind", ["ragged", "empty0", "distinct"])
@pytest.mark.parametrize("R", [1, 2, 17, 64])
@pytest.mark.parametrize("hw", MAPS)
def test_table_pool_gather(hw, R, kind):
    H, W = hw
    Pn = 6 if kind == "distinct" else PP
    rois = roi_set(hw, R, kind)
    K = len(rois)
    assert K >= 1
    r, idx, win, u = run_table(rois, 2, H, W, Pn)
    ref_idx, ref_win = window_table(rois, 2, H, W, Pn)
    U = int(u.item())
    print(f"map {hw} R {R} {kind}: {K * Pn * Pn} bins, {U} windows")
    assert U == len(ref_win)
    if kind == "distinct":
        assert U == K * Pn * Pn
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    assert np.array_equal(win[:U].cpu().numpy(), ref_win)
    assert bool((win[U:] == -1).all())                                  # nothing past the list is written

    for Cc in (64, 1024):
        g = torch.Generator().manual_seed(H * 100 + R)
        feat = torch.randn((2, H, W, Cc), generator=g).half().to(DEV)
        dense = torch.zeros((K, Pn, Pn, Cc), dtype=torch.float16, device=DEV)
        L.call("vk_roi_pool", P(feat), 2, H, W, Cc, P(r), K, SCALE, Pn, P(dense), L.VK_F16, stream())
        pooled_u = torch.full((K * Pn * Pn, Cc), 7.0, dtype=torch.float16, device=DEV)
        L.call("vk_roi_pool_windows", P(feat), 2, H, W, Cc, P(win), P(u), K * Pn * Pn, P(pooled_u), L.VK_F16, stream())
        torch.cuda.synchronize()
        assert bool((pooled_u[U:] == 7.0).all())
        assert torch.equal(pooled_u[idx.long()].view(torch.int16), dense.view(-1, Cc).view(torch.int16))
        out = torch.zeros_like(dense)
        L.call("vk_gather_rows", P(pooled_u), P(idx), K * Pn * Pn, Cc * 2, P(out), stream())
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), dense.view(torch.int16))


def conv_weights(cout, cin, seed):
    g = np.random.default_rng(seed)
    w = (g.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    return pack_conv(w, None, g.standard_normal(cout).astype(np.float32) * 0.1, L.VK_F16)


@pytest.mark.parametrize("case", ["crafted17", "crafted64", "one_window", "distinct"])
def test_gemm4_on_distinct_rows(case):
    """conv1 over U rows with M read on the device, and the fused conv3 + shortcut GEMM with its second input read through idx,
    against the plain launches on the expanded tensors.  Row counts: 17 * 196 = 3332 and 64 * 196 = 12544 (13 and 49 row
    tiles, the first ragged: 3332 = 13 * 256 + 4), 11 * 196 = 2156 with U = 1 (one tile, one live row) and with four boxes'
    worth of windows, none repeated inside a box."""
    hw = MAPS[1]
    if case == "one_window":
        rois = np.tile(np.float32([[1, 33.0, 34.0, 38.0, 39.0]]), (11, 1))      # a box inside one cell: one window for all bins
    elif case == "distinct":
        rois = np.concatenate([distinct_boxes([(14, 28), (14, 28)], 2, P=PP)] * 3)[:11]
        hw = (14, 28)
    else:
        rois = roi_set(hw, int(case[7:]), "ragged")
    K = len(rois)
    M = K * PP * PP
    _, idx, _, u = run_table(rois, 2, hw[0], hw[1], PP)
    U = int(u.item())
    assert U == {"one_window": 1}.get(case, U) and (M % 256 != 0) == (case != "crafted64")
    if case == "distinct":
        assert U == 4 * PP * PP                         # four boxes' worth of distinct windows, repeated
    g = torch.Generator().manual_seed(5)
    x_u = torch.randn((M, 1024), generator=g).half().to(DEV)            # rows from U on are never read
    w1, b1 = conv_weights(512, 1024, 1)
    y_u = torch.full((M, 512), 3.0, dtype=torch.float16, device=DEV)
    L.call("vk_conv1x1_rows", P(x_u), 1024, None, 0, M, P(u), None, P(w1), P(b1), P(y_u), 512, 1, stream())
    x_full = x_u[idx.long()].contiguous()
    y_full = torch.zeros((M, 512), dtype=torch.float16, device=DEV)
    launch("vk_conv2d", P(x_full), 1, 1, M, 1024, P(w1), P(b1), None, P(y_full), 512, 512, 1, 1, 1, 0, 1, 1, 1, L.VK_F16, L.VK_F16,
           stream(), expect_route="gemm4")
    torch.cuda.synchronize()
    assert bool((y_u[U:] == 3.0).all())                                 # rows past the device-side M are not written
    assert torch.equal(y_u[idx.long()].view(torch.int16), y_full.view(torch.int16))
    assert float(y_full.float().abs().max()) > 0.5

    t = torch.randn((M, 512), generator=g).half().to(DEV)
    w3, b3 = conv_weights(2048, 512 + 1024, 2)
    y_idx = torch.zeros((M, 2048), dtype=torch.float16, device=DEV)
    L.call("vk_conv1x1_rows", P(t), 512, P(x_u), 1024, M, None, P(idx), P(w3), P(b3), P(y_idx), 2048, 1, stream())
    y_ref = torch.zeros((M, 2048), dtype=torch.float16, device=DEV)
    launch("vk_conv1x1_dual", P(t), 512, P(x_full), 1024, M, P(w3), P(b3), None, P(y_ref), 2048, 1, stream(), expect_route="gemm4")
    torch.cuda.synchronize()
    assert torch.equal(y_idx.view(torch.int16), y_ref.view(torch.int16))
    # the shortcut half matters: without it the rows differ
    L.call("vk_conv1x1_rows", P(t), 512, P(x_u), 1024, M, None, None, P(w3), P(b3), P(y_idx), 2048, 1, stream())
    torch.cuda.synchronize()
    assert U == M or not torch.equal(y_idx.view(torch.int16), y_ref.view(torch.int16))


# ---- model level ----
STAGES = ("res4", "pooled", "feature_pooled", "obj_logits", "attr_logits")


@pytest.fixture(scope="module")
def setup():
    cfg = vg_c4_config(post_nms_topk=30, detections=12)
    sd = make_state_dict(cfg, seed=1234)
    shapes = torch.tensor([[160, 224], [144, 200]])
    xs = []
    for seed in (21, 22):
        x = synthetic_images(2, 160, 224, seed=seed)
        for i, (hh, ww) in enumerate(shapes.tolist()):
            x[i, :, hh:, :] = 0
            x[i, :, :, ww:] = 0
        xs.append(torch.from_numpy(x).cuda())
    return cfg, sd, xs, shapes


@pytest.fixture(scope="module")
def model(setup):
    cfg, sd, _, _ = setup
    return FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()


def block(p):
    return {k: v.clone() for k, v in p.wait_raw().items()}


def run(m, dedupe, calls, stages=STAGES):
    """The calls one after the other with head_dedupe = dedupe: their outputs, the last one's stages, chunks that took the path."""
    m.set_option("head_dedupe", dedupe)
    n0 = m.get_option("dedupe_chunks")
    outs = [block(m.forward_async(**kw)) for kw in calls]
    st = {s: m.get_stage(s).clone() for s in stages}
    return outs, st, m.get_option("dedupe_chunks") - n0


def same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), (what, i, k)


GIVEN = [np.array([[10.0, 12.0, 90.0, 100.0], [10.0, 12.0, 90.0, 100.0], [30.0, 5.0, 200.0, 150.0], [0.0, 0.0, 50.0, 40.0],
                   [33.0, 34.0, 38.0, 40.0], [10.0, 12.0, 90.0, 100.0], [0.0, 0.0, 223.0, 159.0]] * 2, np.float32),
         np.array([[5.0, 5.0, 60.0, 70.0], [5.0, 5.0, 60.0, 70.0], [100.0, 20.0, 180.0, 120.0]] * 4, np.float32)]


@pytest.mark.parametrize("what", ["detection", "given_boxes"])
def test_model_same_bits(setup, model, what):
    _, _, xs, shapes = setup
    calls = [dict(images=xs[0], image_shapes=shapes, **({"proposals": GIVEN} if what == "given_boxes" else {}))]
    ref, ref_st, n_ref = run(model, 0, calls)
    got, got_st, n_got = run(model, 1, calls)
    assert n_ref == 0 and n_got == 1
    same(got, ref, what)
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["pooled"].float().abs().max()) > 0
    hwn = model.get_stage("head_windows")
    bins = ref_st["pooled"].shape[0] * PP * PP
    print(f"{what}: {bins} bins, {int(hwn[0])} windows")
    assert 0 < int(hwn[0]) < bins


def test_model_two_lanes_overlapped(setup, model):
    _, _, xs, shapes = setup
    calls = [dict(images=x, image_shapes=shapes) for x in (xs[0], xs[1], xs[0], xs[1])]
    model.set_option("forward_lanes", 1)
    ref, ref_st, _ = run(model, 0, calls)
    model.set_option("forward_lanes", 2)
    model.set_option("head_dedupe", 1)
    n0, lane0 = model.get_option("dedupe_chunks"), model.get_option("lane_forwards")
    pend = [model.forward_async(**kw) for kw in calls]
    got = [block(p) for p in pend]
    assert model.get_option("lane_forwards") - lane0 >= 3 and model.get_option("dedupe_chunks") - n0 == 4
    same(got, ref, "lanes")
    for s in STAGES:                                 # the last begun forward's, "pooled" expanded in its own working set
        assert torch.equal(model.get_stage(s), ref_st[s]), s
    assert not torch.equal(ref[0]["roi_features"], ref[1]["roi_features"])


def test_model_chunked(setup):
    """head_chunk = 25 of K = 60 RoIs: chunks of 25, 25 and 10.  The last has 1960 rows, below conv_gemm4's 2048, and takes the
    plain path; the stage "pooled" is not offered by a chunked forward."""
    cfg, sd, xs, shapes = setup
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    m.set_option("head_chunk", 25)
    st = ("res4", "feature_pooled", "obj_logits", "attr_logits")
    calls = [dict(images=xs[1], image_shapes=shapes)]
    ref, ref_st, n_ref = run(m, 0, calls, st)
    got, got_st, n_got = run(m, 1, calls, st)
    assert n_ref == 0 and n_got == 2
    same(got, ref, "chunked")
    for s in st:
        assert torch.equal(got_st[s], ref_st[s]), s


def test_plain_path_where_the_conditions_fail(setup, model, monkeypatch):
    """Strict fp32, head_streams = 2 and a conv_gemm4 that does not take the small grid: head_dedupe = 1 runs the plain path."""
    cfg, sd, xs, shapes = setup
    calls = [dict(images=xs[0], image_shapes=shapes)]
    m32 = FRCNN(cfg, precision="fp32").load_state_dict(sd).eval()
    assert m32.get_option("head_dedupe") == 1
    assert run(m32, 1, calls, ("feature_pooled",))[2] == 0
    ref, ref_st, _ = run(model, 0, calls)
    model.set_option("head_streams", 2)
    try:
        got, got_st, n = run(model, 1, calls)
    finally:
        model.set_option("head_streams", 1)
    assert n == 0
    same(got, ref, "head_streams")
    monkeypatch.delenv("VK_CONV_GEMM4")
    assert run(model, 1, calls)[2] == 0              # 92 tiles: below conv_gemm4's one tile per CU
    monkeypatch.setenv("VK_CONV_GEMM4", "2")
    assert run(model, 1, calls)[2] == 1
