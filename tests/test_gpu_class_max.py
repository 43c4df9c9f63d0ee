"""-m gpu: the box-head tail of the default selection (vltk_amd/csrc/roi_out.hip), piece by piece.

Pieces: vk_softmax_argmax against an fp64 soft-max (ties, padding, hand-built rows); vk_chosen_deltas bit-exact on integer data
(every partial sum below 2^24: fp32 accumulation is exact in any order); vk_concat_embed and vk_make_rois bit-exact.
Selection: vk_roi_outputs against the tests' restatement of the class-max rule (tests/class_max_util.py, held to the reference's
vectors and to the oracle by test_class_max_host.py) at RoI counts on both sides of the workgroup's 256 threads, in every regime
of the threshold loop, every output bit for bit.  The crafted size deltas are zero (exp(0) is exact on both sides) and the
restatement receives (prob, cls) from the device's own vk_softmax_argmax, so every rank, IoU and suppression is the same IEEE
arithmetic on the device and on the host."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                         # noqa: E402

import class_max_util as CM                            # noqa: E402
import gpu_util as G                                   # noqa: E402

SENT = -7.0
INF, NAN = float("inf"), float("nan")


# ---- vk_softmax_argmax ------------------------------------------------------------------------------------------------
def softmax_argmax(x, n_soft, n_arg, K=None, pad=5, raw=True):
    """x [rows, n_soft] f32 on the host -> (prob, cls, raw) of the first K rows from the device; the logits live in a
    [rows, n_soft + pad] matrix whose padding columns hold 1e30, and the outputs of the rows >= K must stay untouched."""
    rows = x.shape[0]
    K = rows if K is None else K
    xd = torch.full((rows, n_soft + pad), 1e30, device=G.DEV)
    xd[:, :n_soft] = x.to(G.DEV)
    prob = torch.full((rows + 3,), SENT, device=G.DEV)
    cls = torch.full((rows + 3,), -7, dtype=torch.int32, device=G.DEV)
    arg = torch.full((rows + 3,), -7, dtype=torch.int32, device=G.DEV)
    L.call("vk_softmax_argmax", G.P(xd), n_soft + pad, K, n_soft, n_arg, G.P(prob), G.P(cls), G.P(arg) if raw else None, G.stream())
    torch.cuda.synchronize()
    prob, cls, arg = prob.cpu(), cls.cpu(), arg.cpu()
    assert (prob[K:] == SENT).all() and (cls[K:] == -7).all() and (arg[K if raw else 0:] == -7).all()
    return prob[:K], cls[:K], arg[:K]


def check_softmax(x, n_soft, n_arg, K=None):
    prob, cls, arg = softmax_argmax(x, n_soft, n_arg, K)
    K = len(prob)
    x64 = x[:K].double().numpy()
    with np.errstate(invalid="ignore"):
        e = np.exp(x64 - x64.max(1, keepdims=True))
    p64 = e / e.sum(1, keepdims=True)
    want_cls = p64[:, :n_arg].argmax(1)                  # numpy: the first of equal maxima
    want_raw = x64.argmax(1)
    np.testing.assert_array_equal(cls.numpy(), want_cls)
    np.testing.assert_array_equal(arg.numpy(), want_raw)
    err = G.rel_err(prob, p64[np.arange(K), want_cls])
    print(f"[softmax_argmax] K={K} n_softmax={n_soft} n_argmax={n_arg}: prob rel err vs fp64 {err:.2e}")
    assert err <= 2e-6
    return prob, cls, arg


@pytest.mark.parametrize("K", [1, 5, 67])
@pytest.mark.parametrize("n_soft,n_arg", [(2, 1), (2, 2), (63, 63), (64, 63), (65, 64), (401, 400), (1601, 1600)])
def test_softmax_argmax_against_fp64(n_soft, n_arg, K):
    """Logits N(0, 3) in multiples of 1/8: exact ties are common (the lowest index wins), and any two distinct logits differ
    in probability by a factor >= e^0.125, far above fp32 error.  Two rows more than K are handed over and must stay unread."""
    g = torch.Generator().manual_seed(n_soft * 100 + K)
    x = torch.round(torch.randn((K + 2, n_soft), generator=g) * 3.0 * 8) / 8
    check_softmax(x, n_soft, n_arg, K)
    if K == 67 and n_soft >= 64:
        sub = x[:K, :n_arg]
        assert ((sub == sub.max(1, keepdim=True).values).sum(1) > 1).any(), "no row has a tied maximum"


def test_softmax_argmax_rows_built_by_hand():
    n_soft, n_arg = 200, 199
    g = torch.Generator().manual_seed(77)
    base = torch.round(torch.randn((12, n_soft), generator=g) * 2.0 * 8) / 8          # |x| < 12
    x = base.clone()
    x[0, 70] = x[0, 134] = 20.0                  # the maximum twice inside one lane's stride (columns c and c + 64)
    x[1, 71] = x[1, 100] = 20.0                  # ... across lanes, the lower column in the lower lane
    x[2, 69] = x[2, 130] = 20.0                  # ... across lanes, the lower column in the higher lane (130 is lane 2)
    x[3, 199] = 20.0                             # the maximum in the last column: n_argmax = n_softmax - 1 must not see it
    x[4, 17] = -INF                              # one -inf entry
    x[5] += 1e4                                  # offsets: no overflow, and the multiples of 1/8 stay exact at 1e4
    x[6] -= 1e4
    x[7, :199], x[7, 199] = 0.0, 100.0           # background 100 above equal class logits: every class ties -> class 0
    x[8, :199], x[8, 199] = 0.0, 120.0           # ... and here the class probabilities underflow to 0 in fp32: still a tie
    x[9, 0] = x[9, 198] = 20.0                   # first and last class
    x[10, 63] = x[10, 64] = 20.0                 # lane 63 and lane 0 of the next stride
    x[11, 198] = 20.0                            # the last class alone
    prob, cls, arg = check_softmax(x, n_soft, n_arg)
    assert cls.tolist()[:3] == [70, 71, 69] and arg.tolist()[:4] == [70, 71, 69, 199] and cls[3] != 199
    assert cls[7] == 0 and cls[8] == 0 and arg[7] == 199 and arg[8] == 199
    assert cls.tolist()[9:] == [0, 63, 198]
    assert bool(torch.isfinite(prob).all()) and float(prob[5]) > 0 and float(prob[6]) > 0


# ---- vk_chosen_deltas -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_head(F, rows):
    """bbox_pred with integer weights in {-3..3} and an integer bias: exact in f16 and f32."""
    g = torch.Generator().manual_seed(F + rows)
    w = torch.randint(-3, 4, (rows, F), generator=g, dtype=torch.int64)
    b = torch.randint(-9, 10, (rows,), generator=g, dtype=torch.int64)
    return w, b


def chosen_deltas(x, ldx, w, b, cls, K, dt):
    """x [rows, F] i64 on the host -> vk_chosen_deltas' [K, 4] from the device; x lives in a [rows, ldx] matrix of dt whose
    padding columns hold 1000; one output row more than K is handed over and must stay untouched."""
    rows, F = x.shape
    td = G.TDT[dt]
    xd = torch.full((rows, ldx), 1000.0, dtype=td, device=G.DEV)
    xd[:, :F] = x.to(td).to(G.DEV)
    wd, bd = w.to(td).to(G.DEV).contiguous(), b.float().to(G.DEV)
    cd = cls.to(torch.int32).to(G.DEV) if cls is not None else None
    out = torch.full((K + 1, 4), SENT, device=G.DEV)
    L.call("vk_chosen_deltas", G.P(xd), ldx, G.P(wd), G.P(bd), G.P(cd), int(cls is None), F, K, G.P(out), dt, G.stream())
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[K:] == SENT).all()
    return out[:K]


@pytest.mark.parametrize("K", [1, 5, 67])
@pytest.mark.parametrize("F", [2048, 100])
@pytest.mark.parametrize("agnostic", [False, True], ids=["C1600", "agnostic"])
@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["f32", "f16"])
def test_chosen_deltas_exact_on_integers(dt, agnostic, F, K):
    """x in {-4..4}, weights in {-3..3}, integer bias: every partial sum is an integer below 2048 * 12 + 9 < 2^24, so the
    fp32 accumulation is exact in any order and the result must equal the int64 product.  ldx > F, as the FPN head calls it."""
    Cn = 1600
    w, b = integer_head(F, 4 if agnostic else 4 * Cn)
    g = torch.Generator().manual_seed(F + K)
    x = torch.randint(-4, 5, (K + 1, F), generator=g, dtype=torch.int64)
    cls = None
    if not agnostic:
        cls = torch.randint(0, Cn, (K,), generator=g)
        cls[-1] = Cn - 1
        if K > 1:
            cls[0] = 0
    got = chosen_deltas(x, F + 8, w, b, cls, K, dt)
    r = torch.arange(4)[None, :] + (4 * cls[:, None] if cls is not None else torch.zeros((K, 1), dtype=torch.int64))
    want = (x[:K, None, :] * w[r]).sum(-1) + b[r]
    assert int(want.abs().max()) > 0
    np.testing.assert_array_equal(got.numpy(), want.float().numpy())


# ---- vk_concat_embed, vk_make_rois ------------------------------------------------------------------------------------
F16_EDGES = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20,   # halfway cases
             2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 1e-40, -1e-40,    # subnormals
             65503.9, 65504.0, 65519.0, -65519.0, 0.0, -0.0]                                                           # the top


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["f32", "f16"])
@pytest.mark.parametrize("F,E", [(2048, 256), (100, 12), (2048, 0)])
def test_concat_embed_exact(F, E, dt):
    K, V, td = 5, 9, G.TDT[dt]
    g = torch.Generator().manual_seed(F + E)
    feat = torch.randn((K + 1, F), generator=g) * 3
    edges = torch.tensor(F16_EDGES, dtype=torch.float64).float()
    feat[0, :len(edges)] = edges
    feat[K - 1, F - len(edges):] = -edges
    emb = (torch.randn((V, max(E, 1)), generator=g) * 2).to(td)
    cls = torch.tensor([V - 1, 0, 3, 3, 8], dtype=torch.int32)
    out = torch.full((K + 1, F + E), SENT, dtype=td, device=G.DEV)
    fd, ed, cd = feat.to(G.DEV), emb.to(G.DEV), cls.to(G.DEV)
    L.call("vk_concat_embed", G.P(fd), F, G.P(ed) if E else None, E, G.P(cd) if E else None, K, G.P(out), dt, G.stream())
    torch.cuda.synchronize()
    want = torch.cat([feat[:K].to(td), emb[cls.long(), :E]], -1)
    if dt == L.VK_F16:
        assert bool(torch.isfinite(want).all()) and float(want[0, 0]) == 1.0 and float(want[0, 5]) == 0.0
    np.testing.assert_array_equal(bits(out.cpu()[:K]), bits(want))
    assert (out.cpu()[K:] == SENT).all()


def test_make_rois_exact():
    N, R = 3, 37
    boxes = torch.randn((N, R, 4), generator=torch.Generator().manual_seed(5)) * 200
    bd = boxes.to(G.DEV)
    rois = torch.full((N * R + 1, 5), SENT, device=G.DEV)
    L.call("vk_make_rois", G.P(bd), N, R, G.P(rois), G.stream())
    torch.cuda.synchronize()
    want = torch.cat([torch.arange(N).repeat_interleave(R)[:, None].float(), boxes.reshape(-1, 4)], 1)
    np.testing.assert_array_equal(bits(rois.cpu()[:N * R]), bits(want))
    assert (rois.cpu()[N * R:] == SENT).all()


# ---- vk_roi_outputs against the restatement -----------------------------------------------------------------------------
OUT_KEYS = ("obj_ids", "obj_probs", "attr_ids", "attr_probs", "boxes", "preds_per_image", "roi_features")


def roi_params(thr, mind, maxd):
    rp = L.vk_roi_params()
    rp.num_nms_thresh = len(thr)
    for i, t in enumerate(thr):
        rp.nms_thresh[i] = t
    rp.min_detections, rp.max_detections = mind, maxd
    return rp


def gpu_roi_outputs(d, thr, mind, maxd, scales=None, attr=True, deltas=None, chosen_only=0, weights=CM.WEIGHTS, R=None, F=None, D=None):
    """vk_roi_outputs on the crafted data d, into buffers pre-filled with a sentinel.  R, F, D override what the call is told
    (for the calls that must be refused)."""
    N, dev = d["N"], G.DEV
    R = d["R"] if R is None else R
    Fd = d["feats"].shape[1] if F is None else F
    D = maxd if D is None else D
    lg, pr, ft = d["logits"].to(dev), d["props"].to(dev), d["feats"].to(dev)
    dl = (d["deltas"] if deltas is None else deltas).to(dev).contiguous()
    al = d["attr"].to(dev) if attr else None
    cn, hw = torch.from_numpy(d["counts"]).to(dev), torch.from_numpy(d["hw"]).to(dev)
    scd = torch.as_tensor(scales, dtype=torch.float32).to(dev) if scales is not None else None
    o = dict(obj_ids=torch.full((N, D), -7, dtype=torch.int64, device=dev), obj_probs=torch.full((N, D), SENT, device=dev),
             attr_ids=torch.full((N, D), -7, dtype=torch.int64, device=dev), attr_probs=torch.full((N, D), SENT, device=dev),
             boxes=torch.full((N, D, 4), SENT, device=dev), preds_per_image=torch.full((N,), -7, dtype=torch.int64, device=dev),
             roi_features=torch.full((N, D, d["feats"].shape[1]), SENT, device=dev))
    keep = torch.full((N, D), -7, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = L.vk_outputs(*[o[k].data_ptr() for k in OUT_KEYS])
    rp = roi_params(thr, mind, maxd)
    try:
        L.call("vk_roi_outputs", G.P(lg), lg.shape[1], G.P(al), CM.A + 1 if attr else 0, G.P(dl), dl.shape[1], chosen_only, G.P(pr),
               G.P(cn), G.P(ft), Fd, N, R, CM.C, CM.A if attr else 0, G.P(hw), G.P(scd), (C.c_float * 4)(*weights), C.byref(rp),
               C.byref(out), G.P(keep), G.P(flag), G.stream())
    finally:
        torch.cuda.synchronize()
        res = {k: v.cpu() for k, v in o.items()}
        res.update(keep_ids=keep.cpu(), flag=int(flag.cpu()))
        d["last"] = res
    return res


def device_softmax(d):
    """(prob, cls) of the class logits and of the attribute logits from vk_softmax_argmax on the same device logits, as
    vk_roi_outputs computes them (test_softmax_argmax_against_fp64 holds that kernel to fp64)."""
    if "dev_sm" not in d:
        K = d["N"] * d["R"]
        p, c, _ = softmax_argmax(d["logits"], CM.C + 1, CM.C, K, pad=0, raw=False)
        ap, ac, _ = softmax_argmax(d["attr"][:, :CM.A], CM.A, CM.A, K, pad=1, raw=False)
        d["dev_sm"] = (p, c.long(), ap, ac.long())
    return d["dev_sm"]


def check_exact(d, got, thr, mind, maxd, scales=None, attr=True, boxes=None, regime=None):
    """Every output of the device call against the restatement, bit for bit; rows beyond preds_per_image are zero.
    boxes [K, C, 4]: the device's own decoded boxes in place of the deltas.  regime: asserted, from the restatement's
    trace alone, before the device's outputs are looked at.  -> the restatement's ids per image."""
    N, R = d["N"], d["R"]
    prob, cls, ap, ac = device_softmax(d)
    refs = []
    for n in range(N):
        c = int(d["counts"][n])
        rows = slice(n * R, n * R + c)
        trace = []
        ref = CM.select_image(prob[rows], cls[rows], d["deltas"][rows] if boxes is None else boxes[rows], d["props"][n, :c] if boxes is None else None,
                              d["hw"][n], CM.WEIGHTS, thr, mind, maxd, None if scales is None else scales[n], trace=trace)
        if regime is not None:
            CM.assert_regime(regime, trace, len(ref[0]), mind, maxd, R)
        refs.append((rows, ref, trace))
    for n, (rows, (ids, classes, probs, bx), trace) in enumerate(refs):
        k = len(ids)
        assert int(got["preds_per_image"][n]) == k, (n, int(got["preds_per_image"][n]), k, trace)
        np.testing.assert_array_equal(got["keep_ids"][n, :k].numpy(), ids.numpy())
        np.testing.assert_array_equal(got["obj_ids"][n, :k].numpy(), classes.numpy())
        np.testing.assert_array_equal(bits(got["obj_probs"][n, :k]), bits(probs))
        np.testing.assert_array_equal(bits(got["boxes"][n, :k]), bits(bx))
        np.testing.assert_array_equal(bits(got["roi_features"][n, :k]), bits(d["feats"][rows][ids]))
        if attr:
            np.testing.assert_array_equal(got["attr_ids"][n, :k].numpy(), ac[rows][ids].numpy())
            np.testing.assert_array_equal(bits(got["attr_probs"][n, :k]), bits(ap[rows][ids]))
        else:
            assert (got["attr_ids"][n, :k] == 0).all() and (got["attr_probs"][n, :k] == 0).all()
        for key in ("keep_ids", "obj_ids", "obj_probs", "boxes", "roi_features", "attr_ids", "attr_probs"):
            assert (got[key][n, k:] == 0).all(), (key, n)
    assert got["flag"] == 0
    return [ref[0] for _, ref, _ in refs]


@functools.lru_cache(maxsize=None)
def crafted(N, R, dups=True, counts=None, F=16):
    return CM.craft(N, R, CM.SEED.get(R, R), counts=None if counts is None else list(counts), F=F, dups=dups)


def regime_args(d, name):
    prob, cls, _, _ = device_softmax(d)
    counts = [CM.kept_counts(d, n, prob, cls, (0.05, 0.3, 0.7)) for n in range(d["N"])]
    return CM.regime(name, d["R"], *zip(*counts))


SCALES = [[1.25, 1.5], [2.0, 0.75], [0.5, 1.75]]


@pytest.mark.parametrize("name", CM.REGIMES)
@pytest.mark.parametrize("R", [255, 256, 257, 300, 1000, 1024])
def test_roi_outputs_regimes(R, name):
    """N = 2 at RoI counts around the workgroup's 256 threads and up to the kernel's 1024, every regime of the threshold loop,
    with scales_yx (retry, none) and without."""
    d = crafted(2, R, dups=name != "full")
    thr, mind, maxd = regime_args(d, name)
    scales = SCALES[:2] if name in ("retry", "none") else None
    ids = check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, scales=scales), thr, mind, maxd, scales=scales, regime=name)
    if name == "full":           # every row comes out, ranked; equal probabilities in row order
        for i in ids:
            assert sorted(i.tolist()) == list(range(R))
            assert i.tolist().index(CM.EQUAL[1]) == i.tolist().index(CM.EQUAL[0]) + 1
    else:                        # the copy of a row never comes out
        assert all(dst not in i.tolist() for i in ids for _, dst in CM.DUP)


@pytest.mark.parametrize("R", [1, 2])
def test_roi_outputs_one_and_two_rois(R):
    d = crafted(2, R)
    for thr, mind, maxd in (((0.05, 0.3, 0.9), 1, R), ((0.97,), R, R), ((0.05, 0.3), 1, 1)):
        check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, scales=SCALES[:2]), thr, mind, maxd, scales=SCALES[:2])


@pytest.mark.parametrize("dead", ["nan-inf", "winning"])
def test_roi_outputs_ragged_counts(dead):
    """counts = [300, 0, 123]: the rows >= counts[n] hold NaN logits and inf deltas and must neither rank nor flag.  A NaN row's
    probability comes out of the soft-max as -inf and would rank last anyhow, so the same again with dead rows that would win:
    probability 1 on a valid box."""
    d = crafted(3, 300, counts=(300, 0, 123))
    assert torch.isnan(d["logits"][300:600]).all() and torch.isinf(d["deltas"][723:]).all()
    if dead == "winning":
        d = {k: v for k, v in d.items() if k not in ("dev_sm", "last")}
        d["logits"], d["deltas"] = d["logits"].clone(), d["deltas"].clone()
        for n, c in enumerate(d["counts"]):
            rows = slice(n * 300 + int(c), (n + 1) * 300)
            d["logits"][rows], d["deltas"][rows] = 0.0, 0.0
            d["logits"][rows, 0] = 50.0
        assert float(device_softmax(d)[0][300:600].min()) == 1.0
    for thr, mind, maxd, scales in (((0.05, 0.3, 0.9), 50, 100, SCALES), ((0.97,), 300, 300, None)):
        ids = check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, scales=scales), thr, mind, maxd, scales=scales)
        assert len(ids[1]) == 0 and 0 < len(ids[2]) <= 123 and len(ids[0]) > 0


def test_roi_outputs_without_attributes_and_wide_features():
    """attr_logits NULL: the attribute outputs are zero.  F = 2048: the feature gather's strided loop runs twice per thread."""
    d = crafted(2, 300, F=2048)
    thr, mind, maxd = regime_args(d, "retry")
    check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, attr=False), thr, mind, maxd, attr=False, regime="retry")
    check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, scales=SCALES[:2]), thr, mind, maxd, scales=SCALES[:2], regime="retry")


def class_boxes(d, deltas):
    """vk_class_boxes: the device's own decode of every (row, class) box -> [K, C, 4] on the host."""
    dev = G.DEV
    dl, pr = deltas.to(dev).contiguous(), d["props"].to(dev)
    cn, hw = torch.from_numpy(d["counts"]).to(dev), torch.from_numpy(d["hw"]).to(dev)
    out = torch.full((d["N"] * d["R"], CM.C, 4), SENT, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("vk_class_boxes", G.P(dl), dl.shape[1], 0, G.P(pr), G.P(cn), d["N"], d["R"], CM.C, G.P(hw), (C.c_float * 4)(*CM.WEIGHTS),
           G.P(out), G.P(flag), G.stream())
    torch.cuda.synchronize()
    assert int(flag.cpu()) == 0
    return out.cpu()


def test_roi_outputs_general_size_deltas():
    """Deltas ~ N(0, 1) in all four columns, some beyond the log(1000 / 16) clamp: exp(dw) differs between expf and the
    host's exp in the last bit, so the restatement receives the device's own boxes (vk_class_boxes: the same apply_deltas_roi,
    held to the restatement of the decode by test_class_boxes_are_the_restatements)."""
    d = dict(crafted(2, 300))
    d.pop("last", None)
    g = torch.Generator().manual_seed(9)
    deltas = torch.randn(d["deltas"].shape, generator=g)
    deltas[torch.rand(deltas.shape, generator=g) < 0.02] = 25.0          # 25 / 5 = 5 > log(1000 / 16) = 4.135
    d["deltas"] = deltas
    boxes = class_boxes(d, deltas)
    assert float(boxes.max()) == 600.0 and float(boxes.min()) == 0.0
    for thr, mind, maxd in (((0.05, 0.3, 0.9), 50, 100), ((0.3, 0.5, 0.7), 280, 300)):
        check_exact(d, gpu_roi_outputs(d, thr, mind, maxd, scales=SCALES[:2]), thr, mind, maxd, scales=SCALES[:2], boxes=boxes)


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_F16], ids=["f32", "f16"])
def test_chosen_only_chain_as_the_model_runs_it(dt):
    """vk_softmax_argmax -> vk_chosen_deltas (integer data: exact) -> vk_roi_outputs(chosen_only = 1, ld_box = 4) against the
    same call given the full [K, 4C] matrix computed exactly on the host from the same integers: all outputs bit-identical.
    The regression weights are (160, 160, 80, 80), so that the integer deltas (sigma about 50) are shifts of about 0.3 of the
    box and size changes of about e^0.6."""
    d = dict(crafted(2, 300, dups=False))
    K, Fx, weights = 600, 100, (160.0, 160.0, 80.0, 80.0)
    w, b = integer_head(Fx, 4 * CM.C)
    x = torch.randint(-4, 5, (K, Fx), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
    _, cls, _, _ = device_softmax(d)
    chosen = chosen_deltas(x, Fx + 8, w, b, cls, K, dt)
    full = (x @ w.T + b).float()
    np.testing.assert_array_equal(chosen.numpy(), full.view(K, CM.C, 4)[torch.arange(K), cls].numpy())
    thr, mind, maxd = (0.05, 0.3, 0.9), 50, 100
    a = gpu_roi_outputs(d, thr, mind, maxd, scales=SCALES[:2], deltas=chosen, chosen_only=1, weights=weights)
    bb = gpu_roi_outputs(d, thr, mind, maxd, scales=SCALES[:2], deltas=full, chosen_only=0, weights=weights)
    assert a["flag"] == 0 and bb["flag"] == 0
    for k in a:
        if k != "flag":
            np.testing.assert_array_equal(a[k].numpy(), bb[k].numpy(), err_msg=k)
    n = a["preds_per_image"].tolist()
    assert all(0 < v <= 100 for v in n) and len(np.unique(a["boxes"][0, :n[0]].numpy(), axis=0)) > n[0] // 2


def test_nonfinite_flag():
    """The finite-ness the header of roi_out.hip documents: evaluated on the boxes that are used."""
    base = crafted(1, 37, counts=(30,))
    cls = device_softmax(base)[1].clamp(max=CM.C - 1)           # the dead rows' logits are NaN: their class is never read
    thr, mind, maxd = (0.3,), 1, 37
    run = lambda deltas, **kw: gpu_roi_outputs(base, thr, mind, maxd, deltas=deltas, **kw)["flag"]      # noqa: E731
    clean = base["deltas"].clone()
    assert run(clean) == 0
    c17, other = int(cls[17]), (int(cls[17]) + 1) % CM.C
    for v in (INF, -INF, NAN):
        bad = clean.clone()
        bad[17, 4 * c17 + 1] = v
        assert run(bad) == 1, v                               # the chosen class of a live row
        bad = clean.clone()
        bad[17, 4 * other + 1] = v
        assert run(bad) == 0, v                               # an unchosen class of a live row (chosen_only = 0)
        four = clean.view(37, CM.C, 4)[torch.arange(37), cls[:37]].clone()
        four[30:] = v
        assert run(four, chosen_only=1) == 0, v               # rows >= counts[n]
        four[29, 0] = v
        assert run(four, chosen_only=1) == 1, v               # the last live row
    assert torch.isinf(clean[30:]).all() and run(clean) == 0  # craft's own dead rows are inf, and NaN logits


@pytest.mark.parametrize("kw,thr,msg", [(dict(R=1025), (0.3,), "R=1025"), (dict(D=8), (0.3,), "max_detections"), (dict(F=18), (0.3,), "multiple of 4"),
                                        ({}, (), "thresholds")], ids=["R1025", "max_detections>R", "F%4", "no-threshold"])
def test_roi_outputs_refuses_before_it_writes(kw, thr, msg):
    """VK_EINVAL, and every output still holds the sentinel.  The buffers are sized for what the call is told."""
    if kw.get("R") == 1025:
        d = dict(crafted(1, 37))
        pad = lambda t, v: torch.cat([t, torch.full((1025 - 37,) + t.shape[1:], v)], 0)      # noqa: E731
        d.update(logits=pad(d["logits"], 0.0), attr=pad(d["attr"], 0.0), deltas=pad(d["deltas"], 0.0), feats=pad(d["feats"], 0.0),
                 props=torch.cat([d["props"], torch.zeros((1, 1025 - 37, 4))], 1))
    elif "F" in kw:
        d = dict(crafted(1, 37))
        d["feats"] = torch.zeros((37, 20))                    # told F = 18
    elif "D" in kw:
        d = dict(crafted(1, 4))                               # max_detections = 8 > R = 4
    else:
        d = dict(crafted(1, 37))
    with pytest.raises(ValueError, match=msg):
        gpu_roi_outputs(d, thr, 1, kw.get("D", 4), **{k: v for k, v in kw.items() if k != "D"})
    got = d["last"]
    for k in OUT_KEYS + ("keep_ids",):
        assert (got[k] == (SENT if got[k].dtype.is_floating_point else -7)).all(), k
    assert got["flag"] == 0
