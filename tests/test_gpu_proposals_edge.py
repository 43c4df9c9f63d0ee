"""-m gpu: the proposal stage (csrc/rpn.hip) at its edges -- top-k selection, level merge, size filter, post-NMS cap and NMS.

The older stage tests read the stage through the <= 300 boxes that survive NMS, a few hundred candidates deep.  Here the entry
points run with nms_thresh = 2.0 and post_nms_topk = pre_nms_topk, so the output IS the selection: every selected candidate
that passed the size filter, in rank order, with out_counts their number.  The inputs are exact (tests/proposals_util.py), so
boxes, logits and counts are compared with assert_array_equal against the oracle; a bit-equal box says which anchor was taken,
which equal logits of a tie class cannot.  The only tolerance in this file is the stage's 2e-6 box-decode bound
(tests/test_gpu_stages.py) on the one case with free-running deltas.

Every selection case asserts that it is not vacuous, on the oracle's side: something is selected, and for the regimes made
for it the class of logits equal to the selection threshold is larger than the number taken from it (SEEDS below: the
generator keys for which that holds, checked on the CPU).  test_zz_report prints what was exercised."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fpn_oracle as fo             # noqa: E402
from oracle import frcnn_oracle as orc          # noqa: E402

import gpu_util as G                            # noqa: E402
import proposals_util as U                      # noqa: E402

REPORT = []                                     # (case, image, regime, HWA, K, threshold class, taken from it)


def _bits_zero(t):
    return not np.ascontiguousarray(t.numpy()).view(np.int32).any()


def _compare_image(n, rb, rl, ob, ol, oc, exact):
    cnt = int(oc[n])
    assert cnt == len(rl), (n, cnt, len(rl))
    np.testing.assert_array_equal(ol[n, :cnt].numpy(), rl.numpy())
    if exact:
        np.testing.assert_array_equal(ob[n, :cnt].numpy(), rb.numpy())
    else:
        assert G.rel_err(ob[n, :cnt], rb) <= 2e-6
    assert torch.isfinite(ob[n, :cnt]).all() and not torch.isnan(ol[n, :cnt]).any()
    assert _bits_zero(ob[n, cnt:]) and _bits_zero(ol[n, cnt:])


def _compare(ref, ob, ol, oc, exact=True, labels=None):
    """Per image: count, logits and boxes equal to the oracle's; the rows behind the count are zero bits (the outputs were
    pre-filled with NaN), the rows before it hold finite boxes.  Every image is looked at; the failure names them all."""
    bad = []
    for n, (rb, rl) in enumerate(ref):
        try:
            _compare_image(n, rb, rl, ob, ol, oc, exact)
        except AssertionError as e:
            bad.append(f"image {n} ({labels[n] if labels else ''}): {str(e).strip()[:600]}")
    assert not bad, "\n".join(bad)


def check_selection(c, expect_empty=None, **call_kw):
    """One single-level call on exact data against the oracle, with the case's non-vacuity conditions."""
    ref = c.oracle()
    ob, ol, oc, flag = U.rpn_call(*c.oracle_layout(), nan_fill=True, **c.kw(), **call_kw)
    assert flag == 0
    _compare(ref, ob, ol, oc, labels=c.regimes)
    empty = tuple(n for n in range(c.N) if len(ref[n][1]) == 0)
    assert len(empty) < c.N and (expect_empty is None or empty == tuple(expect_empty))      # (pre = 1 may pick a filtered box)
    for n, regime in enumerate(c.regimes):
        cls, taken = U.tie_stats(c.logits[n].reshape(-1), c.K)
        REPORT.append((c.name, n, regime, c.HWA, c.K, cls, taken))
        if regime in U.TIE_REGIMES and c.K < c.HWA:
            assert cls > taken, (c.name, n, regime, cls, taken)     # the threshold cuts a tie class: the index rule decides
    return ref, (ob, ol, oc)


# ---- selection, single level ------------------------------------------------------------------------------------------------
SIZES = [(1, 1, 1), (3, 7, 3), (32, 32, 1), (5, 41, 5), (1, 8191, 1), (64, 128, 1), (1, 2731, 3), (1, 683, 15)]
PRES = [1, 64, 65, 1000, 8192]
EXTRA_REGIMES = {           # beside continuous and quantised, which run at every size
    1: ["signs_specials"],
    63: ["all_equal", "two_values", "signs_specials"],
    1024: ["low_byte", "all_negative"],
    1025: ["all_equal", "two_values", "low_byte", "second_byte", "signs_specials", "all_negative"],
    8191: ["two_values", "second_byte"],
    8192: ["all_equal", "low_byte", "second_byte"],
    8193: ["two_values", "low_byte", "signs_specials"],
    10245: ["all_equal", "two_values", "low_byte", "all_negative"],
}
# (case, image) -> generator key, where the default key 0 leaves the threshold class no larger than what is taken from it
SEEDS = {('sel-3x7x3-pre1', 1): 1, ('sel-32x32x1-pre1', 1): 1, ('sel-32x32x1-pre1000', 2): 1, ('sel-64x128x1-pre1', 1): 1,
         ('sel-1x2731x3-pre8192', 1): 2}


def _shapes(N, Hf, Wf, stride):
    cuts = [(5, 11), (-30, -30), (17, 3), (2, 40)]             # inside the anchor grid's extent, beyond it, inside again
    return [U.cut_shape(Hf, Wf, stride, cuts[i % len(cuts)]) for i in range(N)]


def size_case(size, pre, regimes=None, tag="sel", **kw):
    Hf, Wf, A = size
    if regimes is None:
        regimes = ["continuous", "quantised"] + EXTRA_REGIMES[Hf * Wf * A]
        if min(pre, Hf * Wf * A) > 8000:
            regimes = regimes[:3]                   # (the oracle's NMS at thr = 2.0 is 8192^2 IoUs per image)
    stride = kw.pop("stride", 4)
    name = f"{tag}-{Hf}x{Wf}x{A}-pre{pre}"
    return U.SelCase(name, Hf, Wf, A, pre, regimes, _shapes(len(regimes), Hf, Wf, stride), stride=stride,
                     seeds=SEEDS, **kw)


@pytest.mark.parametrize("pre", PRES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_selection_at_the_sweep_and_round_edges(size, pre):
    """HWA around the 1024-thread compaction round and the 8 x 1024 unrolled histogram sweep with its tail, K = min(pre, HWA) on
    both sides of HWA; one image per logit regime in one call, each with its own image size."""
    check_selection(size_case(size, pre))


@pytest.mark.parametrize("size,pre", [((3, 7, 3), 64), ((5, 41, 5), 8192), ((1, 2731, 3), 1000)], ids=["63<64", "1025<8192", "8193>1000"])
def test_three_images_three_regimes(size, pre):
    """The candidate arrays are strided by pre_topk while K = min(pre, HWA) slots are written per image."""
    c = size_case(size, pre, regimes=["quantised", "all_equal", "signs_specials"], tag="three")
    assert c.N == 3 and len({tuple(s) for s in c.shapes}) == 3
    check_selection(c)


@pytest.mark.parametrize("variant", ["interleaved", "offset_half", "stride8", "stride32", "weights", "all"])
def test_selection_layout_and_parameters(variant):
    kw, call = {}, {}
    if variant in ("interleaved", "all"):
        call["interleaved"] = True                 # ld_logits = ld_deltas = 5A, deltas at +A
    if variant in ("offset_half", "all"):
        kw["offset"] = 0.5
    if variant in ("weights", "all"):
        kw["weights"] = (2.0, 4.0, 2.0, 4.0)
    kw["stride"] = {"stride8": 8, "stride32": 32, "all": 8}.get(variant, 4)
    check_selection(size_case((5, 41, 5), 1000, regimes=["quantised", "continuous", "two_values"], tag=variant, **kw), **call)
    check_selection(size_case((3, 7, 3), 64, regimes=["quantised", "all_equal"], tag=variant, **kw), **call)


# ---- size filter ----------------------------------------------------------------------------------------------------------------
FILTER_SIDES = [(16, 16), (8, 32), (32, 8), (24, 24)]


def _filter_case(min_size, name="filter", shapes=None):
    Hf, Wf, A = 12, 14, 4
    shapes = [[Hf * 8 + 40, Wf * 8 + 40], U.cut_shape(Hf, Wf, 8, (20, 30))] if shapes is None else shapes
    return U.SelCase(name, Hf, Wf, A, 400, ["quantised"] * len(shapes), shapes, stride=8, min_size=min_size,
                     cells=U.exact_cells(A, FILTER_SIDES))


def test_size_filter_is_strict():
    """dw = dh = 0: an unclipped box is as wide as its anchor.  min_size equal to a side drops it (strict >); one f32 below
    keeps it.  Image 0 reaches beyond the anchor grid (boxes are clipped at 0 only), image 1 ends inside it."""
    at, below = np.float32(16.0), np.nextafter(np.float32(16.0), np.float32(0.0))
    ref, _ = check_selection(_filter_case(float(at)))
    c = _filter_case(float(below))                          # the same logits and deltas
    ref2, _ = check_selection(c)
    for n in range(2):
        sides = lambda b: torch.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)      # noqa: E731
        assert len(ref[n][0]) > 20 and not (sides(ref[n][0]) == 16).any()               # a side of exactly min_size: dropped
        both = (sides(ref2[n][0]) == 16).all(1)
        assert both.sum() > 10                                                          # kept: the 16 x 16 anchors among them
        assert len(ref2[n][0]) == len(ref[n][0]) + int((sides(ref2[n][0]) == 16).any(1).sum())
    # image 1: candidates whose anchor passes the filter and whose clipped box does not
    idx, b, _, valid = c.restatement(1)
    side_ok = np.isin(idx % 4, [0, 3])
    assert (side_ok & ~valid).sum() > 0 and (side_ok & valid).sum() > 0


def test_an_image_with_every_candidate_filtered():
    shapes = [U.cut_shape(12, 14, 8), [1, 1], U.cut_shape(12, 14, 8, (3, 7))]
    ref, (ob, ol, oc) = check_selection(_filter_case(2.0, "filter-empty-image", shapes), expect_empty=(1,))
    assert oc.tolist()[1] == 0 and oc.tolist()[0] > 100 and oc.tolist()[2] > 100


# ---- non-finite flag --------------------------------------------------------------------------------------------------------------
def test_nonfinite_flag_looks_at_selected_candidates_only():
    c = U.SelCase("flag", 6, 7, 1, 10, ["continuous"], [[60, 70]], stride=8)
    order = orc.argsort_desc(torch.from_numpy(c.logits[0].reshape(-1))).numpy()
    keep = c.deltas.copy()
    c.deltas.reshape(-1, 4)[order[20], 0] = np.inf            # rank 20 of 42, outside the top 10
    check_selection(c)                                        # flag 0, and the oracle's rows
    c.deltas = keep.copy()
    c.deltas.reshape(-1, 4)[order[3], 0] = np.inf             # the same delta on a selected anchor
    _, _, _, flag = U.rpn_call(*c.oracle_layout(), nan_fill=True, **c.kw())
    assert flag == 1


# ---- free-running decode ------------------------------------------------------------------------------------------------------------
def test_free_running_deltas_and_the_scale_clamp():
    """The one case off exact data: logits and counts exact, boxes within the stage's box-decode bound of 2e-6."""
    g = U.rng_for("free")
    N, A, Hf, Wf, pre = 2, 15, 20, 25, 1000
    lg = np.stack([U.regime_logits("quantised", Hf * Wf * A, "free", n).reshape(Hf, Wf, A) for n in range(N)])
    d = (g.standard_normal((N, Hf, Wf, A, 4)) * 0.5).astype(np.float32)
    big = g.random((N, Hf, Wf, A, 2)) < 0.1
    d[..., 2:][big] = g.uniform(4.2, 6.0, int(big.sum())).astype(np.float32)        # beyond log(1000/16) = 4.135
    obj, dlt = U.to_oracle_layout(lg, d)
    from vltk_amd.weights import cell_anchors
    cell = cell_anchors([32, 64, 128, 256, 512], [0.5, 1.0, 2.0])
    shapes = [[320, 400], [300, 390]]
    ref = U.StageOracle(cell, pre, pre, U.NO_SUPPRESSION).rpn_proposals(obj, dlt, shapes)
    ob, ol, oc, flag = U.rpn_call(obj, dlt, shapes, cell, pre, pre, U.NO_SUPPRESSION, nan_fill=True)
    assert flag == 0 and min(len(r[1]) for r in ref) > 500
    sel = [orc.argsort_desc(torch.from_numpy(lg[n].reshape(-1))).numpy()[:pre] for n in range(N)]
    assert all((d[n].reshape(-1, 4)[sel[n], 2:] > 4.2).sum() > 50 for n in range(N))       # clamped scales among the selected
    _compare(ref, ob, ol, oc, exact=False)


# ---- post-NMS cap -------------------------------------------------------------------------------------------------------------------
FILTERED_RANKS = (63, 130, 700)


def _cap_case(post):
    """26 x 40 anchors of 8 x 8, distinct logits: rank r is ours to place.  The image ends before the last column, whose boxes
    clip to nothing; three of them sit at FILTERED_RANKS (63: the last slot of the first 64-box chunk), the rest behind pre."""
    Hf, Wf, pre = 26, 40, 1000
    c = U.SelCase(f"cap-post{post}", Hf, Wf, 1, pre, ["continuous"], [[Hf * 16 + 20, (Wf - 1) * 16 - 6]], stride=16,
                  cells=U.exact_cells(1, [(8, 8)]), post=post)
    flat = np.arange(Hf * Wf)
    gone = flat[flat % Wf == Wf - 1]
    rest = U.rng_for("cap").permutation(flat[flat % Wf != Wf - 1])
    ranks = list(rest)
    for i, r in enumerate(FILTERED_RANKS):
        ranks.insert(r, gone[i])
    ranks += list(gone[len(FILTERED_RANKS):])
    lg = np.empty(Hf * Wf, np.float32)
    lg[np.asarray(ranks)] = 2000.0 - np.arange(Hf * Wf)
    c.logits = lg.reshape(1, Hf, Wf, 1)
    return c


@pytest.mark.parametrize("lead", [None, "64"], ids=["one_phase", "lead64"])
@pytest.mark.parametrize("post", [1, 62, 63, 64, 65, 1000])
def test_post_nms_cap(monkeypatch, post, lead):
    """thr = 2.0: the output is the first `post` valid candidates.  63 valid ones fill the first chunk: post = 63 ends the
    sweep exactly at the chunk's end, 62 inside it, 64 and 65 inside the next one.  With VK_NMS_LEAD = 64 the first phase
    sees one chunk, and the second must finish the sweep when the cap was not reached."""
    if lead is not None:
        monkeypatch.setenv("VK_NMS_LEAD", lead)
    c = _cap_case(post)
    ref, (ob, ol, oc) = check_selection(c)
    valid_logits = [2000.0 - r for r in range(c.pre) if r not in FILTERED_RANKS]
    assert int(oc[0]) == min(post, c.pre - len(FILTERED_RANKS))
    np.testing.assert_array_equal(ol[0, :int(oc[0])].numpy(), np.asarray(valid_logits[:post], np.float32))


# ---- NMS proper -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    return U.chain_boxes(8192), U.chain_scores(8192)


@pytest.mark.parametrize("thr,step", [(0.4, 2), (0.5, 1), (0.19, 3)])
def test_nms_chain(chain, thr, step):
    """n = 8192: 128 mask words, every thread of the sweep owns one.  Neighbours have IoU exactly 1/2: 0.5 suppresses nothing."""
    np.testing.assert_array_equal(U._nms_gpu(*chain, thr), np.arange(0, 8192, step))


@pytest.mark.parametrize("lead", ["0", "64"])
def test_nms_chain_two_phases(monkeypatch, chain, lead):
    """With VK_NMS_LEAD = 64 the second phase rebuilds a sweep that keeps boxes in every one of the 128 chunks."""
    monkeypatch.setenv("VK_NMS_LEAD", lead)
    np.testing.assert_array_equal(U._nms_gpu(*chain, 0.4), np.arange(0, 8192, 2))


def test_nms_chain_with_permuted_scores(chain):
    boxes, _ = chain
    scores = U.chain_scores(8192)[U.rng_for("chain-perm").permutation(8192)]
    got = U._nms_gpu(boxes, scores, 0.4)
    np.testing.assert_array_equal(got, orc.nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.4).numpy())
    np.testing.assert_array_equal(got, U.greedy_nms(boxes, scores, 0.4))


def test_nms_iou_at_equality():
    s = np.array([2, 1], np.float32)
    np.testing.assert_array_equal(U._nms_gpu(U.THIRD_BOXES, s, 1 / 3), [0])                   # f32(1/3) > 1/3 as doubles
    np.testing.assert_array_equal(U._nms_gpu(U.THIRD_BOXES, s, U.THIRD_AS_F32), [0, 1])       # equal: not suppressed


def test_nms_degenerate_and_duplicate_boxes():
    np.testing.assert_array_equal(U._nms_gpu(U.DEGENERATE_BOXES, U.DEGENERATE_SCORES, 0.5), U.DEGENERATE_KEPT)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 127, 128, 129, 8191, 8192])
def test_nms_at_chunk_edges(n):
    boxes, scores = U.clustered_boxes(U.rng_for("clustered", n), n)
    ref = orc.nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.5).numpy()
    assert 0 < len(ref) <= n and (n < 63 or len(np.unique(scores)) < n / 2)   # score ties among the boxes
    np.testing.assert_array_equal(U._nms_gpu(boxes, scores, 0.5), ref)
    if n <= 129:
        np.testing.assert_array_equal(ref, U.greedy_nms(boxes, scores, 0.5))


# ---- RPN with real suppression on tied data -------------------------------------------------------------------------------------------
def test_rpn_suppression_on_tied_logits():
    """thr 0.7, pre = post = 1000 on 7500 anchors: survivors hundreds of candidates deep, boxes bit-equal."""
    c = U.SelCase("suppress", 20, 25, 15, 1000, ["quantised", "quantised"], [[315, 389], [320, 400]], stride=16, thr=0.7)
    ref, (ob, ol, oc) = check_selection(c)
    for n in range(2):
        assert 300 < int(oc[n]) < 1000                                         # NMS did suppress, and the kept set runs deep
        idx, b, lg, valid = c.restatement(n)
        kept = U.greedy_nms(b[valid], -np.arange(int(valid.sum()), dtype=np.float32), 0.7)     # already in rank order
        np.testing.assert_array_equal(ob[n, :int(oc[n])].numpy(), b[valid][kept])


# ---- several levels -------------------------------------------------------------------------------------------------------------------
ML_MAPS, ML_STRIDES, ML_A, ML_PRE = [(16, 20), (8, 10), (4, 5)], [4, 8, 16], 3, 200
ML_SIDES = [[(8, 16), (16, 8), (13, 13)], [(16, 32), (32, 16), (21, 21)], [(32, 64), (64, 32), (37, 37)]]
ML_SHAPES = [[60, 75], [64, 80]]


def ml_inputs(name, regime="quantised", N=2, sides=ML_SIDES):
    lgs, ds = [], []
    for l, (h, w) in enumerate(ML_MAPS):
        lgs.append(np.stack([U.regime_logits(regime, h * w * ML_A, name, l, n).reshape(h, w, ML_A) for n in range(N)]))
        ds.append(U.exact_deltas(U.rng_for("ml-deltas", name, l), N, h, w, ML_A))
    return lgs, ds, [U.exact_cells(ML_A, s) for s in sides]


def check_ml(name, lgs, ds, cells, shapes, post, thr, min_size=0.0, expect_empty=(), **call_kw):
    pairs = [U.to_oracle_layout(lg, d) for lg, d in zip(lgs, ds)]
    objs, dlts = [p[0] for p in pairs], [p[1] for p in pairs]
    ref = fo.multilevel_proposals(objs, dlts, cells, ML_STRIDES, shapes, ML_PRE, post, thr, min_size)
    ob, ol, oc, flag = U.ml_call(objs, dlts, cells, ML_STRIDES, shapes, ML_PRE, post, thr, min_size, nan_fill=True, **call_kw)
    assert flag == 0
    _compare(ref, ob, ol, oc)
    for n in range(len(shapes)):
        assert (len(ref[n][1]) == 0) == (n in expect_empty)
        sel = []
        for l, lg in enumerate(lgs):
            v = lg[n].reshape(-1)
            K = min(ML_PRE, len(v))
            sel.append(set(v[orc.argsort_desc(torch.from_numpy(v)).numpy()[:K]].tolist()))
            cls, taken = U.tie_stats(v, K)
            REPORT.append((f"{name}-level{l}", n, "quantised", len(v), K, cls, taken))
            assert K == len(v) or cls > taken
        assert sel[0] & sel[1] & sel[2]                   # logit values selected on every level: ties cross levels
    return ref, (ob, ol, oc)


def test_multilevel_selection_and_merge():
    """thr = 2.0, post = levels * pre: the merge's whole order (logit descending, ties by concat index, level-major) comes out.
    The last level has HWA = 60 < pre."""
    assert ML_MAPS[2][0] * ML_MAPS[2][1] * ML_A == 60 < ML_PRE
    lgs, ds, cells = ml_inputs("ml-merge")
    ref, (_, _, oc) = check_ml("ml-merge", lgs, ds, cells, ML_SHAPES, 3 * ML_PRE, U.NO_SUPPRESSION)
    assert min(oc.tolist()) > 400


def test_multilevel_with_a_level_wholly_filtered():
    """Level 0's anchors are 3 x 3 and 2 x 5 under min_size = 5: none of its 200 candidates reaches the merge."""
    sides = [[(3, 3), (2, 5), (5, 2)]] + ML_SIDES[1:]
    lgs, ds, cells = ml_inputs("ml-level-out", sides=sides)
    ref, (ob, ol, oc) = check_ml("ml-level-out", lgs, ds, cells, ML_SHAPES, 3 * ML_PRE, U.NO_SUPPRESSION, min_size=5.0)
    for n in range(2):
        assert 0 < int(oc[n]) <= ML_PRE + 60
        w = ob[n, :int(oc[n]), 2] - ob[n, :int(oc[n]), 0]
        assert (w > 5).all()


def test_multilevel_with_an_image_without_candidates():
    lgs, ds, cells = ml_inputs("ml-empty")
    ref, (_, _, oc) = check_ml("ml-empty", lgs, ds, cells, [[1, 1], [64, 80]], 3 * ML_PRE, U.NO_SUPPRESSION, min_size=2.0,
                               expect_empty=(0,))
    assert oc.tolist()[0] == 0 and oc.tolist()[1] > 400


def test_multilevel_level_offset_keeps_levels_apart():
    """thr 0.7: the same box with the same logit on two levels -- both survive (the NMS runs on boxes shifted per level), in
    level order; a duplicate inside one level would not."""
    sides = [[(16, 16), (16, 8), (13, 13)], [(16, 16), (32, 16), (21, 21)], ML_SIDES[2]]
    lgs, ds, cells = ml_inputs("ml-offset", sides=sides)
    for n in range(2):
        lgs[0][n, 4, 4, 0] = lgs[1][n, 2, 2, 0] = 50.0        # level 0 (stride 4) cell (4, 4) and level 1 (stride 8) cell (2, 2)
        ds[0][n, 4, 4, 0] = ds[1][n, 2, 2, 0] = 0.0           # both centred on (16, 16)
    ref, (ob, ol, oc) = check_ml("ml-offset", lgs, ds, cells, ML_SHAPES, 3 * ML_PRE, 0.7)
    for n in range(2):
        np.testing.assert_array_equal(ob[n, :2].numpy(), np.array([[8, 8, 24, 24]] * 2, np.float32))
        np.testing.assert_array_equal(ol[n, :2].numpy(), np.array([50, 50], np.float32))
        assert 2 < int(oc[n]) < 460                           # and the NMS did suppress


# ---- the ignorey instantiations of the same body ----------------------------------------------------------------------------------------
def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert not torch.isnan(x.float()).any()
        np.testing.assert_array_equal(x.numpy(), y.numpy())
    assert a[3] == b[3] == 0


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_ignorey_kernels_select_like_the_plain_ones(f64):
    """One band per image that no box reaches (above every box: neither dropped nor trimmed): the _bands<float|double> forms
    of the selection body must return what the plain entry points return, bit for bit."""
    c = size_case((5, 41, 5), 1000, regimes=["quantised", "quantised", "two_values"], tag="ignorey")
    plain = U.rpn_call(*c.oracle_layout(), nan_fill=True, **c.kw())
    assert int(plain[2].min()) > 500
    _same(U.rpn_call(*c.oracle_layout(), nan_fill=True, bands=[U.NOOP_BAND] * c.N, bands_f64=f64, **c.kw()), plain)
    check_selection(c, bands=[U.NOOP_BAND] * c.N, bands_f64=f64)
    lgs, ds, cells = ml_inputs("ml-ignorey")
    pairs = [U.to_oracle_layout(lg, d) for lg, d in zip(lgs, ds)]
    args = ([p[0] for p in pairs], [p[1] for p in pairs], cells, ML_STRIDES, ML_SHAPES, ML_PRE, 3 * ML_PRE, U.NO_SUPPRESSION)
    plain = U.ml_call(*args, nan_fill=True)
    assert int(plain[2].min()) > 400
    _same(U.ml_call(*args, nan_fill=True, bands=[U.NOOP_BAND] * 2, bands_f64=f64), plain)
    check_ml("ml-ignorey", lgs, ds, cells, ML_SHAPES, 3 * ML_PRE, U.NO_SUPPRESSION, bands=[U.NOOP_BAND] * 2, bands_f64=f64)


def test_zz_report(capsys):
    """Not a check of its own: prints, once, what the selection cases above exercised."""
    with capsys.disabled():
        print("\n[proposals edge] case, image, regime: HWA, K, threshold class, taken from it")
        for name, n, regime, hwa, K, cls, taken in dict.fromkeys(REPORT):
            print(f"[proposals edge]   {name:28s} {n} {regime:15s} {hwa:6d} {K:5d} {cls:6d} {taken:6d}")
        cut = sum(1 for r in set(REPORT) if r[5] > r[6])
        print(f"[proposals edge] {len(set(REPORT))} selections, {cut} with a threshold class larger than what is taken from it")
