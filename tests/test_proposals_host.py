"""CPU (-m "not gpu"): the proposal stage's second reference against the oracle, the hand-built NMS expectations as literals,
and the refusals of vk_rpn_proposals* / vk_nms through the C ABI (every one of them is decided before the device is touched).
The GPU side of the same cases is tests/test_gpu_proposals_edge.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as orc
from vltk_amd import _lib as L

import proposals_util as U
from ignorey_util import band_restatement

SMALL_SIZES = [(1, 1, 1), (3, 7, 3), (7, 9, 15)]                  # HWA 1, 63, 945


# ---- the restatement against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("regime", list(U.REGIMES))
def test_restatement_matches_the_oracle(regime, size):
    """thr = 2.0, post = pre: the oracle returns the selected candidates that pass the size filter, in rank order; the numpy
    restatement must give the same rows bit for bit (exact data: see proposals_util)."""
    Hf, Wf, A = size
    for pre, min_size, offset, weights in ((400, 0.0, 0.0, (1, 1, 1, 1)), (50, 4.0, 0.5, (2, 4, 2, 4)), (1, 0.0, 0.0, (1, 1, 1, 1))):
        c = U.SelCase(f"host-{regime}-{size}-{pre}", Hf, Wf, A, pre, [regime, regime], [U.cut_shape(Hf, Wf, 8), [Hf * 8 + 40, Wf * 8 + 40]],
                      stride=8, offset=offset, weights=weights, min_size=min_size)
        ref = c.oracle()
        for n in range(c.N):
            idx, b, lg, valid = c.restatement(n)
            assert len(idx) == c.K == min(pre, c.HWA)
            np.testing.assert_array_equal(ref[n][0].numpy(), b[valid])
            np.testing.assert_array_equal(ref[n][1].numpy(), lg[valid])
            cls, taken = U.tie_stats(c.logits[n].reshape(-1), c.K)
            assert 1 <= taken <= cls
            if regime in ("all_equal", "two_values") and c.K < c.HWA and c.K != min(c.HWA // 3, 40):
                assert cls > taken                                   # by construction: the threshold cuts a tie class
            if regime == "all_equal":
                np.testing.assert_array_equal(idx, np.arange(c.K))   # the first K flat indices win


def test_restatement_orders_signed_zeros_by_index():
    v = np.array([-0.0, 0.0, 1e-40, -0.0, -1e-40, 0.0, np.inf, -np.inf], np.float32)
    np.testing.assert_array_equal(U.stable_desc_order(v), [6, 2, 0, 1, 3, 5, 4, 7])
    np.testing.assert_array_equal(orc.argsort_desc(torch.from_numpy(v)).numpy(), [6, 2, 0, 1, 3, 5, 4, 7])


def test_a_band_above_every_box_is_a_no_op():
    """The band the GPU ignorey cases use (the reference's box_ignore_above case): no box dropped, none trimmed.  A band
    below the boxes would not do: the reference trims every box that is not above a band."""
    c = U.SelCase("host-band", 7, 9, 15, 400, ["quantised"], [U.cut_shape(7, 9, 8)], stride=8)
    _, b, _, _ = c.restatement(0)
    for dt in (torch.float32, torch.float64):
        out, keep = band_restatement(torch.from_numpy(b), torch.tensor(U.NOOP_BAND, dtype=dt))
        assert keep.all() and torch.equal(out, torch.from_numpy(b))
    out, _ = band_restatement(torch.from_numpy(b), torch.tensor([[1e6, 1e6 + 10]]))
    assert not torch.equal(out, torch.from_numpy(b))


# ---- NMS: hand-built sets, expectations as literals ---------------------------------------------------------------------------
def _both(boxes, scores, thr):
    a = orc.nms(torch.from_numpy(boxes), torch.from_numpy(scores), thr).numpy()
    b = U.greedy_nms(boxes, scores, thr)
    np.testing.assert_array_equal(a, b)
    return a


@pytest.fixture(scope="module")
def chain():
    return U.chain_boxes(8192), U.chain_scores(8192)


def test_chain_neighbours_have_iou_one_half(chain):
    b = chain[0]
    f = np.float32
    assert U.iou_f32(b[0], b[1]) == f(0.5) and U.iou_f32(b[8000], b[8001]) == f(0.5) and U.iou_f32(b[8190], b[8191]) == f(0.5)
    assert U.iou_f32(b[0], b[2]) == f(1) / f(5) and U.iou_f32(b[0], b[3]) == 0
    assert U.iou_f32(*U.THIRD_BOXES) == f(1) / f(3)
    assert np.isnan(U.iou_f32(U.DEGENERATE_BOXES[0], U.DEGENERATE_BOXES[1])) and U.iou_f32(U.DEGENERATE_BOXES[2], U.DEGENERATE_BOXES[3]) == 1


def test_chain_kept_sets(chain):
    boxes, scores = chain
    np.testing.assert_array_equal(_both(boxes, scores, 0.4), np.arange(0, 8192, 2))          # 4096 kept
    np.testing.assert_array_equal(_both(boxes, scores, 0.5), np.arange(8192))                # equality does not suppress
    k = _both(boxes, scores, 0.19)
    np.testing.assert_array_equal(k, np.arange(0, 8192, 3))
    assert len(k) == 2731


def test_chain_with_permuted_scores(chain):
    boxes, _ = chain
    scores = U.chain_scores(8192)[U.rng_for("chain-perm").permutation(8192)]
    k = _both(boxes, scores, 0.4)
    assert 2731 <= len(k) <= 4096 and len(set(k.tolist())) == len(k)


def test_iou_of_one_third_at_equality():
    s = np.array([2, 1], np.float32)
    assert U.THIRD_AS_F32 > 1 / 3                                    # f32(1/3) rounds up
    np.testing.assert_array_equal(_both(U.THIRD_BOXES, s, 1 / 3), [0])                       # f32(1/3) > 1/3 as doubles
    np.testing.assert_array_equal(_both(U.THIRD_BOXES, s, U.THIRD_AS_F32), [0, 1])           # equal: not suppressed


def test_degenerate_and_duplicate_boxes():
    np.testing.assert_array_equal(_both(U.DEGENERATE_BOXES, U.DEGENERATE_SCORES, 0.5), U.DEGENERATE_KEPT)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 1000])
def test_greedy_nms_matches_the_oracle_on_clustered_boxes(n):
    boxes, scores = U.clustered_boxes(U.rng_for("clustered", n), n)
    k = _both(boxes, scores, 0.5)
    assert 0 < len(k) <= n


# ---- refusals, on the CPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


FAKE = C.c_void_p(0x1000)                                          # never dereferenced: every case is refused first


def _rpn(lib, pre, post, ws_bytes=None, N=1, Hf=4, Wf=4, A=1):
    ws = lib.vk_rpn_workspace_bytes(N, Hf * Wf * A, pre) if ws_bytes is None else ws_bytes
    st = lib.vk_rpn_proposals(FAKE, A, FAKE, 4 * A, N, Hf, Wf, A, FAKE, 16, 0.0, FAKE, (C.c_float * 4)(1, 1, 1, 1), 0.0, 0.7, pre, post,
                              FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    return st, lib.vk_last_error().decode()


def _ml(lib, levels, pre, post, ws_bytes=None, N=1):
    nl = max(levels, 1)
    ptrs = (C.c_void_p * nl)(*([0x1000] * nl))
    ints = (C.c_int32 * nl)(*([4] * nl))
    ws = lib.vk_rpn_multilevel_workspace_bytes(N, levels, pre, post) if ws_bytes is None else ws_bytes
    st = lib.vk_rpn_proposals_multilevel(ptrs, ints, ptrs, ints, levels, N, ints, ints, 1, ptrs, ints, 0.0, FAKE, (C.c_float * 4)(1, 1, 1, 1),
                                         0.0, 0.7, pre, post, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    return st, lib.vk_last_error().decode()


@pytest.mark.parametrize("pre,post,msg", [
    (0, 1, "rpn: pre_nms_topk=0 must be in 1..8192"),
    (8193, 1, "rpn: pre_nms_topk=8193 must be in 1..8192"),
    (16, 0, "rpn: post_nms_topk=0 must be in 1..pre_nms_topk"),
    (16, 17, "rpn: post_nms_topk=17 must be in 1..pre_nms_topk"),
])
def test_rpn_refuses_bad_topk(lib, pre, post, msg):
    st, err = _rpn(lib, pre, post, ws_bytes=1 << 30)
    assert st == L.VK_EINVAL and err == msg


def test_rpn_refuses_a_short_workspace(lib):
    need = lib.vk_rpn_workspace_bytes(2, 16, 16)
    st, err = _rpn(lib, 16, 16, ws_bytes=need - 1, N=2)
    assert st == L.VK_EINVAL and err == f"rpn: workspace too small ({need - 1} < {need})"


@pytest.mark.parametrize("levels,pre,post,msg", [
    (0, 16, 8, "rpn_ml: 1..6 levels"),
    (7, 16, 8, "rpn_ml: 1..6 levels"),
    (3, 2731, 8, "rpn_ml: levels * pre_nms_topk = 8193 must be in 1..8192"),
    (3, 0, 8, "rpn_ml: levels * pre_nms_topk = 0 must be in 1..8192"),
    (3, 16, 0, "rpn_ml: post_nms_topk=0 out of range"),
    (3, 16, 49, "rpn_ml: post_nms_topk=49 out of range"),
])
def test_multilevel_refuses_bad_sizes(lib, levels, pre, post, msg):
    st, err = _ml(lib, levels, pre, post, ws_bytes=1 << 30)
    assert st == L.VK_EINVAL and err == msg


def test_multilevel_refuses_a_short_workspace(lib):
    need = lib.vk_rpn_multilevel_workspace_bytes(2, 3, 16, 48)
    st, err = _ml(lib, 3, 16, 48, ws_bytes=need - 1, N=2)
    assert st == L.VK_EINVAL and err == f"rpn_ml: workspace too small ({need - 1} < {need})"
    assert lib.vk_rpn_multilevel_workspace_bytes(2, 0, 16, 48) == 0 == lib.vk_rpn_multilevel_workspace_bytes(2, 7, 16, 48)


def test_nms_refuses_too_many_boxes_and_a_short_workspace(lib):
    st = lib.vk_nms(FAKE, FAKE, 8193, 0.5, FAKE, FAKE, FAKE, 1 << 30, None)
    assert st == L.VK_EINVAL and lib.vk_last_error().decode() == "nms: n=8193 must be in 0..8192"
    st = lib.vk_nms(FAKE, FAKE, 10, 0.5, FAKE, FAKE, FAKE, lib.vk_nms_workspace_bytes(10) - 1, None)
    assert st == L.VK_EINVAL and lib.vk_last_error().decode() == "nms: workspace too small"


def test_workspace_sizes_are_monotone(lib):
    pres = [1, 63, 64, 65, 1000, 6000, 8192]
    for N in (1, 2, 3, 32):
        a = [lib.vk_rpn_workspace_bytes(N, 63000, p) for p in pres]
        assert all(x > 0 for x in a) and a == sorted(a) and len(set(a)) > 1
        assert lib.vk_rpn_workspace_bytes(N + 1, 63000, 1000) > lib.vk_rpn_workspace_bytes(N, 63000, 1000)
        m = [lib.vk_rpn_multilevel_workspace_bytes(N, 3, p, p) for p in (1, 64, 200, 1000, 2730)]
        assert all(x > 0 for x in m) and m == sorted(m) and len(set(m)) > 1
        assert lib.vk_rpn_multilevel_workspace_bytes(N + 1, 3, 200, 600) > lib.vk_rpn_multilevel_workspace_bytes(N, 3, 200, 600)
    # the entry point carves for `post`, the size query for `pre`: what the query returns is enough for every allowed post
    assert lib.vk_rpn_workspace_bytes(2, 5, 16) == lib.vk_rpn_workspace_bytes(2, 63000, 16)
    n = [lib.vk_nms_workspace_bytes(k) for k in (0, 1, 64, 65, 8192)]
    assert n == sorted(n) and n[0] > 0
