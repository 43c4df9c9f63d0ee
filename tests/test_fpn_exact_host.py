"""CPU: what tests/test_gpu_fpn_kernels.py relies on, proved without a GPU -- the form vk_roi_align_form names for every case
of the tables (host only), the exactness of every exact set and of the pyramid (the fp32 oracle, per-sample order, against
roi_align_fp64 bit for bit, every value fp32), that the sets reach both paths of the separable kernel, and that the fp32
oracle stays inside the derived bound on the cases that are not exact."""
import numpy as np
import pytest
import torch

from oracle import fpn_oracle as fo
from vltk_amd import _lib as L

import fpn_exact_util as X
import roi_align_c4_util as U


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("VK_ROIALIGN_TABLES", raising=False)


# ---- the forms ------------------------------------------------------------------------------------------------------------------
def test_case_tables_name_the_form_they_are_for():
    for dt, C_ in X.SCALAR_CASES:
        assert X.form(C_, 7, dt) == "scalar", (dt, C_)
    for dt, C_ in X.SEP_CASES:
        for P in (7, 14, 16):
            assert X.form(C_, P, dt) == "sep", (dt, C_, P)
        assert X.form(C_, 17, dt) == X.form(C_, 32, dt) == "vec"
    for f, cases in X.ROUGH_CASES.items():
        for dt, C_ in cases:
            for P, _, _ in X.ROUGH_GEOMS[f]:
                assert X.form(C_, P, dt) == f, (f, dt, C_, P)


def test_form_edges_and_refusals():
    lib = L.load()
    assert X.form(1024, 7, X.F32) == "sep" and X.form(1028, 7, X.F32) == "scalar"        # C / vec = 256 | 257
    assert X.form(2048, 7, X.BF16) == "sep" and X.form(2056, 7, X.F16) == "scalar"
    assert X.form(4, 7, X.F32) == "sep" and X.form(4, 7, X.F16) == "scalar"              # one 16-byte chunk | half of one
    assert X.form(256, 16, X.F16) == "sep" and X.form(256, 17, X.F16) == "vec"
    for args in ((0, 7, X.F16), (256, 0, X.F16), (-8, 7, X.F32), (256, 7, L.VK_I64), (256, 7, L.VK_I32), (256, 7, 99)):
        assert lib.vk_roi_align_form(*args) == -L.VK_EINVAL, args


def test_tables_switch_is_read_per_call(monkeypatch):
    assert X.form(256, 7, X.F16) == "sep"
    monkeypatch.setenv("VK_ROIALIGN_TABLES", "0")
    assert X.form(256, 7, X.F16) == "vec" and X.form(12, 7, X.F16) == "scalar"
    monkeypatch.setenv("VK_ROIALIGN_TABLES", "1")
    assert X.form(256, 7, X.F16) == "sep"


# ---- the exact sets -------------------------------------------------------------------------------------------------------------
def assert_fp32_exact(got32, ref64, what):
    assert got32.dtype == np.float32
    assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64), f"{what}: a value is not an fp32 number"
    bad = (got32.astype(np.float64) != ref64).reshape(len(ref64), -1).any(1).nonzero()[0].tolist()
    assert not bad, f"{what}: RoIs {bad} differ between the fp32 oracle and the fp64 restatement"


@pytest.mark.parametrize("P,sr,aligned,scale", X.exact_geometries())
def test_exact_sets_are_exact(P, sr, aligned, scale):
    """Eight channels stand for all: a channel's sums do not depend on the others."""
    rois, ref = X.exact_reference(P, sr, aligned, scale, 8)
    got = fo.roi_align(torch.from_numpy(X.exact_map_wide()[:, :8].copy()), rois, P, scale, sr, aligned).numpy()
    assert np.abs(ref).max() > 1
    assert_fp32_exact(got, ref, (P, sr, aligned, scale))


@pytest.mark.parametrize("P,sr,aligned,scale", X.sep_geometries())
def test_sep_sets_hold_both_kinds_of_roi(P, sr, aligned, scale):
    """At least five RoIs whose footprint the separable kernel takes from its tables and five that take its per-sample loop."""
    kinds = [X.sep_takes_tables(r, P, scale, sr, aligned) for r in X.exact_boxes(aligned, P)]
    assert sum(kinds) >= 5 and len(kinds) - sum(kinds) >= 5, (sum(kinds), len(kinds))


def test_predicate_known_answers():
    # P = 7 at 1/4, adaptive: 224 px -> bins of 8 cells, 8 samples, 10 rows: tables; 896 px -> 32 cells, 34 rows: the loop
    assert X.sep_takes_tables(np.float32([0, 0, 0, 224, 224]), 7, X.S4, 0, True)
    assert not X.sep_takes_tables(np.float32([0, 0, 0, 896, 896]), 7, X.S4, 0, True)
    assert not X.sep_takes_tables(np.float32([0, 0, 0, 896, 224]), 7, X.S8, 0, True)
    # a fixed ratio of 2 over bins of 8 cells: 7 x 7 rows against 4 * 4 + 4 reads
    assert not X.sep_takes_tables(np.float32([0, 0, 0, 896, 896]), 7, X.S16, 2, True)
    assert X.sep_takes_tables(np.float32([0, 0, 0, 896, 112]), 7, X.S16, 2, True) is False          # 7 x 3 = 21 > 20
    assert X.sep_takes_tables(np.float32([0, 0, 0, 448, 224]), 7, X.S16, 2, True)                   # 5 x 4 = 20
    assert not X.sep_takes_tables(np.float32([0, 0, 0, 448, 448]), 7, X.S16, 2, True)               # 5 x 5 = 25
    assert not X.sep_takes_tables(np.float32([0, 448, 320, 224, 96]), 7, X.S16, 2, True)            # inverted


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------
def rule_levels():
    return fo.assign_boxes_to_levels(U.exact_rois()[:, 1:], 2, 5).numpy()


def test_pyramid_levels_cover_all_four_and_the_permutation_moves_boxes():
    lv = rule_levels()
    assert set(lv.tolist()) == {0, 1, 2, 3}
    moved = X.permuted_levels(lv)
    assert (moved != lv).sum() >= 10 and set(moved.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("sr", [X.PYR_SR, 0])
@pytest.mark.parametrize("which", ["rule", "permuted"])
def test_pyramid_is_exact_for_every_roi_and_level_used(which, sr):
    lv = rule_levels() if which == "rule" else X.permuted_levels(rule_levels())
    rois, ref = U.exact_rois(), X.pyramid_reference(lv, 8, sr)
    got = np.zeros(ref.shape, np.float32)
    for li, (m, s) in enumerate(zip(X.pyramid_maps(8), X.PYR_SCALES)):
        idx = np.nonzero(lv == li)[0]
        got[idx] = fo.roi_align(torch.from_numpy(m.copy()), rois[idx], X.PYR_P, s, sr, True).numpy()
    assert_fp32_exact(got, ref, (which, sr))
    # a wrong level's map, size or scale gives other numbers for most boxes
    wrong = X.pyramid_reference((lv + 1) % 4, 8, sr)
    assert (wrong != ref).reshape(len(ref), -1).any(1).sum() >= len(ref) - 4


# ---- not exact: the bound -----------------------------------------------------------------------------------------------------
def test_rough_boxes_are_what_they_say():
    r = X.rough_rois()
    N, H, W = X.ROUGH_MAP
    w, h = r[:, 3] - r[:, 1], r[:, 4] - r[:, 2]
    assert (w < 0).sum() >= 3 and ((w > 0) & (w < 16) & (h > 0) & (h < 16)).sum() >= 12          # inverted; below one cell
    assert (w == 0).any() and (r[:, 1] > W * 16).any() and ((r[:, 1] < 0) & (r[:, 3] > W * 16)).any()


@pytest.mark.parametrize("P,sr,aligned", sorted({g for gs in X.ROUGH_GEOMS.values() for g in gs}))
def test_fp32_oracle_stays_inside_the_bound(P, sr, aligned):
    """The oracle sums per sample in its own order: an independent fp32 evaluation of the same geometry."""
    x, rois = X.rough_map(16, torch.float32), X.rough_rois()
    ref, bound = X.rough_reference(x, rois, P, X.S16, sr, aligned, torch.float32)
    got = fo.roi_align(torch.from_numpy(x), rois, P, X.S16, sr, aligned).numpy()
    worst = X.worst_ratio(got, ref, bound)
    print(f"\n[oracle f32 P={P} sr={sr} aligned={aligned}] worst |out - ref| / bound {worst:.3f}")
    assert np.abs(ref).max() > 0.5 and worst <= 1
    # the fp64-geometry restatement is a different function (positions rounded elsewhere): close, not inside the rounding bound's reach
    assert np.abs(U.roi_align_fp64(x, rois, P, X.S16, sr, aligned) - ref).max() <= 1e-4 * np.abs(ref).max()


def test_the_bound_is_tight_enough_to_bite():
    """A relative error of 2^-14 on every element, or the fp64-geometry restatement in place of the fp32 one, leaves it in f32."""
    x, rois = X.rough_map(16, torch.float32), X.rough_rois()
    ref, bound = X.rough_reference(x, rois, 7, X.S16, 3, True, torch.float32)
    assert X.worst_ratio(ref * (1 + 2.0 ** -14), ref, bound) > 1
    assert X.worst_ratio(ref, ref, bound) == 0


def test_half_ulp():
    assert X.half_ulp(np.float64([1.0, 1.5, 2.0, 1e-9, 0.0]), torch.float16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25,
                                                                                         2.0 ** -25]
    assert X.half_ulp(np.float64([1.0, 3.0]), torch.bfloat16).tolist() == [2.0 ** -8, 2.0 ** -7]
    assert X.half_ulp(np.float64([1.0]), torch.float32).tolist() == [0.0]
