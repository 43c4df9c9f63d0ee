"""CPU (-m "not gpu"): LXMERT's pre-training heads and losses, the host side.  The parameter spec against the names and shapes
transformers' own `state_dict()` had (tests/golden/lxmert_pretrain_small.npz), the tied-decoder rules, the label checks (which run
before the library is touched), the loss-only row index, and the checker of the GPU tests itself: the float32 restatements of
the kernels' arithmetic (tests/lxmert_pretrain_util.py) fit the per-row bounds, wrong arithmetic does not, and the float64
references reproduce transformers' loss terms."""
import os
import types

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import lxmert_pretrain as LP

import lxmert_pretrain_util as U

TDS = [torch.float32, torch.float16, torch.bfloat16]
TD_IDS = ["fp32", "fp16", "bf16"]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lxmert_pretrain_small.npz"))


# ---- the parameter spec and the state dict -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B", "noobj", "featonly", "untied"])
def test_param_spec_is_transformers_state_dict(g, tag):
    sw, spec = U.stored_spec(g, tag)
    cfg = LP.lxmert_pretraining_config(**{k[4:]: g[k].item() for k in g.files if k.startswith("cfg/")}, **sw)
    assert [(k, tuple(s)) for k, s in LP.lxmert_pretraining_param_spec(cfg)] == spec
    names = [n for n, _ in spec]
    assert ("answer_head.logit_fc.3.weight" in names) == cfg["task_qa"]
    assert ("obj_predict_head.transform.dense.weight" in names) == cfg["task_obj_predict"]
    assert ("obj_predict_head.decoder_dict.attr.weight" in names) == (cfg["task_obj_predict"] and cfg["visual_attr_loss"])
    sd = LP.make_lxmert_pretraining_state_dict(cfg, 3)
    assert [(k, v.shape) for k, v in sd.items()] == spec
    assert (sd[LP.DECODER] is sd[LP.WORDS]) == cfg["tie_word_embeddings"]


def test_config_defaults_are_lxmert_configs():
    cfg = LP.lxmert_pretraining_config()
    assert (cfg["num_qa_labels"], cfg["num_object_labels"], cfg["num_attr_labels"], cfg["visual_loss_normalizer"]) == (9500, 1600, 400, 6.67)
    assert all(cfg[k] for k in ("task_mask_lm", "task_obj_predict", "task_matched", "task_qa", "visual_obj_loss", "visual_attr_loss",
                                "visual_feat_loss", "tie_word_embeddings"))
    assert LP.visual_losses(cfg) == [("obj", 1600), ("attr", 400), ("feat", 2048)]


def test_tied_decoder_rules(g):
    cfg, sd = U.golden_model(g)
    words = sd[LP.WORDS]
    absent = {k: v for k, v in sd.items() if k != LP.DECODER}
    assert LP.resolve_decoder_weight(cfg, absent) is words                             # tied: the key may be absent
    assert LP.resolve_decoder_weight(cfg, dict(absent, **{LP.DECODER: words.copy()})) is words      # present and equal
    with pytest.raises(RuntimeError, match="differs"):
        LP.resolve_decoder_weight(cfg, dict(absent, **{LP.DECODER: words + 1}))      # present and different
    untied = dict(cfg, tie_word_embeddings=False)
    with pytest.raises(RuntimeError, match="must hold"):
        LP.resolve_decoder_weight(untied, absent)                                      # untied: required ...
    other = words + 1
    assert LP.resolve_decoder_weight(untied, dict(absent, **{LP.DECODER: other})) is other          # ... and used


# ---- the label checks ----------------------------------------------------------------------------------------------------------------
def _labels(g):
    _, kw, lab = U.case_args(g, "all")
    return kw, lab


def test_label_checks_pass_the_golden_labels_and_convert(g):
    cfg, _ = U.golden_model(g)
    _, lab = _labels(g)
    out = LP.check_pretraining_labels(cfg, 3, 9, 5, **lab)
    assert set(out) == {"labels", "matched_label", "ans", "obj_label", "obj_conf", "attr_label", "attr_conf", "feat_label", "feat_conf"}
    assert all(out[k].dtype == np.int64 for k in ("labels", "matched_label", "ans", "obj_label", "attr_label"))
    assert all(out[k].dtype == torch.float32 and out[k].is_contiguous() for k in ("obj_conf", "attr_conf", "feat_label", "feat_conf"))
    conf64 = dict(lab["obj_labels"], feat=(lab["obj_labels"]["feat"][0].double(), lab["obj_labels"]["feat"][1].double()))
    assert LP.check_pretraining_labels(cfg, 3, 9, 5, obj_labels=conf64)["feat_label"].dtype == torch.float32
    # a task the config switches off ignores its labels, as upstream
    off, _ = U.golden_model(g, "B")
    out = LP.check_pretraining_labels(off, 3, 9, 5, ans=torch.tensor([999, 999, 999]), obj_labels={k: v for k, v in lab["obj_labels"].items() if k != "attr"})
    assert set(out) == {"obj_label", "obj_conf", "feat_label", "feat_conf"}


def test_label_checks_raise(g):
    cfg, _ = U.golden_model(g)
    _, lab = _labels(g)
    chk = lambda **kw: LP.check_pretraining_labels(cfg, 3, 9, 5, **kw)      # noqa: E731
    for bad in (cfg["vocab_size"], -1, -99):
        t = lab["labels"].clone()
        t[1, 4] = bad
        with pytest.raises(IndexError):
            chk(labels=t)
    with pytest.raises(ValueError):
        chk(labels=lab["labels"][:, :8])
    with pytest.raises(ValueError):
        chk(labels=lab["labels"].float())
    with pytest.raises(IndexError):
        chk(matched_label=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        chk(matched_label=torch.tensor([[0, 1, 1]]))
    with pytest.raises(IndexError):
        chk(ans=torch.tensor([0, cfg["num_qa_labels"], 1]))
    obj = lab["obj_labels"]
    with pytest.raises(KeyError):
        chk(obj_labels={k: v for k, v in obj.items() if k != "attr"})         # enabled by the config, absent from the dict
    with pytest.raises(IndexError):
        chk(obj_labels=dict(obj, obj=(torch.full((3, 5), cfg["num_object_labels"]), obj["obj"][1])))
    with pytest.raises(ValueError):
        chk(obj_labels=dict(obj, attr=(obj["attr"][0], obj["attr"][1][:, :4])))
    with pytest.raises(ValueError):
        chk(obj_labels=dict(obj, feat=(obj["feat"][0][..., :31], obj["feat"][1])))
    with pytest.raises(ValueError):
        chk(obj_labels=dict(obj, feat=(obj["feat"][0].long(), obj["feat"][1])))


def test_model_checks_labels_before_it_touches_the_library(g, monkeypatch):
    """A call with a bad label raises from the host checks: no library load and no launch happens before them."""
    cfg, _ = U.golden_model(g)
    kw, lab = _labels(g)

    def refuse(*a, **k):
        raise AssertionError("the library was touched before the labels were checked")
    monkeypatch.setattr(L, "load", refuse)
    monkeypatch.setattr(L, "call", refuse)
    m = LP.LxmertForPreTraining.__new__(LP.LxmertForPreTraining)
    m.cfg, m.lxmert = cfg, types.SimpleNamespace(cfg=cfg)
    with pytest.raises(IndexError):
        m(**kw, **dict(lab, ans=torch.tensor([0, 11, 0])))
    with pytest.raises(KeyError):
        m(**kw, obj_labels={"obj": lab["obj_labels"]["obj"]})
    with pytest.raises(ValueError):
        m(**kw, labels=lab["labels"].T)
    with pytest.raises(IndexError):
        m(**dict(kw, input_ids=torch.full((3, 9), cfg["vocab_size"])), **lab)
    with pytest.raises(ValueError, match="needs `labels`"):
        m(**kw, matched_label=lab["matched_label"], logits=False)


def test_loss_only_index():
    lab = np.full((3, 5), -100)
    lab[0, 4], lab[2, 0], lab[1, 1], lab[1, 2] = 7, 0, 96, 5
    idx, picked = LP.loss_only_index(lab)
    assert idx.dtype == np.int32 and picked.dtype == np.int64
    assert idx.tolist() == [4, 6, 7, 10] and picked.tolist() == [7, 96, 5, 0]            # ascending rows of the [B * Lt] view
    idx, picked = LP.loss_only_index(np.full((2, 3), -100))
    assert len(idx) == 0 and len(picked) == 0


# ---- the checker: right arithmetic fits the bounds, wrong arithmetic does not -----------------------------------------------------
def ce_rows_case(C, td, seed=0):
    """Four rows in the storage type: random, logits near +-90 (a single fp32 exp overflows without the max subtraction), all equal,
    and a peaked one; labels 0, C - 1, a middle column and C - 1."""
    gen = np.random.Generator(np.random.PCG64([C, seed]))
    x = gen.standard_normal((4, C)) * 2
    x[1] = np.where(gen.uniform(size=C) < 0.5, 90.0, -90.0) + gen.standard_normal(C)
    x[1, 0] = 90.5
    x[2] = 1.25
    x[3, C // 2] += 12
    x = torch.from_numpy(x).to(td)
    return x, np.asarray([0, C - 1, C // 2, C - 1])


@pytest.mark.parametrize("C", [2, 100, 30522])
@pytest.mark.parametrize("td", TDS, ids=TD_IDS)
def test_restated_cross_entropy_fits_the_bound_and_a_shifted_label_does_not(td, C):
    x, labels = ce_rows_case(C, td)
    ld = (C + 7) // 8 * 8
    forms = {U.ce_form(C, ld, td), "scalar"}
    assert ("vec" in forms) == (C >= 128)
    r = U.ce_reference(x, labels)
    xf = x.float().numpy()
    for form in forms:
        bound = U.ce_bound(r, form, td)
        got = np.asarray([U.ce_row_f32(xf[i], labels[i], form, td) for i in range(4)], np.float64)
        ratio = np.abs(got - r["ref"]) / bound
        print(f"\n[restated cross-entropy {form} C={C}] worst |out - ref| / bound {ratio.max():.3f}", end="")
        assert ratio.max() <= 1.0
        assert (bound <= 1e-4 * np.maximum(np.abs(r["ref"]), 1)).all()              # the bound itself stays a rounding-error bound
        wrong = np.asarray([U.ce_row_f32(xf[i], labels[i], form, td, label_shift=1) for i in (0, 1, 3)], np.float64)
        assert (np.abs(wrong - r["ref"][[0, 1, 3]]) > 100 * bound[[0, 1, 3]]).all()     # the label column off by one


@pytest.mark.parametrize("C", [2, 100])
def test_the_large_row_overflows_without_the_max_subtraction(C):
    """What the +-90 row is for: exp(90.5) is beyond fp32 (e^88.73 is its largest number), so a sum of exponentials taken without
    the row maximum is inf at every width, the two-column one included, while the reference of that row is finite."""
    x, labels = ce_rows_case(C, torch.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(x[1].numpy()).sum(dtype=np.float32))
    assert np.isfinite(U.ce_reference(x, labels)["ref"][1])


@pytest.mark.parametrize("C", [32, 2048])
def test_restated_smooth_l1_fits_the_bound_and_the_quadratic_branch_does_not(C):
    gen = np.random.Generator(np.random.PCG64(C))
    pred = torch.from_numpy(gen.standard_normal((3, C))).to(torch.bfloat16)
    target = pred.float().numpy() + gen.uniform(-3, 3, (3, C)).astype(np.float32)
    target[0, :3] = pred.float().numpy()[0, :3] + np.asarray([1, -1, 0], np.float32)    # exactly +-1 and 0
    r = U.smooth_l1_reference(pred, target)
    bound = U.smooth_l1_bound(r)
    got = np.asarray([U.smooth_l1_row_f32(pred.float().numpy()[i], target[i]) for i in range(3)], np.float64)
    assert (np.abs(got - r["ref"]) <= bound).all()
    wrong = np.asarray([U.smooth_l1_row_f32(pred.float().numpy()[i], target[i], quadratic_everywhere=True) for i in range(3)], np.float64)
    assert (np.abs(wrong - r["ref"]) > 100 * bound).all()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 4097])
def test_restated_reduce_matches_and_wrong_divisors_do_not(M):
    gen = np.random.Generator(np.random.PCG64(M))
    rows = gen.uniform(0.1, 9, M).astype(np.float32)
    labels = np.where(gen.uniform(size=M) < 0.3, -100, 5)
    labels[0] = 5
    conf = gen.uniform(0, 1, M).astype(np.float32)
    assert U.reduce_matches(U.loss_reduce_f32(rows, labels=labels), U.reduce_reference(rows, labels=labels))
    assert U.reduce_matches(U.loss_reduce_f32(rows, weight=conf, scale=6.67), U.reduce_reference(rows, weight=conf, scale=6.67))
    assert U.reduce_matches(U.loss_reduce_f32(rows, labels=np.full(M, -100)), U.reduce_reference(rows, labels=np.full(M, -100)))
    assert np.isnan(U.loss_reduce_f32(rows, labels=np.full(M, -100)))
    if (labels == -100).any():
        for wrong in ("count_ignored", "divide_by_M"):
            assert not U.reduce_matches(U.loss_reduce_f32(rows, labels=labels, wrong=wrong), U.reduce_reference(rows, labels=labels))
    if M > 1:
        assert not U.reduce_matches(U.loss_reduce_f32(rows, weight=conf, scale=6.67, wrong="conf_after_mean"),
                                    U.reduce_reference(rows, weight=conf, scale=6.67))


# ---- the references against transformers ---------------------------------------------------------------------------------------------
def test_references_reproduce_transformers_losses(g):
    """float64 restatements on transformers' own logits give its loss terms to 1e-6 relative (its arithmetic is fp32), NaN where it
    has NaN, and the fp32 total in its order.  This pins the restatements, not the kernels."""
    for case in U.golden_cases(g):
        cname, _, lab = U.case_args(g, case)
        cfg, _ = U.golden_model(g, cname)
        total, terms = U.case_losses(g, case)
        ref_total, ref = U.losses_reference(cfg, U.case_logits(g, case), lab)
        assert set(ref) == set(terms), (case, set(ref), set(terms))
        for k, v in terms.items():
            if np.isnan(v):
                assert np.isnan(ref[k]), (case, k)
            else:
                assert abs(ref[k] - v) <= 1e-6 * max(abs(float(v)), 1e-30), (case, k, ref[k], v)
        if np.isnan(total):
            assert np.isnan(ref_total)
        else:
            assert abs(float(ref_total) - float(total)) <= 1e-6 * abs(float(total))
        assert np.float32(total) == U.total_reference(terms) or np.isnan(total)          # the order of the adds, bit for bit
    assert np.isnan(U.case_losses(g, "nan")[0]) and U.case_losses(g, "obj")[1]["attr"] == 0
    assert set(U.case_losses(g, "switched_off")[1]) == {"mlm", "matched", "obj", "feat"}


def test_oracle_heads_reproduce_transformers_logits(g):
    for case in ("all", "padded", "switched_off"):
        cname, kw, _ = U.case_args(g, case)
        cfg, sd = U.golden_model(g, cname)
        got = U.PretrainOracle(cfg, sd).heads(**{k: v.numpy() for k, v in kw.items()})
        want = U.case_logits(g, case)
        assert set(got) == set(want)
        for k, v in want.items():
            assert np.abs(got[k].numpy() - v).max() <= 1e-5 * np.abs(v).max(), (case, k)
