"""CPU: the LayoutLM oracle (tests/layoutlm_util.py) against vectors produced by transformers.LayoutLMModel and its three heads
themselves, the build's parameter specs against those classes' recorded state_dict, `ocr_token_boxes` against a hand-written
table, the host-side checks of vltk_amd/layoutlm.py that run before any library call, and the three entry points of
csrc/layoutlm.hip as far as they answer without a device."""
import os
import re

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import layoutlm as LM

from layoutlm_util import (CASES, LayoutLMOracle, case_kwargs, golden_head, golden_model, ocr_token_boxes_ref, span_select_ref,
                           stored_spec, token_word_labels_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(vocab_size=50, hidden_size=32, num_attention_heads=2, intermediate_size=64, num_hidden_layers=1,
             max_position_embeddings=8, max_2d_position_embeddings=16)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "layoutlm_small.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-9)


# ---- the oracle against transformers' vectors --------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_oracle_vs_transformers_golden(g, geo, case):
    """Embeddings to 1e-5, every other stored output (model and the three heads) to 1e-4."""
    cfg, sd = golden_model(g)
    ids, kw, tag = g[f"{geo}/input_ids"], case_kwargs(g, geo, case), f"{geo}/{case}"
    (seq, pooled), st = LayoutLMOracle(cfg, sd).forward(ids, return_stages=True, **kw)
    assert rel(st["embeddings"], g[f"{tag}/embedding_output"]) <= 1e-5
    assert rel(seq, g[f"{tag}/last_hidden_state"]) <= 1e-4
    assert rel(pooled, g[f"{tag}/pooler_output"]) <= 1e-4
    assert rel(LayoutLMOracle(cfg, golden_head(g, "token")[2]).token_forward(ids, **kw), g[f"{tag}/token_logits"]) <= 1e-4
    start, end = LayoutLMOracle(cfg, golden_head(g, "qa")[2]).qa_forward(ids, **kw)
    assert rel(start, g[f"{tag}/start_logits"]) <= 1e-4 and rel(end, g[f"{tag}/end_logits"]) <= 1e-4
    assert rel(LayoutLMOracle(cfg, golden_head(g, "seq")[2]).seq_forward(ids, **kw), g[f"{tag}/seq_logits"]) <= 1e-4


def test_golden_cases_exercise_what_they_claim(g):
    """Both geometries, boxes at the edges of the tables (0, 1000, zero width, zero height, the full page), ragged masks that keep
    at least two tokens, and three cases that differ from each other."""
    assert g["short/input_ids"].shape == (3, 40) and g["long/input_ids"].shape == (2, 80)
    assert (int(g["token/num_labels"]), int(g["qa/num_labels"]), int(g["seq/num_labels"])) == (7, 2, 5)
    for geo in ("short", "long"):
        b = g[f"{geo}/bbox"]
        assert b.min() == 0 and b.max() == 1000 and b[0, 0].tolist() == [0, 0, 1000, 1000]
        assert (b[..., 2] >= b[..., 0]).all() and (b[..., 3] >= b[..., 1]).all()
        assert b[0, 1, 0] == b[0, 1, 2] and b[0, 1, 3] > b[0, 1, 1]              # zero width
        assert b[0, 2, 1] == b[0, 2, 3] and b[0, 2, 2] > b[0, 2, 0]              # zero height
        s = g[f"{geo}/attention_mask"].sum(1)
        assert len(set(s.tolist())) > 1 and s.min() >= 2
        assert g[f"{geo}/token_type_ids"].min() == 0 and g[f"{geo}/token_type_ids"].max() == 1
        for a, c in (("plain", "masked"), ("plain", "nobox")):
            assert rel(g[f"{geo}/{a}/embedding_output"], g[f"{geo}/{c}/embedding_output"]) > 1e-2
        assert g[f"{geo}/plain/token_logits"].shape == b.shape[:2] + (7,) and g[f"{geo}/plain/seq_logits"].shape == (b.shape[0], 5)
        assert g[f"{geo}/plain/start_logits"].shape == b.shape[:2] == g[f"{geo}/plain/end_logits"].shape


@pytest.mark.parametrize("emulate,tol", [("bf16", 6e-2), ("fp16", 1e-2)])
def test_emulation_stays_near_fp32(g, emulate, tol):
    """Storage roundings through the embeddings and two layers stay within the bound the LXMERT, VisualBERT and ViT oracles'
    emulation is held to."""
    cfg, sd = golden_model(g)
    seq, pooled = LayoutLMOracle(cfg, sd, emulate=emulate).forward(g["long/input_ids"], **case_kwargs(g, "long", "masked"))
    assert rel(seq, g["long/masked/last_hidden_state"]) <= tol and rel(pooled, g["long/masked/pooler_output"]) <= tol


# ---- parameter specs, config, seeded weights ---------------------------------------------------------------------------------------
def test_param_specs_match_the_recorded_state_dicts(g):
    """Names, shapes and order of `state_dict()` of transformers' four classes, recorded by the generator for the fixture's config
    and for the default one."""
    small, _ = golden_model(g)
    for tag, cfg in (("small", small), ("default", LM.layoutlm_config())):
        assert [(k, tuple(s)) for k, s in LM.layoutlm_param_spec(cfg)] == stored_spec(g, tag, "model")
        for head, lin in (("token", "classifier"), ("qa", "qa_outputs"), ("seq", "classifier")):
            n = int(g[f"{head}/num_labels"])
            assert [(k, tuple(s)) for k, s in LM.layoutlm_head_param_spec(cfg, lin, n)] == stored_spec(g, tag, head)
    names = [k for k, _ in stored_spec(g, "default", "model")]
    assert names[:7] == [f"embeddings.{t}_embeddings.weight" for t in ("word", "position", "x_position", "y_position", "h_position",
                                                                       "w_position", "token_type")]
    assert names[-1] == "pooler.dense.bias" and "encoder.layer.11.output.LayerNorm.bias" in names


def test_config_defaults_and_refusals():
    cfg = LM.layoutlm_config()
    assert (cfg["vocab_size"], cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["intermediate_size"]) == \
        (30522, 768, 12, 12, 3072)
    assert (cfg["max_position_embeddings"], cfg["max_2d_position_embeddings"], cfg["type_vocab_size"], cfg["layer_norm_eps"]) == \
        (512, 1024, 2, 1e-12)
    assert LM.layoutlm_config(hidden_size=128, num_attention_heads=4)["hidden_size"] == 128
    with pytest.raises(NotImplementedError):
        LM.layoutlm_config(hidden_act="relu")


def test_synthetic_weights_are_seeded_per_tensor():
    cfg = LM.layoutlm_config(**SMALL)
    a, b, c = LM.make_layoutlm_state_dict(cfg, 3), LM.make_layoutlm_state_dict(cfg, 3), LM.make_layoutlm_state_dict(cfg, 4)
    assert list(a) == [k for k, _ in LM.layoutlm_param_spec(cfg)]
    assert all(np.array_equal(a[k], b[k]) and a[k].shape == tuple(s) for k, s in LM.layoutlm_param_spec(cfg))
    assert not np.array_equal(a["pooler.dense.weight"], c["pooler.dense.weight"])
    assert not np.array_equal(a["embeddings.x_position_embeddings.weight"], a["embeddings.y_position_embeddings.weight"])
    assert 0.5 <= a["embeddings.LayerNorm.weight"].min() and a["embeddings.LayerNorm.weight"].max() <= 1.5
    qa = LM.make_layoutlm_head_state_dict(cfg, "qa_outputs", 2, 3)
    assert list(qa) == [k for k, _ in LM.layoutlm_head_param_spec(cfg, "qa_outputs", 2)] and qa["qa_outputs.weight"].shape == (2, 32)
    assert np.array_equal(qa["layoutlm.pooler.dense.bias"], a["pooler.dense.bias"])


def test_strict_load_refuses_stray_and_missing_keys():
    """BertOps._check_state_dict is what load_state_dict runs; it needs no GPU."""
    cfg = LM.layoutlm_config(**SMALL)
    sd = LM.make_layoutlm_state_dict(cfg, 5)
    want = dict(LM.layoutlm_param_spec(cfg))
    model = object.__new__(LM.LayoutLMModel)
    model._check_state_dict(sd, want, True)
    with pytest.raises(RuntimeError, match="unexpected"):
        model._check_state_dict(dict(sd, **{"embeddings.z_position_embeddings.weight": sd["pooler.dense.bias"]}), want, True)
    short = dict(sd)
    del short["embeddings.h_position_embeddings.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        model._check_state_dict(short, want, True)
    with pytest.raises(RuntimeError, match="shape"):
        model._check_state_dict(dict(sd, **{"embeddings.w_position_embeddings.weight": np.zeros((15, 32), np.float32)}), want, True)


# ---- ocr_token_boxes -----------------------------------------------------------------------------------------------------------------
#  a 500 x 250 page: x scales by 2, y by 4
WORDS = [[10, 20, 30, 5],        # -> (20, 80, 80, 100)
         [400, 200, 150, 100],   # x + w = 550 and y + h = 300 lie past the page -> (800, 800, 1000, 1000), clamped
         [0.3, 0.2, 0.4, 0.2],   # -> (0.6, 0.8, 1.4, 1.6) floored to (0, 0, 1, 1)
         [100, 10, 0, 7],        # a zero-width word -> (200, 40, 200, 68)
         [250, 125, 1, 1]]       # -> (500, 500, 502, 504)
TOKENMAP = [1, 3, 2, 0, 2]       # the fourth word has no token


def test_ocr_token_boxes_by_hand():
    a, b, c, e = [20, 80, 80, 100], [800, 800, 1000, 1000], [0, 0, 1, 1], [500, 500, 502, 504]
    z, page = [0, 0, 0, 0], [0, 0, 1000, 1000]
    table = [
        (dict(max_len=10), [a, b, b, b, c, c, e, e, z, z], [0, 1, 1, 1, 2, 2, 4, 4, -1, -1]),
        (dict(max_len=3), [a, b, b], [0, 1, 1]),                                         # cut in the middle of word 1
        (dict(max_len=5, add_cls=True), [page, a, b, b, b], [-1, 0, 1, 1, 1]),
        (dict(max_len=10, add_cls=True), [page, a, b, b, b, c, c, e, e, z], [-1, 0, 1, 1, 1, 2, 2, 4, 4, -1]),
        (dict(max_len=1, add_cls=True), [page], [-1]),
    ]
    for kw, want_box, want_ids in table:
        for fn in (LM.ocr_token_boxes, ocr_token_boxes_ref):
            bbox, ids = fn(WORDS, TOKENMAP, (500, 250), **kw)
            assert bbox.dtype == np.int64 and ids.dtype == np.int32
            assert bbox.tolist() == want_box and ids.tolist() == want_ids, (fn.__name__, kw)
    bbox, ids = LM.ocr_token_boxes(np.zeros((0, 4)), [], (500, 250), 4)                  # a page without words
    assert bbox.tolist() == [z] * 4 and ids.tolist() == [-1] * 4
    bbox, _ = LM.ocr_token_boxes([[-5, -5, 3, 3]], [1], (100, 100), 1)                   # a box that begins off the page
    assert bbox.tolist() == [[0, 0, 0, 0]]
    for bad in ((WORDS, TOKENMAP[:4], (500, 250), 4), (WORDS, [1, -1, 1, 1, 1], (500, 250), 4), (WORDS, TOKENMAP, (0, 250), 4),
                (WORDS, TOKENMAP, (500, 250), 0)):
        with pytest.raises(ValueError):
            LM.ocr_token_boxes(*bad)


def test_ocr_token_boxes_feed_the_host_checks():
    """What `ocr_token_boxes` returns passes `check_bbox` at the default table size (1000 < 1024)."""
    bbox, _ = LM.ocr_token_boxes(WORDS, TOKENMAP, (500, 250), 12, add_cls=True)
    LM.check_bbox(bbox[None], 1, 12, 1024)


# ---- host checks ---------------------------------------------------------------------------------------------------------------------
def test_bbox_is_checked_on_the_host():
    """A coordinate of -1, one of max_2d, x1 < x0 and y1 < y0 raise IndexError with transformers' wording; a wrong shape or a float
    array ValueError: all before any library call (check_bbox never loads the library)."""
    ok = np.zeros((2, 5, 4), np.int64)
    ok[0, 0] = (0, 0, 1023, 1023)
    ok[1, 4] = (7, 9, 7, 9)
    LM.check_bbox(ok, 2, 5, 1024)
    LM.check_bbox(torch.from_numpy(ok), 2, 5, 1024)
    LM.check_bbox(None, 2, 5, 1024)
    for idx, box in (((1, 2), (-1, 0, 5, 5)), ((1, 2), (0, 0, 5, 1024)), ((0, 3), (6, 0, 5, 5)), ((0, 3), (0, 6, 5, 5))):
        bad = ok.copy()
        bad[idx] = box
        with pytest.raises(IndexError, match="within 0-1000 range"):
            LM.check_bbox(bad, 2, 5, 1024)
    with pytest.raises(IndexError):
        LM.check_bbox(ok, 2, 5, 1023)
    for bad in (ok[:, :4], ok[..., :3], ok.astype(np.float32), ok[0]):
        with pytest.raises(ValueError):
            LM.check_bbox(bad, 2, 5, 1024)


def test_model_inputs_are_checked_on_the_host():
    """LayoutLMModel._check needs the config only: shapes raise ValueError, a sequence longer than the position table ValueError,
    ids outside their tables IndexError."""
    m = object.__new__(LM.LayoutLMModel)
    m.cfg = LM.layoutlm_config(**SMALL)
    ids = torch.ones((2, 8), dtype=torch.int64)
    box = torch.zeros((2, 8, 4), dtype=torch.int64)
    m._check(ids, box, torch.ones(2, 8), torch.zeros_like(ids))
    m._check(ids, None, None, None)
    for bad in ((ids[0], None, None, None), (ids, box[:, :7], None, None), (ids, box, torch.ones(2, 7), None),
                (ids, box, None, torch.zeros((2, 7), dtype=torch.int64)), (torch.ones((2, 9), dtype=torch.int64), None, None, None),
                (ids[:, :0], None, None, None)):
        with pytest.raises(ValueError):
            m._check(*bad)
    for bad in ((ids * 50, None, None, None), (ids, torch.full_like(box, 16), None, None), (ids, box, None, torch.full_like(ids, 2))):
        with pytest.raises(IndexError):
            m._check(*bad)


# ---- the tail rules' restatements, by hand ----------------------------------------------------------------------------------------------
def test_vote_rule_is_torch_modes():
    """Ties in the vote give the smallest label, torch.mode's rule on the CPU: [3, 1, 3, 1, 2] -> 1."""
    assert int(torch.mode(torch.tensor([3, 1, 3, 1, 2])).values) == 1
    logits = np.full((1, 5, 4), -1.0, np.float32)
    for t, lab in enumerate([3, 1, 3, 1, 2]):
        logits[0, t, lab] = 1.0
    tok, words = token_word_labels_ref(logits, np.zeros((1, 5), np.int32), 2)
    assert tok.tolist() == [[3, 1, 3, 1, 2]] and words.tolist() == [[1, -1]]
    nan = np.asarray([[[np.nan, 2.0, 2.0], [np.nan, np.nan, -np.inf], [-np.inf, -np.inf, -np.inf]]], np.float32)
    tok, words = token_word_labels_ref(nan, np.asarray([[0, 5, -1]], np.int32), 3)       # word id 5 >= W is no word
    assert tok.tolist() == [[1, 0, 0]] and words.tolist() == [[1, -1, -1]]


def test_span_rule_by_hand():
    st = np.asarray([[0, 5, 1, 5, 0, 9]], np.float32)
    en = np.asarray([[9, 0, 4, 4, 1, 0]], np.float32)
    ctx = np.asarray([[0, 1, 1, 1, 1, 0]])
    s, e, sc = span_select_ref(st, en, ctx, 30)
    assert (s.tolist(), e.tolist(), sc.tolist()) == ([1], [2], [9.0])                    # (1, 2) ties (1, 3) and (3, 3): smaller s, then e
    s, e, sc = span_select_ref(st, en, ctx, 1)
    assert (s.tolist(), e.tolist(), sc.tolist()) == ([3], [3], [9.0])                    # one-token answers only
    s, e, sc = span_select_ref(st, en, np.zeros((1, 6), np.int64), 30)
    assert (s.tolist(), e.tolist()) == ([-1], [-1]) and sc[0] == -np.inf
    s, e, _ = span_select_ref(np.zeros((1, 6)), np.zeros((1, 6)), ctx, 30)
    assert (s.tolist(), e.tolist()) == ([1], [1])                                        # all equal: the first context token twice


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW = {"vk_layoutlm_embed": 23, "vk_token_word_labels": 11, "vk_span_select": 13}


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    for name, arity in NEW.items():
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", header)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == arity, f"{name}: the header declares another arity"
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == arity
        assert hasattr(L.load(), name), f"{name} not exported"
    mk = open(os.path.join(ROOT, "vltk_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/layoutlm.o" in re.search(r"^OBJS\s*=\s*(.*)$", mk, re.M).group(1)
    nofma = re.search(r"\$\(if \$\(filter ([^,]*),\$\*\),\$\(NOFMA\)\)", mk).group(1).split()
    hazsrc = re.search(r"^HAZSRC\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "layoutlm" not in nofma and "layoutlm.hip" not in hazsrc


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """The size checks come before anything touches a device, so they answer on a machine without one (pointers are never
    dereferenced on the host)."""
    lib, p = L.load(), 4096

    def embed(B=2, Lt=8, C=128, vocab=50, P=16, M2=1024, T=2, dt=L.VK_BF16, ids=p, box=p, out=p):
        return lib.vk_layoutlm_embed(ids, p, box, B, Lt, p, vocab, p, P, p, p, p, p, M2, p, T, p, p, out, C, 1e-12, dt, None)
    for bad in (dict(B=0), dict(Lt=0), dict(B=-1), dict(Lt=17), dict(B=1 << 27, Lt=16), dict(C=0), dict(C=2049), dict(vocab=0),
                dict(M2=0), dict(T=0), dict(dt=L.VK_I32), dict(dt=L.VK_I64), dict(ids=None), dict(box=None), dict(out=None)):
        assert embed(**bad) == L.VK_EINVAL, bad
    with pytest.raises(ValueError, match="layoutlm_embed"):
        L.call("vk_layoutlm_embed", p, p, p, 2, 17, p, 50, p, 16, p, p, p, p, 1024, p, 2, p, p, p, 128, 1e-12, L.VK_F32, None)

    def labels(B=2, Lt=64, C=7, W=10, ld=8, dt=L.VK_F32, logits=p, wid=p):
        return lib.vk_token_word_labels(logits, ld, wid, B, Lt, C, W, p, p, dt, None)
    for bad in (dict(B=0), dict(Lt=0), dict(Lt=4097, W=1), dict(C=0), dict(C=65, ld=65), dict(ld=6), dict(W=0), dict(W=65),
                dict(dt=L.VK_I32), dict(logits=None), dict(wid=None)):
        assert labels(**bad) == L.VK_EINVAL, bad

    def span(B=2, Lt=64, mx=30, ss=2, es=2, dt=L.VK_F16, start=p, ctx=p):
        return lib.vk_span_select(start, ss, p, es, ctx, B, Lt, mx, p, p, p, dt, None)
    for bad in (dict(B=0), dict(Lt=0), dict(Lt=4097), dict(mx=0), dict(mx=-3), dict(ss=0), dict(es=0), dict(dt=L.VK_I64),
                dict(start=None), dict(ctx=None)):
        assert span(**bad) == L.VK_EINVAL, bad
    with pytest.raises(ValueError, match="span_select"):
        L.call("vk_span_select", p, 1, p, 1, p, 2, 4097, 30, p, p, p, L.VK_F32, None)


def test_lazy_exports():
    import vltk_amd
    for name in ("LayoutLMModel", "LayoutLMForTokenClassification", "LayoutLMForQuestionAnswering", "LayoutLMForSequenceClassification",
                 "layoutlm_config", "ocr_token_boxes"):
        assert getattr(vltk_amd, name) is getattr(LM, name)
