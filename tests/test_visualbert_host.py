"""CPU: the VisualBERT oracle (tests/visualbert_util.py) against vectors produced by transformers.VisualBertModel /
VisualBertForQuestionAnswering themselves, the build's parameter specs against those classes' state_dict, and the host-side
checks of vltk_amd/visualbert.py that run before any library call."""
import os

import numpy as np
import pytest
import torch

from vltk_amd import visualbert as VB

from visualbert_util import CASES, VisualBertOracle, case_kwargs, golden_inputs, golden_qa_state_dict


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "visualbert_small.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-9)


@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_oracle_vs_transformers_golden(g, geo, case):
    cfg, sd, feats = golden_inputs(g, geo)
    (seq, pooled), st = VisualBertOracle(cfg, sd).forward(g[f"{geo}/input_ids"], feats, return_stages=True, **case_kwargs(g, geo, case))
    tag = f"{geo}/{case}"
    assert seq.shape == g[f"{tag}/last_hidden_state"].shape
    assert rel(st["embeddings"], g[f"{tag}/embedding_output"]) <= 1e-5
    assert rel(seq, g[f"{tag}/last_hidden_state"]) <= 1e-5
    assert rel(pooled, g[f"{tag}/pooler_output"]) <= 1e-5


def test_golden_cases_exercise_what_they_claim(g):
    """The fixture's alignment has padding, a box with no valid entry and one whose only valid entry is not the first; the text
    masks are ragged; the aligned case differs from the masked one (so alignment and visual token types are live inputs)."""
    al = g["long/image_text_alignment"]
    assert al.shape == (2, 36, 3) and al.min() == -1 and (al[0, 5] == -1).all() and al[1, 7].tolist() == [-1, 19, -1]
    assert g["long/visual_token_type_ids"].min() == 0 and g["long/visual_token_type_ids"].max() == 1
    for geo in ("short", "long"):
        s = g[f"{geo}/attention_mask"].sum(1)
        assert len(set(s.tolist())) > 1 and s.min() >= 2
        assert g[f"{geo}/visual_attention_mask"][0, 30:].sum() == 0
    assert rel(g["long/aligned/embedding_output"], g["long/masked/embedding_output"]) > 1e-2


@pytest.mark.parametrize("geo", ["short", "long"])
def test_qa_oracle_vs_transformers_golden(g, geo):
    cfg, _, feats = golden_inputs(g, geo)
    kw = case_kwargs(g, geo, "masked")
    kw["attention_mask"] = kw["attention_mask"].astype(np.int64)
    logits = VisualBertOracle(cfg, golden_qa_state_dict(g)).qa_forward(g[f"{geo}/input_ids"], feats, **kw)
    assert rel(logits, g[f"qa/{geo}/logits"]) <= 1e-5


@pytest.mark.parametrize("emulate,tol", [("bf16", 6e-2), ("fp16", 1e-2)])
def test_emulation_stays_near_fp32(g, emulate, tol):
    """Storage roundings (bf16: 2^-8 relative each, fp16: 2^-11) through the embeddings and two layers stay within the bound the
    LXMERT oracle's emulation is held to (6e-2 for bf16; fp16 has 8x the precision)."""
    cfg, sd, feats = golden_inputs(g, "long")
    seq, pooled = VisualBertOracle(cfg, sd, emulate=emulate).forward(g["long/input_ids"], feats, **case_kwargs(g, "long", "aligned"))
    assert rel(seq, g["long/aligned/last_hidden_state"]) <= tol and rel(pooled, g["long/aligned/pooler_output"]) <= tol


def test_param_spec_matches_transformers():
    tr = pytest.importorskip("transformers")
    small = dict(vocab_size=500, hidden_size=128, num_attention_heads=4, intermediate_size=256, num_hidden_layers=2,
                 max_position_embeddings=64, visual_embedding_dim=2048)
    for kw in (small, {}):
        cfg = VB.visualbert_config(**kw)
        with torch.device("meta"):
            m = tr.VisualBertModel(tr.VisualBertConfig(**cfg))
            qa = tr.VisualBertForQuestionAnswering(tr.VisualBertConfig(num_labels=40, **cfg))
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in VB.visualbert_param_spec(cfg)]
        assert [(k, tuple(v.shape)) for k, v in qa.state_dict().items()] == [(k, tuple(s)) for k, s in VB.visualbert_qa_param_spec(cfg, 40)]


def test_config_defaults_and_bypass_transformer():
    cfg = VB.visualbert_config()
    assert (cfg["vocab_size"], cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["intermediate_size"]) == \
        (30522, 768, 12, 12, 3072)
    assert (cfg["max_position_embeddings"], cfg["type_vocab_size"], cfg["visual_embedding_dim"], cfg["layer_norm_eps"]) == (512, 2, 512, 1e-12)
    assert VB.visualbert_config(visual_embedding_dim=2048)["visual_embedding_dim"] == 2048
    with pytest.raises(NotImplementedError):
        VB.visualbert_config(bypass_transformer=True)


def test_synthetic_weights_are_seeded_per_tensor():
    cfg = VB.visualbert_config(vocab_size=50, hidden_size=32, num_attention_heads=2, intermediate_size=64, num_hidden_layers=1,
                               max_position_embeddings=8, visual_embedding_dim=64)
    a, b, c = VB.make_visualbert_state_dict(cfg, 3), VB.make_visualbert_state_dict(cfg, 3), VB.make_visualbert_state_dict(cfg, 4)
    assert list(a) == [k for k, _ in VB.visualbert_param_spec(cfg)]
    assert all(np.array_equal(a[k], b[k]) and a[k].shape == tuple(s) for k, s in VB.visualbert_param_spec(cfg))
    assert not np.array_equal(a["pooler.dense.weight"], c["pooler.dense.weight"])
    assert 0.5 <= a["embeddings.LayerNorm.weight"].min() and a["embeddings.LayerNorm.weight"].max() <= 1.5
    qa = VB.make_visualbert_qa_state_dict(cfg, 7, 3)
    assert list(qa) == [k for k, _ in VB.visualbert_qa_param_spec(cfg, 7)] and qa["cls.weight"].shape == (7, 32)
    assert np.array_equal(qa["visual_bert.pooler.dense.bias"], a["pooler.dense.bias"])


def test_alignment_is_checked_on_the_host():
    """A > 16, an index >= max_position, an index below -1, a float array and a wrong box count raise before any library call
    (these functions never load the library)."""
    ok = np.full((2, 5, 16), -1, np.int64)
    ok[0, 0, 0] = 63
    VB.check_alignment(ok, 2, 5, 64)
    VB.check_alignment(torch.from_numpy(ok), 2, 5, 64)
    with pytest.raises(ValueError):
        VB.check_alignment(np.zeros((2, 5, 17), np.int64), 2, 5, 64)
    bad = ok.copy()
    bad[1, 4, 15] = 64
    with pytest.raises(IndexError):
        VB.check_alignment(bad, 2, 5, 64)
    bad[1, 4, 15] = -2
    with pytest.raises(IndexError):
        VB.check_alignment(bad, 2, 5, 64)
    with pytest.raises(ValueError):
        VB.check_alignment(ok.astype(np.float32), 2, 5, 64)
    with pytest.raises(ValueError):
        VB.check_alignment(ok, 2, 6, 64)


def test_qa_gather_index():
    """Row b * (Lt + V) + (text mask's sum - 2), for a ragged mask of either type; None is all ones; fewer than two tokens (or
    a mask of the wrong shape) raise."""
    m = np.ones((3, 11), np.float32)
    m[1, 7:] = 0
    m[2, 2:] = 0
    want = [0 * 47 + 9, 1 * 47 + 5, 2 * 47 + 0]
    for mask in (m, m.astype(np.int64), torch.from_numpy(m)):
        idx = VB.qa_gather_index(mask, 3, 11, 36)
        assert idx.dtype == np.int32 and idx.tolist() == want
    assert VB.qa_gather_index(None, 2, 20, 36).tolist() == [18, 56 + 18]
    m[2, 1] = 0                                             # one token left: index -1
    with pytest.raises(IndexError):
        VB.qa_gather_index(m, 3, 11, 36)
    with pytest.raises(IndexError):
        VB.qa_gather_index(None, 2, 1, 36)
    with pytest.raises(ValueError):
        VB.qa_gather_index(np.ones((3, 47), np.float32), 3, 11, 36)


def test_lazy_exports():
    import vltk_amd
    assert vltk_amd.VisualBertModel is VB.VisualBertModel
    assert vltk_amd.VisualBertForQuestionAnswering is VB.VisualBertForQuestionAnswering
