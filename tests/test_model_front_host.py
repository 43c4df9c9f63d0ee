"""CPU: what the five encoders share between a caller and `_forward` (vltk_amd/bert_ops.py): the comparison of a replay's inputs
with the captured call's and the refill of the captured buffers, on CPU tensors; the draw of the synthetic weights against digests
recorded before the draw was folded; the head loader's refusals, which need no GPU."""
import hashlib

import numpy as np
import pytest
import torch

from vltk_amd import bert_ops as BO
from vltk_amd import layoutlm as LM
from vltk_amd import lxmert as LX
from vltk_amd import lxmert_pretrain as LP
from vltk_amd import visualbert as VB
from vltk_amd import vit as VT

NAMES = ("input_ids", "visual_feats", "attention_mask", "token_type_ids")


def captured(B=3, Lt=5):
    """The buffers of a captured call that left `token_type_ids` out."""
    return [torch.zeros((B, Lt), dtype=torch.int64), torch.zeros((B, 4, 8)), torch.zeros((B, Lt)), None]


def fresh(B=3, Lt=5):
    gen = torch.Generator().manual_seed(B * 100 + Lt)
    return [torch.randint(1, 50, (B, Lt), generator=gen), torch.randn((B, 4, 8), generator=gen), torch.ones((B, Lt)), None]


# ---- the comparison with the captured call and the refill ---------------------------------------------------------------------------
def test_an_equal_call_passes_and_fills_the_buffers():
    static, new = captured(), fresh()
    before = [s if s is None else s.data_ptr() for s in static]
    BO.check_against_captured(NAMES, static, new)
    BO.refill(static, new)
    for s, n, ptr in zip(static[:3], new[:3], before[:3]):
        assert torch.equal(s, n) and s.data_ptr() == ptr                 # the same buffers, the new values
    assert static[3] is None                                             # None at capture stays None


def test_none_against_a_tensor_is_refused_both_ways():
    static = captured()
    with pytest.raises(ValueError, match="replay: token_type_ids differs from the captured call"):
        BO.check_against_captured(NAMES, static, fresh()[:3] + [torch.zeros((3, 5), dtype=torch.int64)])
    with pytest.raises(ValueError, match="replay: attention_mask differs from the captured call"):
        BO.check_against_captured(NAMES, static, fresh()[:2] + [None, None])
    assert static[3] is None and torch.equal(static[2], torch.zeros((3, 5)))      # a refusal writes nothing


def test_another_shape_is_refused():
    static = captured()
    with pytest.raises(ValueError, match="replay: input_ids differs"):
        BO.check_against_captured(NAMES, static, fresh(3, 6))
    new = fresh()
    new[1] = new[1][:, :3]
    with pytest.raises(ValueError, match="replay: visual_feats differs"):
        BO.check_against_captured(NAMES, static, new)


def test_a_broadcastable_shape_is_refused():
    """[1, L] against [B, L]: `Tensor.copy_` alone would take it and fill every row with the first."""
    static, new = captured(), fresh()
    new[2] = new[2][:1]
    unchecked = captured()[2]
    unchecked.copy_(new[2])                                              # what the refill would do unchecked
    assert torch.equal(unchecked, new[2].expand(3, 5))
    with pytest.raises(ValueError, match="replay: attention_mask differs"):
        BO.check_against_captured(NAMES, static, new)


# ---- the synthetic weights: byte for byte what they were before seeded_tensor learnt the gamma names ------------------------------------
LX_SMALL = dict(vocab_size=300, hidden_size=32, num_attention_heads=2, intermediate_size=64, l_layers=1, x_layers=1, r_layers=1,
                max_position_embeddings=16, visual_feat_dim=64)
PT_SMALL = dict(LX_SMALL, num_qa_labels=11, num_object_labels=13, num_attr_labels=7)
VB_SMALL = dict(vocab_size=300, hidden_size=32, num_attention_heads=2, num_hidden_layers=1, intermediate_size=64,
                max_position_embeddings=16, visual_embedding_dim=64)
LM_SMALL = dict(vocab_size=300, hidden_size=32, num_attention_heads=2, intermediate_size=64, num_hidden_layers=1,
                max_position_embeddings=16, max_2d_position_embeddings=16)
VT_SMALL = dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, image_size=16, patch_size=4)

DRAWS = {
    "lxmert": lambda: (LX.lxmert_param_spec(LX.lxmert_config(**LX_SMALL)), LX.make_lxmert_state_dict(LX.lxmert_config(**LX_SMALL), 3)),
    "lxmert_qa": lambda: (LX.lxmert_qa_param_spec(LX.lxmert_config(**LX_SMALL), 11),
                          LX.make_lxmert_qa_state_dict(LX.lxmert_config(**LX_SMALL), 11, 3)),
    "lxmert_pretraining": lambda: (LP.lxmert_pretraining_param_spec(LP.lxmert_pretraining_config(**PT_SMALL)),
                                   LP.make_lxmert_pretraining_state_dict(LP.lxmert_pretraining_config(**PT_SMALL), 3)),
    "lxmert_pretraining_untied": lambda: (
        LP.lxmert_pretraining_param_spec(LP.lxmert_pretraining_config(**PT_SMALL, tie_word_embeddings=False)),
        LP.make_lxmert_pretraining_state_dict(LP.lxmert_pretraining_config(**PT_SMALL, tie_word_embeddings=False), 3)),
    "visualbert": lambda: (VB.visualbert_param_spec(VB.visualbert_config(**VB_SMALL)),
                           VB.make_visualbert_state_dict(VB.visualbert_config(**VB_SMALL), 3)),
    "visualbert_qa": lambda: (VB.visualbert_qa_param_spec(VB.visualbert_config(**VB_SMALL), 9),
                              VB.make_visualbert_qa_state_dict(VB.visualbert_config(**VB_SMALL), 9, 3)),
    "layoutlm": lambda: (LM.layoutlm_param_spec(LM.layoutlm_config(**LM_SMALL)), LM.make_layoutlm_state_dict(LM.layoutlm_config(**LM_SMALL), 3)),
    "layoutlm_token": lambda: (LM.layoutlm_head_param_spec(LM.layoutlm_config(**LM_SMALL), "classifier", 7),
                               LM.make_layoutlm_head_state_dict(LM.layoutlm_config(**LM_SMALL), "classifier", 7, 3)),
    "vit": lambda: (VT.vit_param_spec(VT.vit_config(**VT_SMALL)), VT.make_vit_state_dict(VT.vit_config(**VT_SMALL), 3)),
    "vit_classifier": lambda: (VT.vit_classifier_param_spec(VT.vit_config(**VT_SMALL), 5),
                               VT.make_vit_classifier_state_dict(VT.vit_config(**VT_SMALL), 5, 3)),
}
# SHA-256 over name, shape and bytes of every tensor in spec order, recorded by `weights_digest` on the commit before this file
DIGESTS = {
    "lxmert": "8b823214eb1ebbaf686f3984c4469b44464a69f1f4b125aa9dd4403aad80678f",
    "lxmert_qa": "d0d4b5c8c4344d5aea1b869c0039f964083d2cc7171f10612afb96dfc9290c31",
    "lxmert_pretraining": "7342d21a1ff18ca23e5374f8e7809ca2e92af0b29af4429171eaed9e5d62b7df",
    "lxmert_pretraining_untied": "32b508b93b4defc66268f3a4aeb23dea932df531de1099d23bf984ba102bde26",
    "visualbert": "f61d290c939b4c19039ad7751e434e85101315b52eb90cf937b5c8054618ad20",
    "visualbert_qa": "da8ddefee151db4f68a17750dc28f440c7fe05a1246082f1eb94bf293f3e84fb",
    "layoutlm": "a11dc200b15c51e21fb0ea740d72222aa38b0c27a7c63773e56786792cd6d378",
    "layoutlm_token": "23c1bf2b6d16f6aa0c0426ff7a0170239b132204e1fbe41d1fdd90f4c1485fc1",
    "vit": "db960f9a2f8f3fc8d86b0fc5e74d0eb503c10ca1fc63231b25f194020b760c72",
    "vit_classifier": "d8e786f18c3c115187f10b6828f2ad7004e3d5c72c54eab21c8691d9f6a55e63",
}


def weights_digest(spec, sd):
    h = hashlib.sha256()
    assert list(sd) == [k for k, _ in spec]
    for name, shape in spec:
        assert sd[name].shape == tuple(shape) and sd[name].dtype == np.float32
        h.update(name.encode() + repr(tuple(shape)).encode() + np.ascontiguousarray(sd[name]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("model", list(DRAWS))
def test_synthetic_weights_keep_their_bytes(model):
    """The golden files hold transformers' outputs for exactly these weights."""
    assert weights_digest(*DRAWS[model]()) == DIGESTS[model]


# ---- the head loader: one strict check of keys and shapes for every wrapper, before anything reaches the encoder ----------------------
class RecordingEncoder:
    """Stands where the encoder stands in a wrapper's `load_state_dict`: records what it is given, needs no GPU."""

    def __init__(self, cfg):
        self.cfg, self.loaded, self.lin, self.ln = cfg, [], [], []

    def load_state_dict(self, sd, strict=True):
        self.loaded.append((dict(sd), strict))

    def _load_lin(self, sd, name, *parts):
        self.lin.append((name, parts))

    def _load_ln(self, sd, name):
        self.ln.append(name)


def lxmert_qa(n=11):
    cfg = LX.lxmert_config(**LX_SMALL)
    m = object.__new__(LX.LxmertForQuestionAnswering)
    m.lxmert, m.num_qa_labels = RecordingEncoder(cfg), n
    return m, cfg, LX.make_lxmert_qa_state_dict(cfg, n, 3)


def test_head_loader_strips_the_prefix_and_hands_the_head_its_tensors():
    m, cfg, sd = lxmert_qa()
    assert m.load_state_dict(sd) is m and m.eval() is m
    (given, strict), = m.lxmert.loaded
    assert strict is True and list(given) == [k for k, _ in LX.lxmert_param_spec(cfg)]        # every encoder tensor, no head tensor
    assert all(given[k] is sd["lxmert." + k] for k in given)
    assert m.lxmert.lin == [("answer.fc0", ("answer_head.logit_fc.0",)), ("answer.fc3", ("answer_head.logit_fc.3",))]
    assert m.lxmert.ln == ["answer_head.logit_fc.2"]


def test_head_loader_refuses_missing_and_unexpected_keys():
    m, _, sd = lxmert_qa()
    short = dict(sd)
    del short["answer_head.logit_fc.0.bias"]
    with pytest.raises(RuntimeError, match=r"LxmertForQuestionAnswering.load_state_dict: missing \['answer_head.logit_fc.0.bias'\]"):
        m.load_state_dict(short)
    with pytest.raises(RuntimeError, match=r"unexpected \['answer_head.logit_fc.4.weight'\]"):
        m.load_state_dict(dict(sd, **{"answer_head.logit_fc.4.weight": sd["answer_head.logit_fc.3.weight"]}))
    assert m.load_state_dict(dict(sd, stray=sd["lxmert.pooler.dense.bias"]), strict=False) is m      # not strict: extra keys pass
    assert len(m.lxmert.loaded) == 1 and "stray" not in m.lxmert.loaded[0][0]


def test_head_loader_checks_the_shapes_of_the_head_tensors():
    """One row too many in the answer head's last weight: refused by shape, before `_pack` sees it."""
    m, _, sd = lxmert_qa()
    w = sd["answer_head.logit_fc.3.weight"]
    with pytest.raises(RuntimeError, match=r"'answer_head.logit_fc.3.weight' has shape \(12, 64\), expected \(11, 64\)"):
        m.load_state_dict(dict(sd, **{"answer_head.logit_fc.3.weight": np.concatenate((w, w[:1]))}))
    assert m.lxmert.loaded == [] and m.lxmert.lin == []                  # refused before anything reached the encoder


def test_head_loader_rekeys_before_it_checks():
    """ViT: hub-era key names under `vit.` load; pre-training heads: the tied decoder may be absent, and is there for the head."""
    cfg = VT.vit_config(**VT_SMALL)
    m = object.__new__(VT.ViTForImageClassification)
    m.vit, m.num_labels = RecordingEncoder(cfg), 5
    sd = VT.make_vit_classifier_state_dict(cfg, 5, 3)
    hub = {k.replace("vit.layers.0.attention.q_proj.", "vit.encoder.layer.0.attention.attention.query."): v for k, v in sd.items()}
    assert set(hub) != set(sd)
    m.load_state_dict(hub)
    assert set(m.vit.loaded[0][0]) == {k for k, _ in VT.vit_param_spec(cfg, add_pooling_layer=False)}
    cfg = LP.lxmert_pretraining_config(**PT_SMALL)
    m = object.__new__(LP.LxmertForPreTraining)
    m.cfg, m.lxmert = cfg, RecordingEncoder(cfg)
    m.lxmert._lin, m.lxmert._pack = {}, lambda w, b: (w, b)
    sd = LP.make_lxmert_pretraining_state_dict(cfg, 3)
    m.load_state_dict({k: v for k, v in sd.items() if k != LP.DECODER})
    assert m.lxmert._lin["cls.predictions.decoder"][0] is sd[LP.WORDS] and LP.DECODER not in m.lxmert.loaded[0][0]
    with pytest.raises(RuntimeError, match="differs"):
        m.load_state_dict(dict(sd, **{LP.DECODER: sd[LP.WORDS] + 1}))
