"""N3: the LXMERT-style vision-language encoder that consumes the extractor's output.

The reference hands `roi_features [B,36,2048]` and `boxes [B,36,4]` to transformers' LXMERT
(`vltk/legacy/legacy_train.py:30-39`; `transformers` is a dependency of the reference, `requirements.txt`).  This module is
the host-side mirror of `transformers.LxmertModel` (modeling_lxmert.py v5.15: `LxmertModel.forward` :691-824,
`LxmertEncoder.forward` :498-557) with the state-dict key layout of that class, so a real checkpoint's tensors load by
name.  All arithmetic runs in `libvltk_hip.so` (MFMA GEMM with bias / residual / GELU / tanh epilogues, LayerNorm,
attention, embedding kernels); torch only owns the device buffers.  No CPU fallback.

`LxmertForQuestionAnswering` is here too; the pre-training heads and their losses (`LxmertForPreTraining`) are in
lxmert_pretrain.py, which shares the answer head and the cross-entropy helpers below with it.
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, BertOps, Model, additive_mask, attention_spec, bert_layer_spec, check_text_inputs, dense_ln_spec, host_array, \
    keep_head, seeded_tensor, to_numpy
from .layers import stream

DEFAULT_CONFIG = dict(vocab_size=30522, hidden_size=768, num_attention_heads=12, intermediate_size=3072, l_layers=9, x_layers=5,
                      r_layers=5, max_position_embeddings=512, type_vocab_size=2, visual_feat_dim=2048, visual_pos_dim=4)


def lxmert_config(**kw):
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(kw)
    assert cfg["hidden_size"] % cfg["num_attention_heads"] == 0
    return cfg


def lxmert_param_spec(cfg):
    """(name, shape) of every tensor of `transformers.LxmertModel(config).state_dict()`, in its order."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    spec = [("embeddings.word_embeddings.weight", (cfg["vocab_size"], H)),
            ("embeddings.position_embeddings.weight", (cfg["max_position_embeddings"], H)),
            ("embeddings.token_type_embeddings.weight", (cfg["type_vocab_size"], H)),
            ("embeddings.LayerNorm.weight", (H,)), ("embeddings.LayerNorm.bias", (H,)),
            ("encoder.visn_fc.visn_fc.weight", (H, cfg["visual_feat_dim"])), ("encoder.visn_fc.visn_fc.bias", (H,)),
            ("encoder.visn_fc.visn_layer_norm.weight", (H,)), ("encoder.visn_fc.visn_layer_norm.bias", (H,)),
            ("encoder.visn_fc.box_fc.weight", (H, cfg["visual_pos_dim"])), ("encoder.visn_fc.box_fc.bias", (H,)),
            ("encoder.visn_fc.box_layer_norm.weight", (H,)), ("encoder.visn_fc.box_layer_norm.bias", (H,))]
    for i in range(cfg["l_layers"]):
        spec += bert_layer_spec(f"encoder.layer.{i}", H, I)
    for i in range(cfg["x_layers"]):
        p = f"encoder.x_layers.{i}"
        spec += attention_spec(p + ".visual_attention.att", H) + dense_ln_spec(p + ".visual_attention.output", H, H)
        spec += attention_spec(p + ".lang_self_att.self", H) + dense_ln_spec(p + ".lang_self_att.output", H, H)
        spec += attention_spec(p + ".visn_self_att.self", H) + dense_ln_spec(p + ".visn_self_att.output", H, H)
        spec += [(p + ".lang_inter.dense.weight", (I, H)), (p + ".lang_inter.dense.bias", (I,))] + dense_ln_spec(p + ".lang_output", I, H)
        spec += [(p + ".visn_inter.dense.weight", (I, H)), (p + ".visn_inter.dense.bias", (I,))] + dense_ln_spec(p + ".visn_output", I, H)
    for i in range(cfg["r_layers"]):
        spec += bert_layer_spec(f"encoder.r_layers.{i}", H, I)
    spec += [("pooler.dense.weight", (H, H)), ("pooler.dense.bias", (H,))]
    return spec


def lxmert_qa_param_spec(cfg, num_qa_labels):
    """`transformers.LxmertForQuestionAnswering(config).state_dict()`: the encoder under `lxmert.` + the answer head."""
    H = cfg["hidden_size"]
    return [("lxmert." + k, s) for k, s in lxmert_param_spec(cfg)] + [
        ("answer_head.logit_fc.0.weight", (2 * H, H)), ("answer_head.logit_fc.0.bias", (2 * H,)),
        ("answer_head.logit_fc.2.weight", (2 * H,)), ("answer_head.logit_fc.2.bias", (2 * H,)),
        ("answer_head.logit_fc.3.weight", (num_qa_labels, 2 * H)), ("answer_head.logit_fc.3.bias", (num_qa_labels,))]


def make_lxmert_qa_state_dict(cfg, num_qa_labels, seed=0):
    sd = {"lxmert." + k: v for k, v in make_lxmert_state_dict(cfg, seed).items()}
    for name, shape in lxmert_qa_param_spec(cfg, num_qa_labels)[-6:]:
        sd[name] = seeded_tensor(name, shape, seed)
    return sd


def make_lxmert_state_dict(cfg, seed=0):
    """Seeded synthetic weights (no checkpoint can be fetched offline): BERT-style N(0, 0.05) matrices (wider than the
    0.02 init so every layer matters in a parity check), LayerNorm gamma ~ U(0.5, 1.5), small biases."""
    return {name: seeded_tensor(name, shape, seed) for name, shape in lxmert_param_spec(cfg)}


class LxmertEncoder(BertOps):
    """`transformers.LxmertModel` on the HIP path: `model(input_ids, visual_feats, visual_pos, attention_mask=None,
    visual_attention_mask=None, token_type_ids=None)` -> (language_output, vision_output, pooled_output)."""

    _INPUTS = ("input_ids", "visual_feats", "visual_pos", "attention_mask", "visual_attention_mask", "token_type_ids")

    def load_state_dict(self, sd, strict=True):
        sd = to_numpy(sd)
        self._check_state_dict(sd, dict(lxmert_param_spec(self.cfg)), strict)
        lin, ln = (lambda name, *parts: self._load_lin(sd, name, *parts)), (lambda name: self._load_ln(sd, name))
        for t in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
            self._load_tab(sd, t)
        ln("embeddings.LayerNorm")
        lin("encoder.visn_fc.visn_fc", "encoder.visn_fc.visn_fc")
        lin("encoder.visn_fc.box_fc", "encoder.visn_fc.box_fc")
        ln("encoder.visn_fc.visn_layer_norm")
        ln("encoder.visn_fc.box_layer_norm")
        for i in range(self.cfg["l_layers"]):
            self._load_bert_layer(sd, f"encoder.layer.{i}")
        for i in range(self.cfg["r_layers"]):
            self._load_bert_layer(sd, f"encoder.r_layers.{i}")
        for i in range(self.cfg["x_layers"]):
            p = f"encoder.x_layers.{i}"
            lin(p + ".visual_attention.att.q", p + ".visual_attention.att.query")
            lin(p + ".visual_attention.att.kv", p + ".visual_attention.att.key", p + ".visual_attention.att.value")
            lin(p + ".visual_attention.output.dense", p + ".visual_attention.output.dense")
            ln(p + ".visual_attention.output.LayerNorm")
            for m in ("lang", "visn"):
                self._load_att_self(sd, f"{p}.{m}_self_att.self")
                lin(f"{p}.{m}_self_att.output.dense", f"{p}.{m}_self_att.output.dense")
                ln(f"{p}.{m}_self_att.output.LayerNorm")
                lin(f"{p}.{m}_inter.dense", f"{p}.{m}_inter.dense")
                lin(f"{p}.{m}_output.dense", f"{p}.{m}_output.dense")
                ln(f"{p}.{m}_output.LayerNorm")
        lin("pooler.dense", "pooler.dense")
        self._loaded = True
        return self

    def _cross_att_block(self, p, x, ctx_in, ctx_mask, B, Lx, Lc):   # LxmertCrossAttentionLayer :283-295
        H = self.cfg["hidden_size"]
        q = self._linear(x, p + ".att.q")
        kv = self._linear(ctx_in, p + ".att.kv")
        ctx = self._attention(q, kv[:, :H], kv[:, H:], ctx_mask, B, Lx, Lc)
        t = self._linear(ctx, p + ".output.dense", residual=x)
        return self._layernorm(t, p + ".output.LayerNorm")

    def capture(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None):
        """Capture one forward for these input SHAPES into a HIP graph (~430 launches become one graph launch: the
        small-batch forward is launch-bound).  Returns `replay(input_ids, visual_feats, visual_pos, ...)`, which checks the
        new ids on the host, copies the new inputs into the captured buffers, launches the graph and returns the (static) output tensors.
        A replay with None where the capture had a tensor (or the reverse), or with another shape, raises ValueError."""
        run = self._capture_inputs((input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids))

        def replay(input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None):
            return run((input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids))
        return replay

    def _check(self, input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids):
        check_text_inputs(input_ids, token_type_ids, self.cfg)

    def __call__(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None):
        return self._run(self._forward, (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids))

    @torch.no_grad()
    def _forward(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None):
        self._require_loaded()
        cfg, dev = self.cfg, self.device
        B, Lq = input_ids.shape
        V = visual_feats.shape[1]
        H = cfg["hidden_size"]
        ids = input_ids.to(dev, torch.int64).contiguous()
        tts = (torch.zeros_like(ids) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous())
        lmask = additive_mask(torch.ones((B, Lq), device=dev) if attention_mask is None else attention_mask, dev)
        vmask = additive_mask(visual_attention_mask, dev)
        # embeddings :191-214
        lang = torch.empty((B * Lq, H), dtype=self.tdt, device=dev)
        g, b = self._ln["embeddings.LayerNorm"]
        L.call("vk_embed_layernorm", ids.data_ptr(), tts.data_ptr(), B, Lq, self._tab["word_embeddings"].data_ptr(),
               self._tab["position_embeddings"].data_ptr(), self._tab["token_type_embeddings"].data_ptr(), g.data_ptr(), b.data_ptr(),
               lang.data_ptr(), H, LN_EPS, self.dt, stream(self.device))
        # visual feature encoder :468-476: (LN(fc(feats)) + LN(fc(pos))) / 2
        vf = visual_feats.to(dev).reshape(B * V, -1).to(self.tdt).contiguous()
        vp = visual_pos.to(dev).reshape(B * V, -1).to(self.tdt).contiguous()
        visn = self._layernorm(self._linear(vf, "encoder.visn_fc.visn_fc"), "encoder.visn_fc.visn_layer_norm", scale=0.5)
        self._layernorm(self._linear(vp, "encoder.visn_fc.box_fc"), "encoder.visn_fc.box_layer_norm", out=visn, scale=0.5, accumulate=True)
        # encoder :521-546
        for i in range(cfg["l_layers"]):
            lang = self._bert_layer(f"encoder.layer.{i}", lang, lmask, B, Lq)
        for i in range(cfg["r_layers"]):
            visn = self._bert_layer(f"encoder.r_layers.{i}", visn, vmask, B, V)
        for i in range(cfg["x_layers"]):
            p = f"encoder.x_layers.{i}"
            # cross attention, both directions through the SAME module (:377-398)
            l_att = self._cross_att_block(p + ".visual_attention", lang, visn, vmask, B, Lq, V)
            v_att = self._cross_att_block(p + ".visual_attention", visn, lang, lmask, B, V, Lq)
            l_att = self._self_att_block(p + ".lang_self_att", l_att, lmask, B, Lq)
            v_att = self._self_att_block(p + ".visn_self_att", v_att, vmask, B, V)
            lang = self._ffn(p + ".lang_inter", p + ".lang_output", l_att)
            visn = self._ffn(p + ".visn_inter", p + ".visn_output", v_att)
        return lang.view(B, Lq, H), visn.view(B, V, H), self._pooler(lang, B, Lq)


IGNORE_INDEX = -100                      # `CrossEntropyLoss`'s default, what the reference's `config.ignore_id` carries


def check_class_labels(name, t, shape, num_classes):
    """One tensor of class labels, host-side, before any launch: integer, of `shape`, every entry IGNORE_INDEX or in
    [0, num_classes).  -> int64 numpy array.  A wrong shape or type raises ValueError, a label outside IndexError (torch's
    cross-entropy would fault on the device there)."""
    a = host_array(t)
    if tuple(a.shape) != tuple(shape) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be an integer {tuple(shape)} array, got {a.dtype} {tuple(a.shape)}")
    bad = (a != IGNORE_INDEX) & ((a < 0) | (a >= num_classes))
    if bad.any():
        raise IndexError(f"{name} must be {IGNORE_INDEX} or lie in [0, {num_classes}): found {int(a[bad].flat[0])}")
    return np.ascontiguousarray(a, np.int64)


def load_answer_head(enc, sd):
    """`LxmertVisualAnswerHead` :602-614 into the encoder's packed weights."""
    enc._load_lin(sd, "answer.fc0", "answer_head.logit_fc.0")
    enc._load_lin(sd, "answer.fc3", "answer_head.logit_fc.3")
    enc._load_ln(sd, "answer_head.logit_fc.2")
    keep_head(enc, sd, "answer_head.logit_fc.0", "answer_head.logit_fc.2", "answer_head.logit_fc.3")


def answer_head(enc, pooled):
    h = enc._linear(pooled, "answer.fc0", act=L.VK_ACT_GELU)
    h = enc._layernorm(h, "answer_head.logit_fc.2")
    return enc._linear(h, "answer.fc3")


def cross_entropy_rows(enc, logits, labels):
    """`CrossEntropyLoss(reduction="none")` of logits [M, C] (storage type, unit column stride, any row stride) under int64
    device labels [M] -> fp32 [M]."""
    M, Cn = logits.shape
    assert logits.stride(1) == 1 and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == M
    rows = torch.empty((M,), dtype=torch.float32, device=enc.device)
    L.call("vk_cross_entropy", logits.data_ptr(), logits.stride(0), M, Cn, labels.data_ptr(), IGNORE_INDEX, rows.data_ptr(), enc.dt,
           stream(enc.device))
    return rows


def cross_entropy_mean(enc, logits, labels, out):
    """`CrossEntropyLoss()` into the fp32 device scalar `out`: the mean over the rows whose label is not IGNORE_INDEX."""
    rows = cross_entropy_rows(enc, logits, labels)
    L.call("vk_loss_reduce", rows.data_ptr(), None, labels.data_ptr(), IGNORE_INDEX, rows.numel(), 1.0, out.data_ptr(), stream(enc.device))


class LxmertForQuestionAnswering(Model):
    """`transformers.LxmertForQuestionAnswering` (modeling_lxmert.py :1123-1290, the VQA/GQA model of BASELINE config 5) on the
    HIP path: encoder + `LxmertVisualAnswerHead` :602-614 (Linear -> GELU -> LayerNorm -> Linear on the pooled output).
    `model(...)` returns `question_answering_score [B, num_qa_labels]` (storage dtype); with `labels=` it returns (loss, score)."""

    def __init__(self, config, num_qa_labels, precision="bf16", device="cuda:0"):
        self.lxmert = LxmertEncoder(config, precision, device)
        self.num_qa_labels = int(num_qa_labels)

    def load_state_dict(self, sd, strict=True):
        enc = self.lxmert
        load_answer_head(enc, self._load_with_encoder(enc, "lxmert.", lxmert_qa_param_spec(enc.cfg, self.num_qa_labels), sd, strict))
        return self

    def _head_features(self, *inputs):
        return self.lxmert._forward(*inputs)[2]

    def head_features(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None):
        """What the answer head consumes: the pooled output [B, H], storage type (`HeadTrainer.step_features` takes it)."""
        return self.lxmert._run(self._head_features, (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids))

    @torch.no_grad()
    def __call__(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                 labels=None):
        """`labels [B]` (an answer id each, -100 to leave an example out) -> (loss, score): `CrossEntropyLoss()` of the scores
        (:1270-1272), fp32, from `vk_cross_entropy` + `vk_loss_reduce`.  Without labels: the score alone."""
        enc = self.lxmert

        def forward(*inputs):
            lab = None if labels is None else check_class_labels("labels", labels, (input_ids.shape[0],), self.num_qa_labels)
            score = answer_head(enc, self._head_features(*inputs))
            if lab is None:
                return score
            loss = torch.empty((), dtype=torch.float32, device=enc.device)
            cross_entropy_mean(enc, score, torch.from_numpy(lab).to(enc.device), loss)
            return loss, score
        return enc._run(forward, (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids))
