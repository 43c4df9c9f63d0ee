"""N6: LXMERT's pre-training heads and their losses.  The reference's language processors (`vltk/processing/lang.py`:
`masked_language_modeling` writes `masked_labels` with `config.ignore_id`, `masked_feature_modeling` writes `feat_mask`,
`matched_sentence_modeling` writes `is_matched`; `vltk/configs.py` `PretrainConfig`) prepare the batches of LXMERT's three
pre-training tasks; the model they feed is `transformers.LxmertForPreTraining`, which the reference never shipped.

Host-side mirror of that class (modeling_lxmert.py v5.15 :826-1115; the heads :575-657) with its state-dict key layout, so a real
checkpoint's tensors load by name.  The heads are GEMMs and LayerNorms of `bert_ops.BertOps`; the losses are the kernels of
csrc/losses.hip (`vk_cross_entropy`, `vk_smooth_l1_rows`, `vk_loss_reduce`, `vk_loss_total`).  Logits come in the storage type,
losses in fp32.  All arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No CPU fallback.

Out of scope: backward passes and optimisers, the random masking itself (the reference draws it with Python's `random` on the
host), `inputs_embeds`, `output_attentions` / `output_hidden_states`.
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import Model, check_against_captured, check_text_inputs, dense_ln_spec, refill, seeded_tensor
from .layers import stream
from .lxmert import (IGNORE_INDEX, LxmertEncoder, answer_head, check_class_labels, cross_entropy_mean, cross_entropy_rows,
                     load_answer_head, lxmert_config, lxmert_param_spec)

PRETRAIN_DEFAULTS = dict(num_qa_labels=9500, num_object_labels=1600, num_attr_labels=400, task_mask_lm=True, task_obj_predict=True,
                         task_matched=True, task_qa=True, visual_obj_loss=True, visual_attr_loss=True, visual_feat_loss=True,
                         visual_loss_normalizer=6.67, tie_word_embeddings=True)
TERMS = ("mlm", "matched", "obj", "attr", "feat", "ans")       # the order of vk_loss_total's terms
DECODER, WORDS = "cls.predictions.decoder.weight", "lxmert.embeddings.word_embeddings.weight"


def lxmert_pretraining_config(**kw):
    """`lxmert_config` + the pre-training keys, with `transformers.LxmertConfig`'s defaults."""
    return lxmert_config(**{**PRETRAIN_DEFAULTS, **kw})


def visual_losses(cfg):
    """The visual losses the config enables, in transformers' order: [(key, columns of its decoder)]."""
    return [(k, n) for k, on, n in (("obj", cfg["visual_obj_loss"], cfg["num_object_labels"]),
                                    ("attr", cfg["visual_attr_loss"], cfg["num_attr_labels"]),
                                    ("feat", cfg["visual_feat_loss"], cfg["visual_feat_dim"])) if on]


def lxmert_pretraining_param_spec(cfg):
    """(name, shape) of every tensor of `transformers.LxmertForPreTraining(config).state_dict()`, in its order."""
    H = cfg["hidden_size"]
    spec = [("lxmert." + k, s) for k, s in lxmert_param_spec(cfg)]
    spec += [("cls.predictions.bias", (cfg["vocab_size"],))] + dense_ln_spec("cls.predictions.transform", H, H)
    spec += [(DECODER, (cfg["vocab_size"], H)), ("cls.seq_relationship.weight", (2, H)), ("cls.seq_relationship.bias", (2,))]
    if cfg["task_obj_predict"]:
        spec += dense_ln_spec("obj_predict_head.transform", H, H)
        for key, n in visual_losses(cfg):
            spec += [(f"obj_predict_head.decoder_dict.{key}.weight", (n, H)), (f"obj_predict_head.decoder_dict.{key}.bias", (n,))]
    if cfg["task_qa"]:
        spec += [("answer_head.logit_fc.0.weight", (2 * H, H)), ("answer_head.logit_fc.0.bias", (2 * H,)),
                 ("answer_head.logit_fc.2.weight", (2 * H,)), ("answer_head.logit_fc.2.bias", (2 * H,)),
                 ("answer_head.logit_fc.3.weight", (cfg["num_qa_labels"], 2 * H)), ("answer_head.logit_fc.3.bias", (cfg["num_qa_labels"],))]
    return spec


def make_lxmert_pretraining_state_dict(cfg, seed=0):
    """Seeded synthetic weights, drawn as `make_lxmert_state_dict` draws them.  The encoder's tensors are the ones that function
    gives for the same seed (under `lxmert.`); the decoder over the word table is tied, or a draw of its own when
    `tie_word_embeddings` is off."""
    sd = {}
    for name, shape in lxmert_pretraining_param_spec(cfg):
        key = name[len("lxmert."):] if name.startswith("lxmert.") else name
        if key == "answer_head.logit_fc.2.weight":
            key = "answer_head.logit_fc.2.LayerNorm.weight"          # the name this gamma's generator has been keyed by from the start
        sd[name] = seeded_tensor(key, shape, seed)
    if cfg["tie_word_embeddings"]:
        sd[DECODER] = sd[WORDS]
    return sd


def resolve_decoder_weight(cfg, sd):
    """The weight of `cls.predictions.decoder` from a state dict of numpy arrays.  Tied (`tie_word_embeddings`): the word table;
    the key may be absent, and if present must equal the table, else RuntimeError.  Untied: the key is required and is used."""
    if not cfg["tie_word_embeddings"]:
        if DECODER not in sd:
            raise RuntimeError(f"tie_word_embeddings is off: the state dict must hold '{DECODER}'")
        return sd[DECODER]
    if DECODER in sd and not np.array_equal(sd[DECODER], sd[WORDS]):
        raise RuntimeError(f"tie_word_embeddings is on, but '{DECODER}' differs from '{WORDS}'")
    return sd[WORDS]


def _float_labels(name, t, shape, floating=False):
    """`conf` or the feature target: only its shape (and, for the target, its type) is checked, so a device tensor stays where it
    is.  -> contiguous fp32 torch tensor."""
    t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape) or (floating and not t.is_floating_point()):
        raise ValueError(f"{name} must be a{' float' if floating else 'n'} {tuple(shape)} array, got {t.dtype} {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def check_pretraining_labels(cfg, B, Lt, V, labels=None, matched_label=None, obj_labels=None, ans=None):
    """Everything the loss kernels trust about the labels, host-side (device tensors are read back), before any launch or
    capture.  A label of a task the config switches off is ignored, as upstream.  -> dict with keys among `labels`,
    `matched_label`, `ans`, and `<key>_label` / `<key>_conf` for the enabled visual losses: class labels as int64 numpy arrays,
    `conf` and the feature target as fp32 torch tensors on the device they came from.  Wrong shape or type: ValueError; a class
    label outside {-100} and [0, C): IndexError; an enabled visual loss that `obj_labels` lacks: KeyError."""
    out = {}
    if labels is not None and cfg["task_mask_lm"]:
        out["labels"] = check_class_labels("labels", labels, (B, Lt), cfg["vocab_size"])
    if matched_label is not None and cfg["task_matched"]:
        out["matched_label"] = check_class_labels("matched_label", matched_label, (B,), 2)
    if ans is not None and cfg["task_qa"]:
        out["ans"] = check_class_labels("ans", ans, (B,), cfg["num_qa_labels"])
    if obj_labels is not None and cfg["task_obj_predict"]:
        for key, n in visual_losses(cfg):
            label, conf = obj_labels[key]
            if key == "feat":
                out["feat_label"] = _float_labels("obj_labels['feat'] target", label, (B, V, n), floating=True)
            else:
                out[key + "_label"] = check_class_labels(f"obj_labels['{key}'] label", label, (B, V), n)
            out[key + "_conf"] = _float_labels(f"obj_labels['{key}'] conf", conf, (B, V))
    return out


def loss_only_index(labels):
    """Rows of `lang_output.view(B * Lt, H)` the loss-only mode decodes: those with a label other than -100, ascending.
    -> (index int32 [n], their labels int64 [n])."""
    flat = np.asarray(labels).reshape(-1)
    idx = np.flatnonzero(flat != IGNORE_INDEX)
    return idx.astype(np.int32), np.ascontiguousarray(flat[idx], np.int64)


class LxmertForPreTrainingOutput:
    """`loss`: fp32 device scalar, None when no label was given.  `losses`: the terms present, fp32 device scalars under the keys
    mlm, matched, obj, attr, feat, ans.  `prediction_logits [B, Lt, vocab]` (None in the loss-only mode),
    `cross_relationship_score [B, 2]`, `question_answering_score [B, num_qa_labels]` (None without `task_qa`), storage type.
    `visual_prediction_scores`: what `obj_predict_head` gives, {"obj" | "attr" | "feat": [B * V, columns]} as column slices of
    the one GEMM; None unless `obj_labels` was given (upstream runs that head only then, and does not return its scores)."""

    def __init__(self, loss, losses, prediction_logits, cross_relationship_score, question_answering_score,
                 visual_prediction_scores=None):
        self.loss, self.losses = loss, losses
        self.prediction_logits, self.cross_relationship_score = prediction_logits, cross_relationship_score
        self.question_answering_score = question_answering_score
        self.visual_prediction_scores = visual_prediction_scores


class LxmertForPreTraining(Model):
    """`transformers.LxmertForPreTraining` on the HIP path: `model(input_ids, visual_feats, visual_pos, attention_mask=None,
    visual_attention_mask=None, token_type_ids=None, labels=None, matched_label=None, obj_labels=None, ans=None, logits=True)`
    -> `LxmertForPreTrainingOutput`.  `obj_labels` is transformers' dict {"obj": (label [B, V], conf [B, V]), "attr": (..),
    "feat": (target [B, V, D], conf [B, V])}.

    `logits=False` is the loss-only mode: it needs `labels`, and runs the transform, the decoder over the word table and the
    cross-entropy on the labelled rows only (`vk_gather_rows`, about 15 % of the rows at the reference's `word_mask_rate`)."""

    def __init__(self, config, precision="bf16", device="cuda:0"):
        self.cfg = lxmert_pretraining_config(**config)
        self.lxmert = LxmertEncoder(self.cfg, precision, device)

    def load_state_dict(self, sd, strict=True):
        enc, cfg = self.lxmert, self.cfg
        sd = self._load_with_encoder(enc, "lxmert.", lxmert_pretraining_param_spec(cfg), sd, strict,
                                     rekey=lambda sd: {**sd, DECODER: resolve_decoder_weight(cfg, sd)})    # tied: the key may be absent
        enc._load_lin(sd, "cls.predictions.transform.dense", "cls.predictions.transform.dense")
        enc._load_ln(sd, "cls.predictions.transform.LayerNorm")
        enc._lin["cls.predictions.decoder"] = enc._pack(sd[DECODER], sd["cls.predictions.bias"])     # a packed copy of the table
        enc._load_lin(sd, "cls.seq_relationship", "cls.seq_relationship")
        if cfg["task_obj_predict"]:
            enc._load_lin(sd, "obj_predict_head.transform.dense", "obj_predict_head.transform.dense")
            enc._load_ln(sd, "obj_predict_head.transform.LayerNorm")
            keys = [k for k, _ in visual_losses(cfg)]
            if keys:                                     # the decoders share their input: one GEMM, columns side by side
                enc._load_lin(sd, "obj_predict_head.decoders", *[f"obj_predict_head.decoder_dict.{k}" for k in keys])
        if cfg["task_qa"]:
            load_answer_head(enc, sd)
        return self

    # ---- inputs ---------------------------------------------------------------------------------------------------------
    def _check(self, inputs, label_args):
        """Host checks of one call -> the labels as numpy arrays (check_pretraining_labels)."""
        input_ids, visual_feats = inputs[0], inputs[1]
        check_text_inputs(input_ids, inputs[5], self.cfg)
        B, Lt = input_ids.shape
        return check_pretraining_labels(self.cfg, B, Lt, visual_feats.shape[1], *label_args)

    def _to_device(self, lab):
        return {k: torch.as_tensor(v).to(self.lxmert.device) for k, v in lab.items()}

    # ---- the heads and the losses (no host reads: this is what a graph captures) -------------------------------------------
    def _transform(self, p, x):                          # LxmertPredictionHeadTransform :575-586
        enc = self.lxmert
        return enc._layernorm(enc._linear(x, p + ".dense", act=L.VK_ACT_GELU), p + ".LayerNorm")

    def _weighted_mean(self, rows, conf, out):           # (loss * mask_conf.view(-1)).mean() * visual_loss_normalizer  :1090
        enc = self.lxmert
        L.call("vk_loss_reduce", rows.data_ptr(), conf.data_ptr(), None, IGNORE_INDEX, rows.numel(), float(self.cfg["visual_loss_normalizer"]),
               out.data_ptr(), stream(enc.device))

    def _visual_terms(self, visn, lab, terms, present):
        """-> (present with the visual terms' bits, {key: the key's columns of the visual GEMM})."""
        enc, cfg = self.lxmert, self.cfg
        keys = visual_losses(cfg)
        parts = {}
        if not keys:
            return present, parts
        scores = enc._linear(self._transform("obj_predict_head.transform", visn), "obj_predict_head.decoders")
        col = 0
        for key, n in keys:
            part, i = scores[:, col:col + n], TERMS.index(key)
            parts[key] = part
            col += n
            if key == "feat":
                target = lab["feat_label"].view(-1, n)
                rows = torch.empty((part.shape[0],), dtype=torch.float32, device=enc.device)
                L.call("vk_smooth_l1_rows", part.data_ptr(), part.stride(0), target.data_ptr(), n, part.shape[0], n, rows.data_ptr(),
                       enc.dt, stream(enc.device))
            else:
                rows = cross_entropy_rows(enc, part, lab[key + "_label"].view(-1))
            self._weighted_mean(rows, lab[key + "_conf"].view(-1), terms[i])
            present |= 1 << i
        return present, parts

    def _finish(self, terms, present, any_label):
        """-> (loss, losses) from the filled terms."""
        if not any_label:
            return None, {}
        enc = self.lxmert
        loss = torch.empty((), dtype=torch.float32, device=enc.device)
        L.call("vk_loss_total", terms.data_ptr(), present, loss.data_ptr(), stream(enc.device))
        return loss, {k: terms[i] for i, k in enumerate(TERMS) if present & (1 << i)}

    @torch.no_grad()
    def _forward(self, inputs, lab, any_label, logits=True, gather=None):
        """inputs: the encoder's six; lab: device labels (`_to_device`); gather: (index, labels) of the loss-only mode."""
        enc, cfg = self.lxmert, self.cfg
        lang, visn, pooled = enc._forward(*inputs)
        B, Lt, H = lang.shape
        lang, visn = lang.view(B * Lt, H), visn.view(-1, H)
        terms = torch.zeros((len(TERMS),), dtype=torch.float32, device=enc.device)
        present = 0
        prediction = visual = None
        if logits:
            scores = enc._linear(self._transform("cls.predictions.transform", lang), "cls.predictions.decoder")
            prediction = scores.view(B, Lt, cfg["vocab_size"])
            if "labels" in lab:
                cross_entropy_mean(enc, scores, lab["labels"].view(-1), terms[0])
                present |= 1
        else:
            idx, picked = gather
            if idx.numel():
                scores = enc._linear(self._transform("cls.predictions.transform", enc._gather_rows(lang, idx)), "cls.predictions.decoder")
                cross_entropy_mean(enc, scores, picked, terms[0])
            else:                  # no labelled row: no GEMM; the reduction over rows that all are ignored gives NaN, as torch
                unread = torch.empty((B * Lt,), dtype=torch.float32, device=enc.device)
                L.call("vk_loss_reduce", unread.data_ptr(), None, lab["labels"].data_ptr(), IGNORE_INDEX, B * Lt, 1.0, terms[0].data_ptr(),
                       stream(enc.device))
            present |= 1
        matched = enc._linear(pooled, "cls.seq_relationship")
        if "matched_label" in lab:
            cross_entropy_mean(enc, matched, lab["matched_label"], terms[1])
            present |= 2
        if "feat_conf" in lab or "obj_conf" in lab or "attr_conf" in lab:
            present, visual = self._visual_terms(visn, lab, terms, present)
        answer = answer_head(enc, pooled) if cfg["task_qa"] else None
        if "ans" in lab:
            cross_entropy_mean(enc, answer, lab["ans"], terms[5])
            present |= 0x20
        loss, losses = self._finish(terms, present, any_label)
        return LxmertForPreTrainingOutput(loss, losses, prediction, matched, answer, visual)

    def __call__(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                 labels=None, matched_label=None, obj_labels=None, ans=None, logits=True):
        enc = self.lxmert
        inputs = (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids)
        label_args = (labels, matched_label, obj_labels, ans)
        lab = self._check(inputs, label_args)
        gather = None
        if not logits:
            if "labels" not in lab:
                raise ValueError("logits=False (the loss-only mode) needs `labels` and a config with task_mask_lm")
            gather = tuple(torch.from_numpy(a).to(enc.device) for a in loss_only_index(lab["labels"]))
        out = self._forward(inputs, self._to_device(lab), any(a is not None for a in label_args), logits, gather)
        torch.cuda.synchronize(enc.device)
        return out

    def capture(self, input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                labels=None, matched_label=None, obj_labels=None, ans=None):
        """Capture one `logits=True` call for these SHAPES into a HIP graph.  Returns `replay(...)` with the model's signature
        (without `logits`), which repeats the host checks, copies the new inputs and labels into the captured buffers, launches
        the graph and returns the (static) output.  What was None at capture stays None."""
        enc = self.lxmert
        inputs = (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids)
        label_args = (labels, matched_label, obj_labels, ans)
        s_lab = {k: v.clone() for k, v in self._to_device(self._check(inputs, label_args)).items()}
        s_in = [None if a is None else a.to(enc.device).clone() for a in inputs]
        any_label = any(a is not None for a in label_args)
        graph, out = enc._capture(lambda: self._forward(s_in, s_lab, any_label), [])

        def replay(input_ids, visual_feats, visual_pos, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                   labels=None, matched_label=None, obj_labels=None, ans=None):
            new = (input_ids, visual_feats, visual_pos, attention_mask, visual_attention_mask, token_type_ids)
            check_against_captured(enc._INPUTS, s_in, new)
            lab = self._check(new, (labels, matched_label, obj_labels, ans))
            if set(lab) != set(s_lab):
                raise ValueError(f"replay: labels {sorted(lab)} differ from the captured call's {sorted(s_lab)}")
            refill(s_in, new)
            refill(s_lab.values(), [torch.as_tensor(lab[k]) for k in s_lab])     # their shapes follow from the inputs' (_check)
            graph.replay()
            return out
        return replay
