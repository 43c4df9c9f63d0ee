"""TEST INFRASTRUCTURE ONLY -- tests/golden/layoutlm_small.npz (tools/gen_golden_layoutlm.py): its models rebuilt from the seed, the
keyword arguments of each stored case, a CPU restatement of transformers' LayoutLM forward and its three heads, and numpy
restatements of the rules the two tail kernels and `ocr_token_boxes` follow.

`LayoutLMOracle` follows transformers/models/layoutlm/modeling_layoutlm.py (v5.15): LayoutLMEmbeddings.forward :66-119,
LayoutLMModel.forward :433-524 and the heads :649, :777, :879.  Its layers are BERT layers, the ones
`oracle.lxmert_oracle.LxmertOracle` restates (linear / ln / attention / bert_layer and their rounding points), so it subclasses
that; what it adds is the embedding stage and the heads.  It is pinned by the stored vectors of transformers itself
(tests/test_layoutlm_host.py).  `emulate="bf16"|"fp16"` rounds where the HIP path stores: the tables, the embedding output and
the GEMM outputs; the embedding sum stays fp32, as in csrc/layoutlm.hip.

The tail rules (`token_word_labels_ref`, `span_select_ref`) and the box rule (`ocr_token_boxes_ref`) are written as plain loops
over the rules' own words (include/vltk_hip.h, vltk_amd/layoutlm.py); the reference's processors do not import here, so parity
with them is unpinned for the rule.
"""
import math

import numpy as np
import torch

from oracle.lxmert_oracle import LxmertOracle
from vltk_amd.layoutlm import layoutlm_config, make_layoutlm_head_state_dict, make_layoutlm_state_dict

GEOMETRY = ("short", "long")
CASES = [(geo, case) for geo in GEOMETRY for case in ("plain", "masked", "nobox")]
HEADS = {"token": "classifier", "qa": "qa_outputs", "seq": "classifier"}


def golden_model(g):
    """-> (cfg, state dict of the bare model)."""
    cfg = layoutlm_config(**{k[4:]: int(g[k]) for k in g.files if k.startswith("cfg/")})
    return cfg, make_layoutlm_state_dict(cfg, int(g["seed"]))


def golden_head(g, head):
    """-> (cfg, num_labels, state dict) of one head ("token" | "qa" | "seq")."""
    cfg, _ = golden_model(g)
    n = int(g[f"{head}/num_labels"])
    return cfg, n, make_layoutlm_head_state_dict(cfg, HEADS[head], n, int(g["seed"]))


def case_kwargs(g, geo, case):
    """Keyword arguments of the stored case `<geo>/<case>` besides input_ids (numpy arrays)."""
    kw = {}
    if case != "nobox":
        kw["bbox"] = g[f"{geo}/bbox"]
    if case == "masked":
        kw.update({k: g[f"{geo}/{k}"] for k in ("attention_mask", "token_type_ids")})
    return kw


def stored_spec(g, tag, which):
    """The `state_dict()` names and shapes the generator recorded from transformers: tag "small" | "default", which "model" | head."""
    names, shapes = g[f"spec/{tag}/{which}/names"], g[f"spec/{tag}/{which}/shapes"]
    return [(str(n), tuple(int(v) for v in s if v)) for n, s in zip(names, shapes)]


class LayoutLMOracle(LxmertOracle):
    def embeddings(self, input_ids, bbox=None, token_type_ids=None):
        sd, q = self.sd, self.q
        ids = torch.as_tensor(np.asarray(input_ids)).long()
        B, Lt = ids.shape
        box = torch.zeros((B, Lt, 4), dtype=torch.long) if bbox is None else torch.as_tensor(np.asarray(bbox)).long()
        tts = torch.zeros_like(ids) if token_type_ids is None else torch.as_tensor(np.asarray(token_type_ids)).long()

        def tab(name):
            return q(sd[f"embeddings.{name}_embeddings.weight"])
        x, y = tab("x_position"), tab("y_position")
        e = tab("word")[ids] + tab("position")[:Lt][None]                     # :106-116, in that order
        e = e + x[box[..., 0]]
        e = e + y[box[..., 1]]
        e = e + x[box[..., 2]]
        e = e + y[box[..., 3]]
        e = e + tab("h_position")[box[..., 3] - box[..., 1]]
        e = e + tab("w_position")[box[..., 2] - box[..., 0]]
        e = e + tab("token_type")[tts]
        return q(self.ln(e, "embeddings.LayerNorm"))

    def forward(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, return_stages=False):
        x = self.embeddings(input_ids, bbox, token_type_ids)
        B, Lt = x.shape[:2]
        am = torch.ones((B, Lt)) if attention_mask is None else torch.as_tensor(np.asarray(attention_mask)).float()
        mask = ((1.0 - am) * torch.finfo(torch.float32).min)[:, None, None, :]
        st = {"embeddings": x}
        for i in range(self.cfg["num_hidden_layers"]):
            x = self.bert_layer(x, mask, f"encoder.layer.{i}")
        out = (x, self.linear(x[:, 0], "pooler.dense", act="tanh"))
        return (out, st) if return_stages else out

    def _bare(self, *args, **kw):
        """The model's forward from a head's state dict (the `layoutlm.` prefix)."""
        full = self.sd
        self.sd = {k[len("layoutlm."):]: v for k, v in full.items() if k.startswith("layoutlm.")}
        try:
            return self.forward(*args, **kw)
        finally:
            self.sd = full

    def token_forward(self, *args, **kw):                 # LayoutLMForTokenClassification :862-863 -> [B, L, num_labels]
        return self.linear(self._bare(*args, **kw)[0], "classifier")

    def qa_forward(self, *args, **kw):                    # LayoutLMForQuestionAnswering :972-975 -> (start, end), each [B, L]
        logits = self.linear(self._bare(*args, **kw)[0], "qa_outputs")
        return logits[..., 0], logits[..., 1]

    def seq_forward(self, *args, **kw):                   # LayoutLMForSequenceClassification :736-737 -> [B, num_labels]
        return self.linear(self._bare(*args, **kw)[1], "classifier")


# ---- the tail rules, as loops -----------------------------------------------------------------------------------------------------
def token_word_labels_ref(logits, word_ids, W):
    """logits [B, L, C] (any float array), word_ids [B, L] -> (token_labels [B, L], word_labels [B, W]) int32, by the rule of
    vk_token_word_labels: first arg-max under `v > best` from -inf; most frequent label per word, the smallest on a tie, -1 for
    a word without tokens; a word id outside [0, W) is no word."""
    logits = np.asarray(logits, np.float32)
    B, Lt, Cn = logits.shape
    tok = np.zeros((B, Lt), np.int32)
    words = np.full((B, W), -1, np.int32)
    for b in range(B):
        for t in range(Lt):
            best, lab = -math.inf, 0
            for c in range(Cn):
                v = float(logits[b, t, c])
                if v > best:
                    best, lab = v, c
            tok[b, t] = lab
        for w in range(W):
            counts = np.bincount(tok[b][np.asarray(word_ids[b]) == w], minlength=Cn)
            best = 0
            for c in range(Cn):
                if counts[c] > best:
                    best, words[b, w] = counts[c], c
    return tok, words


def span_select_ref(start_logits, end_logits, context_mask, max_answer_tokens):
    """[B, L] each -> (start [B], end [B]) int32, score [B] float32, by the rule of vk_span_select: the best pair s <= e of context
    tokens with e - s + 1 <= max_answer_tokens under `float32(start[s]) + float32(end[e]) > best` from -inf, scanning s upward
    and e upward within s; (-1, -1, -inf) if nothing wins."""
    st, en = np.asarray(start_logits, np.float32), np.asarray(end_logits, np.float32)
    ctx = np.asarray(context_mask) != 0
    B, Lt = st.shape
    s_out, e_out, sc_out = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, -np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for s in range(Lt):
                if not ctx[b, s]:
                    continue
                stop = min(Lt, s + max_answer_tokens)
                sc = st[b, s] + en[b, s:stop]             # one fp32 add per pair
                sc = np.where(ctx[b, s:stop] & ~np.isnan(sc), sc, -np.inf)
                k = int(np.argmax(sc))                    # the first of the largest: the smallest e
                if sc[k] > sc_out[b]:
                    s_out[b], e_out[b], sc_out[b] = s, s + k, sc[k]
    return s_out, e_out, sc_out


def ocr_token_boxes_ref(word_boxes_xywh, tokenmap, raw_wh, max_len, add_cls=False):
    """`ocr_token_boxes` as a loop over words and their tokens."""
    sx, sy = np.float32(1000) / np.float32(raw_wh[0]), np.float32(1000) / np.float32(raw_wh[1])
    boxes, ids = ([[0, 0, 1000, 1000]], [-1]) if add_cls else ([], [])
    for i, ((x, y, w, h), n) in enumerate(zip(word_boxes_xywh, tokenmap)):
        x, y, w, h = (np.float32(v) for v in (x, y, w, h))
        box = [(x * sx), (y * sy), ((x + w) * sx), ((y + h) * sy)]
        box = [int(math.floor(min(max(float(v), 0.0), 1000.0))) for v in box]
        boxes += [box] * int(n)
        ids += [i] * int(n)
    boxes, ids = boxes[:max_len], ids[:max_len]
    pad = max_len - len(ids)
    return (np.asarray(boxes + [[0, 0, 0, 0]] * pad, np.int64).reshape(max_len, 4), np.asarray(ids + [-1] * pad, np.int32))
