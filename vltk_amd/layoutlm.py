"""The document half of the reference: the encoder its OCR data is prepared for.  The `FUNSD` / `DocVQA` adapters
(`vltk/adapters/funsd.py`, `docvqa.py`) store OCR words with one `tokenbox` each; `vltk/processing/visn.py` (`XYWHtoXYXY`,
`OCRBox`, `OCRBoxFixed`, `TokenLabels`) expands them to one box per sub-token in 0..1000, and `vltk/utils/adapters.py`
`map_ocr_predictions` folds per-token predictions back into one per word.  That is LayoutLM's input and output contract; the
reference never shipped the model, `transformers` has it.

Host-side mirror of `transformers.LayoutLMModel` and its three inference heads (modeling_layoutlm.py v5.15:
`LayoutLMEmbeddings.forward` :66-119, `LayoutLMModel.forward` :433-524, `LayoutLMForSequenceClassification` :649,
`LayoutLMForTokenClassification` :777, `LayoutLMForQuestionAnswering` :879) with the state-dict key layout of those classes, so a
real checkpoint's tensors load by name.  The layers are BERT layers, shared with the other encoders through `bert_ops.BertOps`.
What is new here is the embedding stage (`vk_layoutlm_embed`), the word vote (`vk_token_word_labels`) and the span decode
(`vk_span_select`), all in csrc/layoutlm.hip.  All arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No
CPU fallback.

Out of scope: training and losses, `LayoutLMForMaskedLM`, `inputs_embeds`, custom `position_ids`, `output_attentions` /
`output_hidden_states`, and tokenisation (callers pass ids and `tokenmap`, as the reference's processors produce them).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, BertOps, Model, additive_mask, bert_layer_spec, check_text_inputs, host_array, keep_head, require_gelu, \
    seeded_tensor, to_numpy
from .layers import stream

DEFAULT_CONFIG = dict(vocab_size=30522, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                      max_position_embeddings=512, max_2d_position_embeddings=1024, type_vocab_size=2, layer_norm_eps=LN_EPS,
                      hidden_act="gelu")
TABLES = ("word_embeddings", "position_embeddings", "x_position_embeddings", "y_position_embeddings", "h_position_embeddings",
          "w_position_embeddings", "token_type_embeddings")
MAX_LABELS = 64                          # vk_token_word_labels: labels per token (TWL_MAX_C)
MAX_TOKENS = 4096                        # the two tails: tokens per example (TWL_MAX_L, SPN_MAX_L)
BBOX_RANGE = "The `bbox`coordinate values should be within 0-1000 range."      # transformers' wording (:100)


def layoutlm_config(**kw):
    """transformers' `LayoutLMConfig` defaults."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(kw)
    require_gelu(cfg)
    assert cfg["hidden_size"] % cfg["num_attention_heads"] == 0
    return cfg


def layoutlm_param_spec(cfg):
    """(name, shape) of every tensor of `transformers.LayoutLMModel(config).state_dict()`, in its order."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    rows = dict(word_embeddings=cfg["vocab_size"], position_embeddings=cfg["max_position_embeddings"],
                token_type_embeddings=cfg["type_vocab_size"])
    spec = [(f"embeddings.{t}.weight", (rows.get(t, cfg["max_2d_position_embeddings"]), H)) for t in TABLES]
    spec += [("embeddings.LayerNorm.weight", (H,)), ("embeddings.LayerNorm.bias", (H,))]
    for i in range(cfg["num_hidden_layers"]):
        spec += bert_layer_spec(f"encoder.layer.{i}", H, I)
    spec += [("pooler.dense.weight", (H, H)), ("pooler.dense.bias", (H,))]
    return spec


def layoutlm_head_param_spec(cfg, head, num_labels):
    """`state_dict()` of a head class: the model under `layoutlm.` + one nn.Linear, `classifier` (token and sequence
    classification) or `qa_outputs` (question answering, two labels)."""
    return [("layoutlm." + k, s) for k, s in layoutlm_param_spec(cfg)] + [
        (head + ".weight", (num_labels, cfg["hidden_size"])), (head + ".bias", (num_labels,))]


def make_layoutlm_state_dict(cfg, seed=0):
    """Seeded synthetic weights, drawn as `make_lxmert_state_dict` draws them: N(0, 0.05) matrices, tables and biases,
    LayerNorm gamma ~ U(0.5, 1.5)."""
    return {name: seeded_tensor(name, shape, seed) for name, shape in layoutlm_param_spec(cfg)}


def make_layoutlm_head_state_dict(cfg, head, num_labels, seed=0):
    sd = {"layoutlm." + k: v for k, v in make_layoutlm_state_dict(cfg, seed).items()}
    for name, shape in layoutlm_head_param_spec(cfg, head, num_labels)[-2:]:
        sd[name] = seeded_tensor(name, shape, seed)
    return sd


def check_bbox(bbox, B, Lt, max_2d):
    """`bbox [B, L, 4]` (x0, y0, x1, y1): integer, every coordinate in [0, max_2d), x1 >= x0 and y1 >= y0.  Host-side (a device
    tensor is read back), so it runs before a launch or a graph capture, never inside one.  transformers raises this IndexError
    for a coordinate past its table; a negative extent would index the h / w table from its end there, which is refused here."""
    if bbox is None:
        return
    b = host_array(bbox)
    if b.shape != (B, Lt, 4) or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"bbox must be an integer [B={B}, L={Lt}, 4] array, got {b.dtype} {b.shape}")
    if b.min() < 0 or b.max() >= max_2d:
        raise IndexError(f"{BBOX_RANGE} Found {int(b.min())}..{int(b.max())}; the tables have {max_2d} rows.")
    if (b[..., 2] < b[..., 0]).any() or (b[..., 3] < b[..., 1]).any():
        raise IndexError(f"{BBOX_RANGE} Found a box with x1 < x0 or y1 < y0.")


def ocr_token_boxes(word_boxes_xywh, tokenmap, raw_wh, max_len, add_cls=False):
    """The reference's `XYWHtoXYXY` + `OCRBoxFixed` (vltk/processing/visn.py) for one page, restated:
    -> (bbox int64 [max_len, 4], word_ids int32 [max_len]).

    Each word box (x, y, w, h) in raw pixels becomes (x, y, x + w, y + h); x is multiplied by 1000 / raw_w and y by 1000 / raw_h
    in float32, clamped to [0, 1000] and floored.  Word i's box is repeated `tokenmap[i]` times; the sequence is cut at `max_len`
    (a word the limit cuts keeps its leading tokens) and padded with [0, 0, 0, 0] / word id -1.  `add_cls` (the reference's
    `add_visual_cls`) prepends the whole page, [0, 0, 1000, 1000], with word id -1."""
    boxes = np.asarray(word_boxes_xywh, np.float32).reshape(-1, 4)
    counts = np.asarray(tokenmap, np.int64).reshape(-1)
    if len(counts) != len(boxes) or (counts < 0).any():
        raise ValueError(f"tokenmap must hold one non-negative token count per word box: {len(counts)} counts, {len(boxes)} boxes")
    raw_w, raw_h = (np.float32(v) for v in raw_wh)
    if not (raw_w > 0 and raw_h > 0) or max_len < 1:
        raise ValueError(f"raw size {tuple(raw_wh)} and max_len {max_len} must be positive")
    xyxy = boxes.copy()
    xyxy[:, 2:] += boxes[:, :2]
    xyxy *= np.asarray([np.float32(1000) / raw_w, np.float32(1000) / raw_h] * 2, np.float32)
    words = np.floor(np.clip(xyxy, 0, 1000)).astype(np.int64)
    ids = np.repeat(np.arange(len(words), dtype=np.int32), counts)
    tok = words[ids]
    if add_cls:
        tok = np.concatenate((np.asarray([[0, 0, 1000, 1000]], np.int64), tok))
        ids = np.concatenate((np.asarray([-1], np.int32), ids))
    n = min(len(ids), max_len)
    bbox, word_ids = np.zeros((max_len, 4), np.int64), np.full((max_len,), -1, np.int32)
    bbox[:n], word_ids[:n] = tok[:n], ids[:n]
    return bbox, word_ids


class LayoutLMModel(BertOps):
    """`transformers.LayoutLMModel` on the HIP path: `model(input_ids, bbox=None, attention_mask=None, token_type_ids=None)` ->
    (sequence_output [B, L, H], pooled_output [B, H]).  Defaults are transformers': bbox all zeros, the mask all ones, token
    types 0."""

    _INPUTS = ("input_ids", "bbox", "attention_mask", "token_type_ids")

    def __init__(self, config, precision="bf16", device="cuda:0"):
        super().__init__(layoutlm_config(**config), precision, device)

    def load_state_dict(self, sd, strict=True):
        sd = to_numpy(sd)
        self._check_state_dict(sd, dict(layoutlm_param_spec(self.cfg)), strict)
        for t in TABLES:
            self._load_tab(sd, t)
        self._load_ln(sd, "embeddings.LayerNorm")
        for i in range(self.cfg["num_hidden_layers"]):
            self._load_bert_layer(sd, f"encoder.layer.{i}")
        self._load_lin(sd, "pooler.dense", "pooler.dense")
        self._loaded = True
        return self

    # ---- host-side checks: everything that needs the VALUES of an input, before any launch or capture ----------------
    def _check(self, input_ids, bbox, attention_mask, token_type_ids):
        cfg = self.cfg
        if input_ids.dim() != 2 or 0 in input_ids.shape:
            raise ValueError(f"input_ids [B, L] with B, L >= 1 expected, got {tuple(input_ids.shape)}")
        check_text_inputs(input_ids, token_type_ids, cfg)
        B, Lt = input_ids.shape
        check_bbox(bbox, B, Lt, cfg["max_2d_position_embeddings"])
        if attention_mask is not None and tuple(attention_mask.shape) != (B, Lt):
            raise ValueError(f"attention_mask must be {(B, Lt)}, got {tuple(attention_mask.shape)}")

    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        return self._run(self._forward, (input_ids, bbox, attention_mask, token_type_ids))

    def capture(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        """Capture one forward for these input SHAPES into a HIP graph.  Returns `replay(...)` with the model's signature, which
        checks the new inputs on the host, copies them into the captured buffers, launches the graph and returns the (static)
        output tensors.  An input given as None at capture stays at its default."""
        run = self._capture_inputs((input_ids, bbox, attention_mask, token_type_ids))

        def replay(input_ids, bbox=None, attention_mask=None, token_type_ids=None):
            return run((input_ids, bbox, attention_mask, token_type_ids))
        return replay

    def embeddings(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        """The embedding stage alone: what transformers' `model.embeddings` returns, [B, L, H]."""
        x, _ = self._run(self._embed, (input_ids, bbox, attention_mask, token_type_ids))
        return x.view(input_ids.shape[0], -1, self.cfg["hidden_size"])

    @torch.no_grad()
    def _embed(self, input_ids, bbox, attention_mask, token_type_ids):
        """-> (LayerNormed embeddings [B * L, H], additive mask [B, L] or None)."""
        self._require_loaded()
        cfg, dev, tab = self.cfg, self.device, self._tab
        B, Lt = input_ids.shape
        H = cfg["hidden_size"]
        ids = input_ids.to(dev, torch.int64).contiguous()
        tts = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous()
        # LayoutLMModel.forward :498: no boxes are boxes of zeros
        box = torch.zeros((B, Lt, 4), dtype=torch.int32, device=dev) if bbox is None else bbox.to(dev, torch.int32).contiguous()
        mask = additive_mask(attention_mask, dev)
        x = torch.empty((B * Lt, H), dtype=self.tdt, device=dev)
        g, b = self._ln["embeddings.LayerNorm"]
        L.call("vk_layoutlm_embed", ids.data_ptr(), tts.data_ptr(), box.data_ptr(), B, Lt, tab["word_embeddings"].data_ptr(),
               cfg["vocab_size"], tab["position_embeddings"].data_ptr(), cfg["max_position_embeddings"],
               tab["x_position_embeddings"].data_ptr(), tab["y_position_embeddings"].data_ptr(), tab["h_position_embeddings"].data_ptr(),
               tab["w_position_embeddings"].data_ptr(), cfg["max_2d_position_embeddings"], tab["token_type_embeddings"].data_ptr(),
               cfg["type_vocab_size"], g.data_ptr(), b.data_ptr(), x.data_ptr(), H, cfg["layer_norm_eps"], self.dt, stream(dev))
        return x, mask

    def _encode(self, *inputs):
        """-> the last layer's rows [B * L, H]."""
        x, mask = self._embed(*inputs)
        B, Lt = inputs[0].shape
        for i in range(self.cfg["num_hidden_layers"]):   # LayoutLMEncoder: plain BERT layers
            x = self._bert_layer(f"encoder.layer.{i}", x, mask, B, Lt)
        return x

    def _forward(self, *inputs):
        x = self._encode(*inputs)
        B, Lt = inputs[0].shape
        return x.view(B, Lt, self.cfg["hidden_size"]), self._pooler(x, B, Lt)


class _Head(Model):
    """What the three heads share: the whole model under the `layoutlm.` prefix and one nn.Linear on top of it."""

    _HEAD = "classifier"

    def __init__(self, config, num_labels, precision="bf16", device="cuda:0"):
        self.layoutlm = LayoutLMModel(config, precision, device)
        self.num_labels = int(num_labels)

    def load_state_dict(self, sd, strict=True):
        enc = self.layoutlm
        sd = self._load_with_encoder(enc, "layoutlm.", layoutlm_head_param_spec(enc.cfg, self._HEAD, self.num_labels), sd, strict)
        enc._load_lin(sd, self._HEAD, self._HEAD)
        keep_head(enc, sd, self._HEAD)
        return self


def _strided_rows(t, what):
    """(element stride between the rows of a [B, L(, C)] tensor whose rows lie evenly spaced in memory)."""
    if t.stride(0) != t.shape[1] * t.stride(1) or (t.dim() == 3 and t.stride(2) != 1):
        raise ValueError(f"{what}: rows must be evenly spaced in memory (strides {t.stride()} for shape {tuple(t.shape)})")
    return t.stride(1)


class LayoutLMForTokenClassification(_Head):
    """`transformers.LayoutLMForTokenClassification`: `classifier` over every token in one GEMM.  `model(...)` takes the
    encoder's arguments and returns logits [B, L, num_labels] in the storage type (a view of the GEMM's padded output)."""

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        enc = self.layoutlm
        logits = enc._run(lambda *inputs: enc._linear(enc._encode(*inputs), "classifier"), (input_ids, bbox, attention_mask, token_type_ids))
        return logits.view(input_ids.shape[0], input_ids.shape[1], self.num_labels)

    @torch.no_grad()
    def word_labels(self, logits, word_ids, num_words):
        """The reference's `map_ocr_predictions` on the device (`vk_token_word_labels`): logits [B, L, C <= 64], word_ids [B, L]
        (the word of each token, -1 for special and padding tokens; `ocr_token_boxes` returns them) -> (token_labels [B, L],
        word_labels [B, num_words]) int32.  A token's label is the first arg-max; a word's label is the most frequent label of
        its tokens, the smallest on a tie, -1 for a word with no token."""
        enc = self.layoutlm
        if logits.dim() != 3 or logits.dtype != enc.tdt:
            raise ValueError(f"logits [B, L, C] in {enc.tdt} expected, got {logits.dtype} {tuple(logits.shape)}")
        B, Lt, Cn = logits.shape
        if tuple(word_ids.shape) != (B, Lt):
            raise ValueError(f"word_ids must be {(B, Lt)}, got {tuple(word_ids.shape)}")
        if not (1 <= Cn <= MAX_LABELS and 1 <= Lt <= MAX_TOKENS and 1 <= num_words <= Lt):
            raise ValueError(f"word_labels takes 1..{MAX_LABELS} labels, 1..{MAX_TOKENS} tokens and 1..L words: got C={Cn} L={Lt} W={num_words}")
        logits = logits.to(enc.device)
        ld = _strided_rows(logits, "logits")
        wid = word_ids.to(enc.device, torch.int32).contiguous()
        tok = torch.empty((B, Lt), dtype=torch.int32, device=enc.device)
        words = torch.empty((B, num_words), dtype=torch.int32, device=enc.device)
        L.call("vk_token_word_labels", logits.data_ptr(), ld, wid.data_ptr(), B, Lt, Cn, num_words, tok.data_ptr(), words.data_ptr(),
               enc.dt, stream(enc.device))
        torch.cuda.synchronize(enc.device)
        return tok, words


class LayoutLMForQuestionAnswering(_Head):
    """`transformers.LayoutLMForQuestionAnswering`: `qa_outputs` (two columns) as one GEMM.  `model(...)` returns
    (start_logits, end_logits), each [B, L] in the storage type: the two columns of the GEMM's output, not copied."""

    _HEAD = "qa_outputs"

    def __init__(self, config, precision="bf16", device="cuda:0"):
        super().__init__(config, 2, precision, device)

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        enc = self.layoutlm                                           # logits [B * L, 2], rows as far apart as the GEMM pads them
        logits = enc._run(lambda *inputs: enc._linear(enc._encode(*inputs), "qa_outputs"), (input_ids, bbox, attention_mask, token_type_ids))
        B, Lt = input_ids.shape
        return logits[:, 0].view(B, Lt), logits[:, 1].view(B, Lt)

    @torch.no_grad()
    def best_span(self, start_logits, end_logits, context_mask, max_answer_tokens=30):
        """`vk_span_select`: the best pair s <= e of context tokens with e - s + 1 <= max_answer_tokens under
        start_logits[s] + end_logits[e] -> (start [B], end [B]) int32, score [B] fp32; (-1, -1, -inf) where there is none.  Ties
        go to the smaller s, then the smaller e.  The logits are read where they are (the columns `model(...)` returned)."""
        enc = self.layoutlm
        for t in (start_logits, end_logits):
            if t.dim() != 2 or t.dtype != enc.tdt or t.shape != start_logits.shape:
                raise ValueError(f"start_logits and end_logits [B, L] in {enc.tdt} expected, got {t.dtype} {tuple(t.shape)}")
        B, Lt = start_logits.shape
        if tuple(context_mask.shape) != (B, Lt):
            raise ValueError(f"context_mask must be {(B, Lt)}, got {tuple(context_mask.shape)}")
        if not (1 <= Lt <= MAX_TOKENS) or max_answer_tokens < 1:
            raise ValueError(f"best_span takes 1..{MAX_TOKENS} tokens and max_answer_tokens >= 1: got L={Lt}, {max_answer_tokens}")
        s_log, e_log = start_logits.to(enc.device), end_logits.to(enc.device)
        ctx = (context_mask.to(enc.device) != 0).to(torch.int32).contiguous()
        start = torch.empty((B,), dtype=torch.int32, device=enc.device)
        end = torch.empty((B,), dtype=torch.int32, device=enc.device)
        score = torch.empty((B,), dtype=torch.float32, device=enc.device)
        L.call("vk_span_select", s_log.data_ptr(), _strided_rows(s_log, "start_logits"), e_log.data_ptr(),
               _strided_rows(e_log, "end_logits"), ctx.data_ptr(), B, Lt, int(min(max_answer_tokens, Lt)), start.data_ptr(),
               end.data_ptr(), score.data_ptr(), enc.dt, stream(enc.device))
        torch.cuda.synchronize(enc.device)
        return start, end, score


class LayoutLMForSequenceClassification(_Head):
    """`transformers.LayoutLMForSequenceClassification`: `classifier` on the pooled output -> logits [B, num_labels]."""

    def _head_features(self, *inputs):
        return self.layoutlm._forward(*inputs)[1]

    @torch.no_grad()
    def head_features(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        """What `classifier` consumes: the pooled output [B, H], storage type (`HeadTrainer.step_features` takes it)."""
        return self.layoutlm._run(self._head_features, (input_ids, bbox, attention_mask, token_type_ids))

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None):
        enc = self.layoutlm
        return enc._run(lambda *inputs: enc._linear(self._head_features(*inputs), "classifier"), (input_ids, bbox, attention_mask, token_type_ids))
