"""The single-stream vision-language encoder the reference's training script builds: `VisualBertForQuestionAnswering`
(`vltk/legacy/legacy_train.py:8, 156-160`), fed with the extractor's `roi_features [B, 36, 2048]` as `visual_embeds`.

Host-side mirror of `transformers.VisualBertModel` / `VisualBertForQuestionAnswering` (modeling_visual_bert.py v5.15:
`VisualBertEmbeddings.forward` :72-168, `VisualBertModel.forward` :599-662, `VisualBertForQuestionAnswering.forward` :1106-1132)
with the state-dict key layout of those classes, so a real checkpoint's tensors load by name.  Text and boxes form ONE
sequence (text first); the layers are BERT layers, shared with `LxmertEncoder` through `bert_ops.BertOps`.  What is new here is
the embedding stage (`vk_visualbert_embed`, csrc/visualbert.hip) and the gather head.  All arithmetic runs in `libvltk_hip.so`;
torch only owns the device buffers.  No CPU fallback.

Out of scope: training and the pre-training heads, `inputs_embeds`, custom `position_ids`, `output_attentions` /
`output_hidden_states`, `bypass_transformer`.
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, BertOps, Model, additive_mask, bert_layer_spec, check_ids, check_text_inputs, host_array, keep_head, require_gelu, \
    seeded_tensor, to_numpy
from .layers import stream

DEFAULT_CONFIG = dict(vocab_size=30522, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                      max_position_embeddings=512, type_vocab_size=2, visual_embedding_dim=512, layer_norm_eps=LN_EPS,
                      hidden_act="gelu", bypass_transformer=False)
MAX_ALIGNMENT = 16                       # alignment entries per box the embedding kernel takes (VBE_MAX_ALIGN)


def visualbert_config(**kw):
    """transformers' `VisualBertConfig` defaults; callers set `visual_embedding_dim=2048` for this extractor's features."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(kw)
    if cfg["bypass_transformer"]:
        raise NotImplementedError("VisualBERT with bypass_transformer=True (the extra layer over [text encoder | raw visual rows]) is not built")
    require_gelu(cfg)
    assert cfg["hidden_size"] % cfg["num_attention_heads"] == 0
    return cfg


def visualbert_param_spec(cfg):
    """(name, shape) of every tensor of `transformers.VisualBertModel(config).state_dict()`, in its order."""
    H, I, P, T = cfg["hidden_size"], cfg["intermediate_size"], cfg["max_position_embeddings"], cfg["type_vocab_size"]
    spec = [("embeddings.word_embeddings.weight", (cfg["vocab_size"], H)), ("embeddings.position_embeddings.weight", (P, H)),
            ("embeddings.token_type_embeddings.weight", (T, H)),
            ("embeddings.LayerNorm.weight", (H,)), ("embeddings.LayerNorm.bias", (H,)),
            ("embeddings.visual_token_type_embeddings.weight", (T, H)), ("embeddings.visual_position_embeddings.weight", (P, H)),
            ("embeddings.visual_projection.weight", (H, cfg["visual_embedding_dim"])), ("embeddings.visual_projection.bias", (H,))]
    for i in range(cfg["num_hidden_layers"]):
        spec += bert_layer_spec(f"encoder.layer.{i}", H, I)
    spec += [("pooler.dense.weight", (H, H)), ("pooler.dense.bias", (H,))]
    return spec


def visualbert_qa_param_spec(cfg, num_labels):
    """`transformers.VisualBertForQuestionAnswering(config).state_dict()`: the model under `visual_bert.` + `cls`."""
    return [("visual_bert." + k, s) for k, s in visualbert_param_spec(cfg)] + [
        ("cls.weight", (num_labels, cfg["hidden_size"])), ("cls.bias", (num_labels,))]


def make_visualbert_state_dict(cfg, seed=0):
    """Seeded synthetic weights, drawn as `make_lxmert_state_dict` draws them: N(0, 0.05) matrices, tables and biases,
    LayerNorm gamma ~ U(0.5, 1.5)."""
    return {name: seeded_tensor(name, shape, seed) for name, shape in visualbert_param_spec(cfg)}


def make_visualbert_qa_state_dict(cfg, num_labels, seed=0):
    sd = {"visual_bert." + k: v for k, v in make_visualbert_state_dict(cfg, seed).items()}
    for name, shape in visualbert_qa_param_spec(cfg, num_labels)[-2:]:
        sd[name] = seeded_tensor(name, shape, seed)
    return sd


def check_alignment(image_text_alignment, B, V, max_position):
    """`image_text_alignment [B, V, A]`: integer, A <= 16, entries in [-1, max_position).  Host-side (a device tensor is read
    back), so it runs before a launch or a graph capture, never inside one."""
    a = host_array(image_text_alignment)
    if a.ndim != 3 or a.shape[:2] != (B, V) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"image_text_alignment must be an integer [B={B}, V={V}, A] array, got {a.dtype} {a.shape}")
    if not 1 <= a.shape[2] <= MAX_ALIGNMENT:
        raise ValueError(f"image_text_alignment has {a.shape[2]} entries per box: 1..{MAX_ALIGNMENT} are supported")
    if a.min() < -1 or a.max() >= max_position:
        raise IndexError(f"image_text_alignment entries must lie in [-1, {max_position}) (-1 pads): found {int(a.min())}..{int(a.max())}")


def qa_gather_index(attention_mask, B, Lt, V):
    """Row of `sequence_output.view(B * (Lt + V), H)` the answer head reads per example: `b * (Lt + V) + (attention_mask.sum(1) - 2)`
    of the TEXT mask (VisualBertForQuestionAnswering.forward :1106, "as in original code"); None counts as all ones.  Host-side.
    An index outside [0, Lt + V) raises IndexError."""
    if attention_mask is None:
        idx = np.full((B,), Lt - 2, np.int64)
    else:
        m = host_array(attention_mask)
        if m.shape != (B, Lt):
            raise ValueError(f"attention_mask must be [B={B}, Lt={Lt}], got {m.shape}")
        idx = m.sum(1).astype(np.int64) - 2
    if idx.min() < 0 or idx.max() >= Lt + V:
        raise IndexError(f"VisualBertForQuestionAnswering gathers token attention_mask.sum(1) - 2 = {idx.tolist()}: outside [0, {Lt + V})")
    return (np.arange(B, dtype=np.int64) * (Lt + V) + idx).astype(np.int32)


class VisualBertModel(BertOps):
    """`transformers.VisualBertModel` on the HIP path: `model(input_ids, visual_embeds, attention_mask=None,
    visual_attention_mask=None, token_type_ids=None, visual_token_type_ids=None, image_text_alignment=None)` ->
    (sequence_output [B, Lt + V, H] with the text tokens first, pooled_output [B, H]).  Defaults are transformers': masks all
    ones, token types 0 for text and 1 for boxes, visual position id 0."""

    _INPUTS = ("input_ids", "visual_embeds", "attention_mask", "visual_attention_mask", "token_type_ids", "visual_token_type_ids",
               "image_text_alignment")

    def __init__(self, config, precision="bf16", device="cuda:0"):
        super().__init__(visualbert_config(**config), precision, device)

    def load_state_dict(self, sd, strict=True):
        sd = to_numpy(sd)
        self._check_state_dict(sd, dict(visualbert_param_spec(self.cfg)), strict)
        for t in ("word_embeddings", "position_embeddings", "token_type_embeddings", "visual_token_type_embeddings",
                  "visual_position_embeddings"):
            self._load_tab(sd, t)
        self._load_ln(sd, "embeddings.LayerNorm")
        self._load_lin(sd, "embeddings.visual_projection", "embeddings.visual_projection")
        for i in range(self.cfg["num_hidden_layers"]):
            self._load_bert_layer(sd, f"encoder.layer.{i}")
        self._load_lin(sd, "pooler.dense", "pooler.dense")
        self._loaded = True
        return self

    # ---- host-side checks: everything that needs the VALUES of an input, before any launch or capture ----------------
    def _check(self, input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids,
               image_text_alignment):
        cfg = self.cfg
        if input_ids.dim() != 2 or visual_embeds.dim() != 3 or visual_embeds.shape[0] != input_ids.shape[0]:
            raise ValueError(f"input_ids [B, Lt] and visual_embeds [B, V, D] expected, got {tuple(input_ids.shape)} {tuple(visual_embeds.shape)}")
        B, Lt = input_ids.shape
        V = visual_embeds.shape[1]
        if visual_embeds.shape[2] != cfg["visual_embedding_dim"]:
            raise ValueError(f"visual_embeds are {visual_embeds.shape[2]} wide, config.visual_embedding_dim is {cfg['visual_embedding_dim']}")
        check_text_inputs(input_ids, token_type_ids, cfg)
        check_ids("visual_token_type_ids", visual_token_type_ids, (B, V), cfg["type_vocab_size"])
        for name, t, shape in (("attention_mask", attention_mask, (B, Lt)), ("visual_attention_mask", visual_attention_mask, (B, V))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
        if image_text_alignment is not None:
            check_alignment(image_text_alignment, B, V, cfg["max_position_embeddings"])

    def __call__(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                 visual_token_type_ids=None, image_text_alignment=None):
        return self._run(self._forward, (input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids,
                                         visual_token_type_ids, image_text_alignment))

    def capture(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                visual_token_type_ids=None, image_text_alignment=None):
        """Capture one forward for these input SHAPES into a HIP graph (about 90 dependent small launches become one graph
        launch).  Returns `replay(...)` with the model's signature, which checks the new inputs on the host, copies them into the
        captured buffers, launches the graph and returns the (static) output tensors.  An input given as None at capture stays
        at its default."""
        run = self._capture_inputs((input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids,
                                    image_text_alignment))

        def replay(input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                   visual_token_type_ids=None, image_text_alignment=None):
            return run((input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids,
                        image_text_alignment))
        return replay

    def embeddings(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                   visual_token_type_ids=None, image_text_alignment=None):
        """The embedding stage alone: what transformers returns as `hidden_states[0]`, [B, Lt + V, H]."""
        x, _ = self._run(self._embed, (input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids,
                                       visual_token_type_ids, image_text_alignment))
        return x.view(input_ids.shape[0], -1, self.cfg["hidden_size"])

    @torch.no_grad()
    def _embed(self, input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids,
               image_text_alignment):
        """-> (LayerNormed embeddings [B * (Lt + V), H], additive mask [B, Lt + V])."""
        self._require_loaded()
        cfg, dev, tab = self.cfg, self.device, self._tab
        B, Lt = input_ids.shape
        V = visual_embeds.shape[1]
        H = cfg["hidden_size"]
        ids = input_ids.to(dev, torch.int64).contiguous()
        tts = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous()
        vtts = (torch.ones((B, V), dtype=torch.int64, device=dev) if visual_token_type_ids is None
                else visual_token_type_ids.to(dev, torch.int64).contiguous())
        align = None if image_text_alignment is None else image_text_alignment.to(dev, torch.int32).contiguous()
        # VisualBertModel.forward :605-613: the combined mask is [text mask | visual mask], ones where none is given
        am = torch.ones((B, Lt), device=dev) if attention_mask is None else attention_mask.to(dev, torch.float32)
        vm = torch.ones((B, V), device=dev) if visual_attention_mask is None else visual_attention_mask.to(dev, torch.float32)
        mask = additive_mask(torch.cat((am, vm), dim=1), dev)
        # VisualBertEmbeddings.forward :72-168: visual_projection on the GEMM, then one launch for both kinds of row
        vf = visual_embeds.to(dev).reshape(B * V, -1).to(self.tdt).contiguous()
        proj = self._linear(vf, "embeddings.visual_projection")
        x = torch.empty((B * (Lt + V), H), dtype=self.tdt, device=dev)
        g, b = self._ln["embeddings.LayerNorm"]
        L.call("vk_visualbert_embed", ids.data_ptr(), tts.data_ptr(), vtts.data_ptr(), None if align is None else align.data_ptr(),
               0 if align is None else align.shape[2], B, Lt, V, tab["word_embeddings"].data_ptr(), cfg["vocab_size"],
               tab["position_embeddings"].data_ptr(), cfg["max_position_embeddings"], tab["token_type_embeddings"].data_ptr(),
               tab["visual_token_type_embeddings"].data_ptr(), cfg["type_vocab_size"], tab["visual_position_embeddings"].data_ptr(),
               proj.data_ptr(), proj.stride(0), g.data_ptr(), b.data_ptr(), x.data_ptr(), H, cfg["layer_norm_eps"], self.dt, stream(dev))
        return x, mask

    def _forward(self, *inputs):
        x, mask = self._embed(*inputs)
        B, Lx, H = inputs[0].shape[0], inputs[0].shape[1] + inputs[1].shape[1], self.cfg["hidden_size"]
        for i in range(self.cfg["num_hidden_layers"]):   # VisualBertEncoder: plain BERT layers over the joint sequence
            x = self._bert_layer(f"encoder.layer.{i}", x, mask, B, Lx)
        return x.view(B, Lx, H), self._pooler(x, B, Lx)


class VisualBertForQuestionAnswering(Model):
    """`transformers.VisualBertForQuestionAnswering` (modeling_visual_bert.py :1106-1132, the model `legacy_train.py` builds) on
    the HIP path: the encoder, then `cls` on the row `attention_mask.sum(1) - 2` of each example's sequence output (the last
    text token before [SEP]; the TEXT mask counts).  `model(...)` takes the encoder's arguments and returns logits
    `[B, num_labels]` in the storage type.

    `attention_mask=None` counts as all ones (row `Lt - 2`); transformers itself fails on None there (`None.sum`).  A row
    outside `[0, Lt + V)` -- a text mask summing to less than 2 -- raises IndexError before anything is launched."""

    def __init__(self, config, num_labels, precision="bf16", device="cuda:0"):
        self.visual_bert = VisualBertModel(config, precision, device)
        self.num_labels = int(num_labels)

    def load_state_dict(self, sd, strict=True):
        enc = self.visual_bert
        sd = self._load_with_encoder(enc, "visual_bert.", visualbert_qa_param_spec(enc.cfg, self.num_labels), sd, strict)
        enc._load_lin(sd, "cls", "cls")
        keep_head(enc, sd, "cls")
        return self

    def _head_features(self, *inputs):
        enc = self.visual_bert
        input_ids, visual_embeds, attention_mask = inputs[:3]
        B, Lt = input_ids.shape
        idx = torch.from_numpy(qa_gather_index(attention_mask, B, Lt, visual_embeds.shape[1])).to(enc.device)    # host, before any launch
        seq, _ = enc._forward(*inputs)
        return enc._gather_rows(seq.view(-1, enc.cfg["hidden_size"]), idx)

    def head_features(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                      visual_token_type_ids=None, image_text_alignment=None):
        """What `cls` consumes: row `attention_mask.sum(1) - 2` of each sequence [B, H], storage type (`HeadTrainer.step_features`
        takes it; the dropout transformers puts before `cls` in training mode is not applied)."""
        return self.visual_bert._run(self._head_features, (input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids,
                                                          visual_token_type_ids, image_text_alignment))

    @torch.no_grad()
    def __call__(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                 visual_token_type_ids=None, image_text_alignment=None):
        enc = self.visual_bert

        def forward(*inputs):
            return enc._linear(self._head_features(*inputs), "cls")
        return enc._run(forward, (input_ids, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids,
                                  image_text_alignment))
