"""N8: fine-tune the top encoder layers and the answer head.  The reference's training script (`vltk/legacy/legacy_train.py`)
trains the whole `VisualBertForQuestionAnswering`; its framework step (`vltk/abc/simple.py:665-682`) is `loss.backward();
clip_grad_norm_(params, config.train.max_norm); optim.step(); scheduler.step()` with `max_norm = 5.0` (`configs.py:88`), and
`freeze_layers` (`vltk/abc/complex.py:109-120`) freezes a prefix of the layers and trains the rest: the recipe on extracted
features.  `EncoderTrainer` is that recipe: the first `L - n` layers run the encoder's own forward in its own precision, the last
`n` layers and the head run in fp32 with every activation the backward needs kept, and are walked backwards.

Forward, loss, backward, clipping and the optimiser step are kernels of csrc/train.hip, csrc/attention_grad.hip and
csrc/index_add.hip (`vk_gemm_f32`, `vk_attention` in fp32, `vk_attention_grad`, `vk_layernorm`, `vk_layernorm_grad`, `vk_act_f32`, `vk_act_grad_f32`,
`vk_col_sums`, `vk_add_f32` for the residuals, `vk_scatter_rows_f32`, `vk_embed_sum_f32`, `vk_index_add_rows`, `vk_cross_entropy(_grad)`, `vk_grad_clip`, `vk_adamw_step`)
through the op wrappers of train.py.  All arithmetic runs in `libvltk_hip.so`; torch owns the device buffers and makes the one
cast there is, at the boundary: the frozen layers' 16-bit hidden state to fp32, which is exact.  No CPU fallback.

`attention.self.key.bias`: soft-max is invariant to a shift of a whole score row, so this tensor's gradient is mathematically zero
and what the kernels (and torch) compute for it is rounding noise below AdamW's eps.  It is trained as torch trains it; only weight
decay moves it in earnest.

`compute_dtype=torch.bfloat16` is the mixed-precision mode, what `torch.autocast` gives: fp32 masters,
gradients and optimiser; bf16 operands on the matrix cores for every layer GEMM (`vk_gemm_16` after `vk_cast_16`) and for attention
(`vk_attention_tiled` forward, `vk_attention_grad_16` backward, csrc/gemm16.hip and csrc/attention_grad16.hip); fp32 accumulation,
LayerNorm, GELU, column sums, residual adds, head and loss, on the kernels of the fp32 mode.  The default, `None`, is the fp32
trainer with every launch and every bit as before.

Both modes walk ONE layer forward and ONE layer backward (`_layer_forward`, `_layer_backward`) under train.py's `Precision`, which
answers what they differ on: `operand(t)` (t itself in fp32, so that mode issues no cast; one `vk_cast_16` at the point of first
use in the mixed mode), the GEMM entry, and whether a product is written in 16 bits (the QKV projection and `dctx`, which
attention reads).  The weight a product reads comes from `self._w`: the fp32 master, or its 16-bit copy that `_cast_weights`
refreshes at the start of a step.  The attention wrappers pick their entry from the dtype of what they are given.

`train_embeddings=True` is the reference script's own setting, every parameter to AdamW: with all layers trained, the tables, the
embedding LayerNorm and VisualBERT's `visual_projection` join the trained set.  The stage runs in fp32 in both modes (only the
projection, a Linear, follows `Precision`): index columns built with torch on the device, `vk_embed_sum_f32` per modality (the sum
in transformers' order of `+`), `vk_layernorm` with the sum kept; backwards `vk_layernorm_grad`, then one `vk_index_add_rows` per
table over the gradient of the sum (csrc/index_add.hip: a stable radix sort by table row and a segmented fp64 sum, no atomics, the
same bits on every run).  VisualBERT's text and visual rows are picked out of the joint sequence by the
kernel's `src_row`; LayoutLM's x table takes `left` and `right`, its y table `upper` and `lower`, as two index columns of one launch.

`hidden_dropout`, `attention_dropout` and `seed` give the step transformers' training-mode dropout, at the
sites transformers has it: the embedding stage's output (under `train_embeddings`), per trained layer the attention probabilities
and the outputs of `attention.output.dense` and `output.dense` before their residuals, and the head's input rows.  A decision is
Philox4x32-10 of (seed, stream = steps * 2^16 + the site's number, granule, byte), regenerated in registers wherever it is needed:
no mask tensor exists.  A hidden site is `vk_dropout_add_f32` in place of the residual's `vk_add_f32`, and once more, without a
residual, on the gradient that enters the site's Linear; the attention site is `vk_attention_tiled_dropout` and
`vk_attention_grad_16_dropout` under one (rate, seed, stream), so it needs the mixed mode.  Both rates 0.0, the default, is the
trainer without the arguments, launch for launch.  The frozen layers run the model's own eval forward.

`LayoutLMv3ForSequenceClassification`: row 0 goes through `classifier.dense` + tanh to
`classifier.out_proj`, the pooled path under other keys; the attention pair of a trained layer is `vk_attention_relpos` /
`vk_attention_relpos_grad`, and the bias matrices that exist (`layoutlmv3.encoder.rel_pos_bias.weight`, `...rel_pos_x_bias.weight`,
`...rel_pos_y_bias.weight`), shared by all layers, are trained like any other tensor.  Each step builds the device table from their
fp32 masters by a gather through `relpos_bucket_map`; the frozen layers read the same tables, so they run with the trainer's table
(the model's own is written by `commit()` only); backwards, `vk_relpos_lut_grad` sums each trained layer's table gradient by bucket
into the matrices' gradients, the top layer writing and the others adding.  With neither bias flag the existing kernels run.
Refused (ValueError): `compute_dtype=None` with a bias term, `attention_dropout > 0`, `train_embeddings=True`.

Out of scope: the strict fp32 backward of the position-bias attention, attention dropout and embedding training for LayoutLMv3,
`LayoutLMv3ForTokenClassification`, dropout on the fp32 attention pair, HIP-graph capture of a step, `image_text_alignment` under `train_embeddings` (a weighted lookup), sparse
(row-wise) AdamW, 16-bit tables, ViT (pre-LN layers) and LXMERT (cross-attention top layers), running the top layer only on the rows the head reads (for `train_layers=1` the FFN is needed on B rows, not B * L:
measure first, then build it as its own change), fp16 as the compute type (its gradients need loss scaling) and producers that
write both precisions at once (the cast passes are measured first).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, additive_mask, bert_layer_spec, to_numpy
from .train import (Precision, _Trainer, act_f32, act_grad_f32, add_f32, attention, attention_grad, cast_16, check_scatter_index,
                    dropout_add_f32, dropout_rate, embed_sum_f32, gather_rows_f32, gemm_f32, grad_clip, index_add_rows, layernorm_f32,
                    layernorm_grad, linear_backward, loss_and_grad, scatter_rows_f32)


# ---- what is trained ---------------------------------------------------------------------------------------------------------------------
def _describe(model):
    """-> (encoder, its state-dict prefix, head prefix, the prefix of the dense + tanh on row 0 that stands between the layers and
    the head, or None)."""
    from .layoutlm import LayoutLMForSequenceClassification
    from .layoutlmv3 import LayoutLMv3ForSequenceClassification
    from .visualbert import VisualBertForQuestionAnswering
    if isinstance(model, VisualBertForQuestionAnswering):
        return model.visual_bert, "visual_bert.", "cls", None
    if isinstance(model, LayoutLMForSequenceClassification):
        return model.layoutlm, "layoutlm.", "classifier", "layoutlm.pooler.dense"
    if isinstance(model, LayoutLMv3ForSequenceClassification):
        return model.layoutlmv3, "layoutlmv3.", "classifier.out_proj", "classifier.dense"
    why = {"ViTForImageClassification": ": ViT's layers are pre-LN, the backward here is the post-LN BERT layer's",
           "LxmertForQuestionAnswering": ": LXMERT's top layers are cross-attention layers"}.get(type(model).__name__, "")
    raise TypeError("EncoderTrainer takes VisualBertForQuestionAnswering, LayoutLMForSequenceClassification or "
                    f"LayoutLMv3ForSequenceClassification, not {type(model).__name__}{why}")


def _check_compute_dtype(compute_dtype, cfg):
    """None (the fp32 trainer) or torch.bfloat16 where the encoder's sizes allow the 16-bit kernels; ValueError otherwise."""
    if compute_dtype is None:
        return None
    if compute_dtype == torch.float16:
        raise ValueError("compute_dtype=torch.float16: fp16 gradients underflow without loss scaling, which the trainer does not do; "
                         "use torch.bfloat16 (the kernels themselves take fp16)")
    if compute_dtype != torch.bfloat16:
        raise ValueError(f"compute_dtype must be None (fp32) or torch.bfloat16, not {compute_dtype}: the mixed mode's kernels take 16-bit operands")
    H, I, heads = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"]
    if H // heads not in (32, 64) or H % heads:
        raise ValueError(f"compute_dtype=torch.bfloat16: the head dim is {H // heads}, and the 16-bit attention kernels take 32 or 64 only")
    if H % 8 or I % 8:
        raise ValueError(f"compute_dtype=torch.bfloat16: hidden size {H} and intermediate size {I} must be multiples of 8 "
                         "(16-byte rows of 16-bit matrices)")
    return compute_dtype


# transformers' `pad_token_id` of `VisualBertConfig` and `LayoutLMConfig`, where the model's config dict names none: the word
# table's `padding_idx`
DEFAULT_PAD_TOKEN_ID = {"visual_bert.": 1, "layoutlm.": 0}


def _embedding_spec(enc_prefix, cfg):
    """(key, shape) of the embedding stage's tensors under transformers' names, in the state dict's order."""
    from .layoutlm import layoutlm_param_spec
    from .visualbert import visualbert_param_spec
    spec = (visualbert_param_spec if enc_prefix == "visual_bert." else layoutlm_param_spec)(cfg)
    return [(enc_prefix + k, shp) for k, shp in spec if k.startswith("embeddings.")]


# the weight matrices of a trained layer that the mixed mode keeps a 16-bit copy of (the packed [3H, H] QKV master beside them)
_LAYER_MATRICES = (".attention.output.dense.weight", ".intermediate.dense.weight", ".output.dense.weight")


class EncoderTrainer(_Trainer):
    """`EncoderTrainer(model, state_dict, train_layers=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(),
    schedule=None, max_grad_norm=None)`: trains the last `train_layers` BERT layers and the head of
    `VisualBertForQuestionAnswering` (layers -> the gathered row -> `cls`), `LayoutLMForSequenceClassification` (layers ->
    `pooler.dense` + tanh on the first token -> `classifier`; `pooler.dense` is trained too) or `LayoutLMv3ForSequenceClassification`
    (layers -> `classifier.dense` + tanh on row 0 -> `classifier.out_proj`, and the relative-position bias matrices; mixed mode only) with cross-entropy, optional clipping
    of the global gradient norm and `torch.optim.AdamW`'s rule.  The lower layers and the embeddings stay frozen.  Any other
    model: TypeError.

    `state_dict` is the checkpoint the model was loaded from (the model keeps only packed weights of its layers): the keys and
    shapes of the trained tensors must match, and its head tensors must be bit-equal to the model's (else ValueError).  The
    trainer holds fp32 masters, gradients and AdamW's `m`, `v` under transformers' key names.  `no_decay`, `schedule`: as
    `HeadTrainer`.  `train_layers=0` is `HeadTrainer`'s job.

    `compute_dtype=torch.bfloat16` runs the trained layers in mixed precision: each step casts the trained weight matrices to
    bf16 copies, every layer GEMM and attention, forward and backward, takes bf16 operands on the matrix cores and accumulates
    in fp32; masters, gradients, AdamW, clipping, LayerNorm, GELU, the head and the loss stay fp32.  It needs a head dim of 32 or
    64 and hidden / intermediate sizes that are multiples of 8; `torch.float16` and every other dtype are refused (ValueError).
    It is independent of the model's own precision.  `compute_dtype` (read-only) tells the mode; `None` is the fp32 trainer.

    `train_embeddings=True` (needs `train_layers == num_hidden_layers`, else ValueError) also trains the embedding stage:
    VisualBERT's word, position, token-type, visual token-type and visual position tables, `visual_projection` and
    `embeddings.LayerNorm`; LayoutLM's word, position, x, y, h, w and token-type tables and `embeddings.LayerNorm`, under
    transformers' key names, which `state_dict` must hold in their shapes.  The word table's `padding_idx` row takes no gradient
    (weight decay still moves it, as in torch): it is the config's `pad_token_id`, by default transformers' own, 1 for
    `VisualBertConfig` and 0 for `LayoutLMConfig`.  `image_text_alignment` in a step is then refused (ValueError).  `commit()` also
    writes the tables (one rounding to the storage type), the projection and the LayerNorm back.  The default, `False`, is the
    trainer as before, launch for launch.

    `hidden_dropout`, `attention_dropout` (rates in [0, 1), else ValueError) and `seed` (an integer below 2^64): training-mode
    dropout in the trained part of a step, where transformers has it (the module docstring lists the sites).  A rate p acts as
    lrintf(p * 256) / 256, which the read-only properties of the same names return.  The mask of a step is a function of (`seed`, the
    number of steps taken, the site): two trainers with one seed take the same steps, bit for bit.  `attention_dropout > 0` needs
    `compute_dtype=torch.bfloat16` (ValueError in the fp32 mode); `hidden_dropout` works in both modes.  The frozen layers,
    `model(...)` and `commit()` know no dropout.  Both rates 0.0: the trainer as before, launch for launch.

    The model keeps answering with the weights it was loaded with until `commit()`.  Out of scope: see the module docstring."""

    def __init__(self, model, state_dict, train_layers=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(),
                 schedule=None, max_grad_norm=None, compute_dtype=None, train_embeddings=False, hidden_dropout=0.0,
                 attention_dropout=0.0, seed=0):
        self._need_gpu()
        self._hidden_dropout = dropout_rate(hidden_dropout, "hidden_dropout")
        self._attention_dropout = dropout_rate(attention_dropout, "attention_dropout")
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
        if self._attention_dropout > 0 and compute_dtype is None:
            raise ValueError("attention_dropout > 0 needs the mixed mode, compute_dtype=torch.bfloat16: the fp32 attention kernels have no "
                             "dropout form")
        self.enc, self.enc_prefix, self.head, self._pool = _describe(model)
        self.pooled = self._pool is not None
        self.model = model
        enc, cfg = self.enc, self.enc.cfg
        # LayoutLMv3 with a bias term: the attention pair is vk_attention_relpos / vk_attention_relpos_grad and the bias matrices,
        # shared by all layers, are trained; without one the model runs the plain attention and so does the trainer
        self._relpos = self.enc_prefix == "layoutlmv3." and getattr(enc, "_lut", None) is not None
        if self.enc_prefix == "layoutlmv3.":
            if self._relpos and compute_dtype is None:
                raise ValueError("LayoutLMv3 with a relative-position bias needs compute_dtype=torch.bfloat16: the backward of its attention "
                                 "is built for 16-bit operands only (no strict fp32 form)")
            if self._attention_dropout > 0:
                raise ValueError("attention_dropout > 0 with LayoutLMv3: the backward of the position-bias attention has no dropout form; use "
                                 "hidden_dropout, whose sites lie outside the attention")
            if train_embeddings:
                raise ValueError("train_embeddings=True with LayoutLMv3: the backward of its joint embedding stage is not built; train the "
                                 "layers and the head (train_embeddings=False)")
        self._compute_dtype = _check_compute_dtype(compute_dtype, cfg)
        nl = cfg["num_hidden_layers"]
        n = int(train_layers)
        if n == 0:
            raise ValueError("train_layers=0 trains no encoder layer: that is HeadTrainer")
        if not 1 <= n <= nl:
            raise ValueError(f"train_layers must lie in 1..{nl} (num_hidden_layers), got {train_layers}")
        head_keys = (self.head + ".weight", self.head + ".bias")
        if any(k not in getattr(enc, "_head", {}) for k in head_keys):
            raise RuntimeError(f"{type(model).__name__}: load_state_dict() first (no head tensor {head_keys[0]})")
        self.train_embeddings = bool(train_embeddings)
        if self.train_embeddings and n != nl:
            raise ValueError(f"train_embeddings=True needs every layer trained: train_layers must be {nl} (num_hidden_layers), got {train_layers}")
        self.train_layers, self.first = n, nl - n
        H, I = cfg["hidden_size"], cfg["intermediate_size"]
        self.H, self.heads = H, cfg["num_attention_heads"]
        self.ln_eps = cfg.get("layer_norm_eps", LN_EPS)
        spec = []
        self._bias_keys = ()
        if self._relpos:                                                 # (key, term of the table, buckets) of the matrices that exist
            terms = ((("rel_pos_bias", 0, cfg["rel_pos_bins"]),) +
                     ((("rel_pos_x_bias", 1, cfg["rel_2d_pos_bins"]), ("rel_pos_y_bias", 2, cfg["rel_2d_pos_bins"]))
                      if cfg["has_spatial_attention_bias"] else ()))
            self._bias_keys = tuple((f"{self.enc_prefix}encoder.{t}.weight", term, bins) for t, term, bins in terms)
            spec += [(k, (cfg["num_attention_heads"], bins)) for k, _, bins in self._bias_keys]
        if self.train_embeddings:
            spec += _embedding_spec(self.enc_prefix, cfg)
            self._emb = self.enc_prefix + "embeddings."
            self._tables = tuple(k[len(self._emb):-len(".weight")] for k, _ in spec if k.endswith("_embeddings.weight"))
            self.pad_token_id = int(cfg.get("pad_token_id", DEFAULT_PAD_TOKEN_ID[self.enc_prefix]))
            if self._compute_dtype is not None and cfg.get("visual_embedding_dim", 8) % 8:
                raise ValueError(f"compute_dtype=torch.bfloat16: visual_embedding_dim {cfg['visual_embedding_dim']} must be a multiple of 8")
        for i in range(self.first, nl):
            spec += bert_layer_spec(f"{self.enc_prefix}encoder.layer.{i}", H, I)
        if self.pooled:
            spec += [(self._pool + ".weight", (H, H)), (self._pool + ".bias", (H,))]
        spec += [(k, enc._head[k].shape) for k in head_keys]
        keys = tuple(k for k, _ in spec)
        sd = to_numpy({k: state_dict[k] for k in keys if k in state_dict})
        for k, shp in spec:
            if k not in sd:
                raise ValueError(f"state_dict has no tensor '{k}'")
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"state_dict['{k}'] has shape {tuple(sd[k].shape)}, expected {tuple(shp)}")
        for k in head_keys:
            if sd[k].tobytes() != enc._head[k].tobytes():
                raise ValueError(f"state_dict['{k}'] is not the tensor the model was loaded with: pass the model's own checkpoint")
        dev = self.device = enc.device
        # masters and gradients: q, k, v of a layer are the three row blocks of ONE [3H, H] buffer, so that the projection, its
        # dX and its dW are one GEMM each; the per-key tensors are views of it
        p, g, self._layers = {}, {}, []
        for i in range(self.first, nl):
            P = f"{self.enc_prefix}encoder.layer.{i}.attention.self."
            lay = {"prefix": f"{self.enc_prefix}encoder.layer.{i}", "name": f"encoder.layer.{i}"}
            for part in ("weight", "bias"):
                full = torch.from_numpy(np.concatenate([sd[P + t + "." + part] for t in ("query", "key", "value")], 0)).to(dev)
                gfull = torch.zeros_like(full)
                lay["qkv_" + part], lay["g_qkv_" + part] = full, gfull
                for j, t in enumerate(("query", "key", "value")):
                    p[P + t + "." + part], g[P + t + "." + part] = full[j * H:(j + 1) * H], gfull[j * H:(j + 1) * H]
            self._layers.append(lay)
        for k in keys:
            if k not in p:
                p[k] = torch.from_numpy(np.ascontiguousarray(sd[k])).to(dev)
                g[k] = torch.zeros_like(p[k])
        self._hold(keys, p, g, lr, betas, eps, weight_decay, no_decay, schedule)
        # the weight matrix each product of a trained layer reads (the packed QKV master under ".qkv"): the fp32 master, or in the
        # mixed mode its 16-bit copy, refreshed from the master at the start of every step
        self._prec = Precision(self._compute_dtype)
        self._masters = {lay["prefix"] + t: lay["qkv_weight"] if t == ".qkv" else p[lay["prefix"] + t]
                         for lay in self._layers for t in (".qkv",) + _LAYER_MATRICES}
        if self.train_embeddings and not self.pooled:
            self._masters[self._emb + "visual_projection.weight"] = p[self._emb + "visual_projection.weight"]
        self._w = self._masters if self._compute_dtype is None else {k: torch.empty_like(t, dtype=self._compute_dtype)
                                                                     for k, t in self._masters.items()}
        if self._relpos:                                                 # the fold's entry -> bucket map, uploaded once
            from .layoutlmv3 import relpos_bucket_map
            self._r1, self._r2 = cfg["max_rel_pos"], cfg["max_rel_2d_pos"]
            self._bucket = relpos_bucket_map(cfg["rel_pos_bins"], cfg["rel_2d_pos_bins"], self._r1, self._r2).to(dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None:
            if not self.max_grad_norm > 0:
                raise ValueError("max_grad_norm must be positive")
            self._norm_coef = torch.zeros((2,), dtype=torch.float32, device=dev)
            self._clip_work = torch.empty((L.load().vk_grad_clip_workspace_bytes(len(self.keys)) // 8,), dtype=torch.float64, device=dev)

    @property
    def grad_norm(self):
        """The total gradient norm of the last step before clipping, or None when clipping is off (or no step was taken)."""
        if self.max_grad_norm is None or self.steps == 0:
            return None
        return float(self._norm_coef[0])

    @property
    def compute_dtype(self):
        """None: the fp32 trainer; torch.bfloat16: the mixed-precision mode."""
        return self._compute_dtype

    @property
    def hidden_dropout(self):
        """The hidden dropout rate in effect, t / 256."""
        return self._hidden_dropout

    @property
    def attention_dropout(self):
        """The rate in effect on the attention probabilities, t / 256."""
        return self._attention_dropout

    def _drop(self, site, attention=False):
        """(rate, seed, stream) of dropout site number `site` in the step being taken, or None where its rate is 0: the sites are
        0 the embedding output; 1 + 3 i, 2 + 3 i, 3 + 3 i the probabilities, `attention.output.dense` and `output.dense` of trained
        layer i; 1 + 3 n the head's input rows."""
        rate = self._attention_dropout if attention else self._hidden_dropout
        return (rate, self.seed, (self.steps << 16) + site) if rate > 0 else None

    @staticmethod
    def _residual(t, res, drop):
        """t <- dropout(t) + res (dropout: the identity without `drop`), in place."""
        return add_f32(t, res, out=t) if drop is None else dropout_add_f32(t, res, drop, out=t)

    @staticmethod
    def _undrop(dy, drop):
        """The gradient that enters a dropout site's producer from the gradient `dy` of its output (a new tensor; `dy` itself is
        the residual path's)."""
        return dy if drop is None else dropout_add_f32(dy, None, drop)

    # ---- LayoutLMv3's shared bias tables ------------------------------------------------------------------------------------------------
    def _build_lut(self):
        """The device table the attention kernels read, from the fp32 masters by a gather through the bucket map (`relpos_lut`'s
        fold: T1 | TX | TY side by side); a term the config switches off is zeros."""
        n1, n2 = 2 * self._r1 + 1, 2 * self._r2 + 1
        lut = torch.zeros((self.heads, n1 + 2 * n2), dtype=torch.float32, device=self.device)
        for k, term, _ in self._bias_keys:
            off, n = (0, n1) if term == 0 else (n1 + (term - 1) * n2, n2)
            lut[:, off:off + n] = self.p[k][:, self._bucket[off:off + n].long()]
        return lut

    def _frozen_forward(self, inputs):
        """The frozen layers on the model's own kernels.  LayoutLMv3's frozen layers read the shared tables too, so they run with the
        trainer's current table; the model's own is put back (only `commit()` writes it)."""
        if not self._relpos:
            return self.enc._hidden_after(self.first, *inputs)
        own, self.enc._lut = self.enc._lut, self._lut
        try:
            return self.enc._hidden_after(self.first, *inputs)
        finally:
            self.enc._lut = own

    def _attention(self, qkv, mask, B, Lx, drop):
        if not self._relpos:
            return attention(qkv, mask, B, Lx, self.heads, drop)
        from .layoutlmv3 import attention_relpos
        H, rel = self.H, self.enc._rel
        return attention_relpos(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], rel, rel, self._lut, self._r1, self._r2, self.heads, mask)

    def _attention_grad(self, qkv, mask, ctx, dctx, B, Lx, drop):
        """-> dqkv.  LayoutLMv3: also the table's gradient, summed by bucket into the bias matrices' gradients; the layers are
        walked top to bottom, the first writes and the others add, so the order of the sum is fixed."""
        if not self._relpos:
            return attention_grad(qkv, mask, ctx, dctx, B, Lx, self.heads, drop)
        from .layoutlmv3 import attention_relpos_grad, relpos_lut_grad
        H, rel = self.H, self.enc._rel
        dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
        *_, dlut = attention_relpos_grad(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], ctx, dctx, rel, rel, self._lut, self._r1, self._r2,
                                         self.heads, mask, out=tuple(dqkv[:, i * H:(i + 1) * H] for i in range(3)))
        for k, term, _ in self._bias_keys:
            relpos_lut_grad(dlut, self._bucket, self._r1, self._r2, term, self.g[k], accumulate=self._bias_seen)
        self._bias_seen = True
        return dqkv

    def _cast_weights(self):
        """The mixed mode's 16-bit copies of the trained weight matrices from the fp32 masters; the packed QKV master of a layer is
        one cast."""
        for k, master in self._masters.items():
            cast_16(master, self._compute_dtype, out=self._w[k])

    # ---- one post-LN BERT layer (bert_ops.BertOps._bert_layer), activations kept; fp32, or 16-bit operands under self._prec -----------
    def _layer_forward(self, lay, x, mask, B, Lx, site=1):
        """-> (the layer's output, what the backward reads again).  fp32 mode keeps x, qkv, ctx, t1, a, z, h, t2 in fp32.  The mixed
        mode keeps the 16-bit copies of what only a GEMM or the attention backward reads again (x, qkv, ctx, a, h) and the fp32
        inputs of the fp32 backward kernels (t1, t2, z)."""
        P, p, w, pr = lay["prefix"], self.p, self._w, self._prec
        kept = {"x": pr.operand(x)}
        qkv = kept["qkv"] = pr.gemm(kept["x"], w[P + ".qkv"], lay["qkv_bias"], trans_b=True, out16=True)
        ctx = kept["ctx"] = self._attention(qkv, mask, B, Lx, self._drop(site, attention=True))
        t1 = pr.gemm(ctx, w[P + ".attention.output.dense.weight"], p[P + ".attention.output.dense.bias"], trans_b=True)
        kept["t1"] = self._residual(t1, x, self._drop(site + 1))         # the residual, fp32
        a = layernorm_f32(t1, p[P + ".attention.output.LayerNorm.weight"], p[P + ".attention.output.LayerNorm.bias"], self.ln_eps)
        kept["a"] = pr.operand(a)
        z = kept["z"] = pr.gemm(kept["a"], w[P + ".intermediate.dense.weight"], p[P + ".intermediate.dense.bias"], trans_b=True)
        kept["h"] = pr.operand(act_f32(z, L.VK_ACT_GELU))
        t2 = pr.gemm(kept["h"], w[P + ".output.dense.weight"], p[P + ".output.dense.bias"], trans_b=True)
        kept["t2"] = self._residual(t2, a, self._drop(site + 2))
        return layernorm_f32(t2, p[P + ".output.LayerNorm.weight"], p[P + ".output.LayerNorm.bias"], self.ln_eps), kept

    def _layer_backward(self, lay, kept, dy, mask, B, Lx, need_dx, site=1):
        """The layer walked backwards under the fp32 gradient `dy` of its output -> the gradient of its input, or None for the
        lowest trained layer (`need_dx=False`: nothing below it is trained).  Each Linear is one `linear_backward`: in the mixed
        mode an fp32 gradient is cast once and feeds both of its GEMMs (dW straight into the fp32 gradient buffer, dX in fp32, or
        in 16 bits where attention reads it); bias gradients are column sums of the fp32 gradient."""
        P, p, g, w, pr = lay["prefix"], self.p, self.g, self._w, self._prec

        def linear(dy, x, k, **kw):
            return linear_backward(dy, x, w[k + ".weight"], g[k + ".weight"], g[k + ".bias"], prec=pr, **kw)

        k = P + ".output.LayerNorm"
        dt2, _, _ = layernorm_grad(kept["t2"], p[k + ".weight"], dy, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        dz = act_grad_f32(kept["z"], linear(self._undrop(dt2, self._drop(site + 2)), kept["h"], P + ".output.dense"), L.VK_ACT_GELU)
        da = linear(dz, kept["a"], P + ".intermediate.dense")
        add_f32(da, dt2, out=da)                                         # the residual path
        k = P + ".attention.output.LayerNorm"
        dt1, _, _ = layernorm_grad(kept["t1"], p[k + ".weight"], da, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        dctx = linear(self._undrop(dt1, self._drop(site + 1)), kept["ctx"], P + ".attention.output.dense", dx16=True)
        dqkv = self._attention_grad(kept["qkv"], mask, kept["ctx"], dctx, B, Lx, self._drop(site, attention=True))
        dx = linear_backward(dqkv, kept["x"], w[P + ".qkv"], lay["g_qkv_weight"], lay["g_qkv_bias"], need_dx, prec=pr)
        return add_f32(dx, dt1, out=dx) if need_dx else None             # dX = dQKV . Wqkv + the residual path

    # ---- the embedding stage (train_embeddings): fp32 tables, sums and LayerNorm; only visual_projection follows self._prec -----------
    def _embed_columns(self, inputs, B):
        """The int32 index columns of a step, built with torch on the device -> (forward, backward, mask, visual): `forward` lists
        (table names, their index columns, the rows of the joint sequence they fill or None for all); `backward` lists (table name,
        its indices, the rows of the sequence they read or None); `visual`: (the visual features [B * V, D] fp32, their rows)."""
        dev = self.device

        def col(t, shape, fill=0):
            return (torch.full(shape, fill, dtype=torch.int32, device=dev) if t is None else t.to(dev).to(torch.int32)).reshape(-1).contiguous()

        Lt = inputs[0].shape[1]
        ids, pos = col(inputs[0], None), torch.arange(Lt, dtype=torch.int32, device=dev).repeat(B)
        if self.pooled:                                                  # LayoutLMEmbeddings.forward: the nine terms in its order
            _, bbox, attention_mask, token_type_ids = inputs
            box = col(bbox, (B, Lt, 4)).view(-1, 4)
            left, upper, right, lower = (box[:, i].contiguous() for i in range(4))
            cols = dict(word_embeddings=ids, position_embeddings=pos, x_position_embeddings=torch.cat((left, right)),
                        y_position_embeddings=torch.cat((upper, lower)), h_position_embeddings=lower - upper,
                        w_position_embeddings=right - left, token_type_embeddings=col(token_type_ids, (B, Lt)))
            order = (("word_embeddings", ids), ("position_embeddings", pos), ("x_position_embeddings", left), ("y_position_embeddings", upper),
                     ("x_position_embeddings", right), ("y_position_embeddings", lower), ("h_position_embeddings", cols["h_position_embeddings"]),
                     ("w_position_embeddings", cols["w_position_embeddings"]), ("token_type_embeddings", cols["token_type_embeddings"]))
            twice = torch.arange(B * Lt, dtype=torch.int32, device=dev).repeat(2)           # one token, two rows of the x / y table
            backward = [(t, c, twice if c.numel() == 2 * B * Lt else None) for t, c in cols.items()]
            return [(order, None)], backward, additive_mask(attention_mask, dev), None
        _, visual_embeds, attention_mask, visual_attention_mask, token_type_ids, visual_token_type_ids, _ = inputs
        V = visual_embeds.shape[1]
        first = torch.arange(B, dtype=torch.int32, device=dev)[:, None] * (Lt + V)
        text_rows = (first + torch.arange(Lt, dtype=torch.int32, device=dev)).reshape(-1).contiguous()
        vis_rows = (first + Lt + torch.arange(V, dtype=torch.int32, device=dev)).reshape(-1).contiguous()
        # VisualBertEmbeddings.forward: word + token type + position; projection + visual position (id 0) + visual token type (1)
        text = (("word_embeddings", ids), ("token_type_embeddings", col(token_type_ids, (B, Lt))), ("position_embeddings", pos))
        vis = (("visual_position_embeddings", col(None, (B, V))), ("visual_token_type_embeddings", col(visual_token_type_ids, (B, V), 1)))
        am = torch.ones((B, Lt), device=dev) if attention_mask is None else attention_mask.to(dev, torch.float32)
        vm = torch.ones((B, V), device=dev) if visual_attention_mask is None else visual_attention_mask.to(dev, torch.float32)
        backward = [(t, c, text_rows) for t, c in text] + [(t, c, vis_rows) for t, c in vis]
        vf = visual_embeds.to(dev, torch.float32).reshape(B * V, -1).contiguous()
        return [(text, text_rows), (vis, vis_rows)], backward, additive_mask(torch.cat((am, vm), dim=1), dev), (vf, vis_rows)

    def _embed_forward(self, inputs, B, Lx):
        """-> (the LayerNormed embeddings [B * Lx, H] fp32, the additive mask, what `_embed_backward` reads again)."""
        E, p, pr = self._emb, self.p, self._prec
        forward, backward, mask, visual = self._embed_columns(inputs, B)
        pre = torch.empty((B * Lx, self.H), dtype=torch.float32, device=self.device)
        kept = {"pre": pre, "backward": backward}
        for terms, rows in forward:
            base = None
            if rows is not None and rows is visual[1]:                   # the visual rows start from their projection, a Linear
                kept["vf"], kept["vis_rows"] = pr.operand(visual[0]), rows
                base = pr.gemm(kept["vf"], self._w[E + "visual_projection.weight"], p[E + "visual_projection.bias"], trans_b=True)
            embed_sum_f32([p[E + t + ".weight"] for t, _ in terms], torch.stack([c for _, c in terms]), base=base, out=pre, out_row=rows)
        x = layernorm_f32(pre, p[E + "LayerNorm.weight"], p[E + "LayerNorm.bias"], self.ln_eps)
        return self._undrop(x, self._drop(0)), mask, kept              # forward and backward of the site are one function

    def _embed_backward(self, kept, dy):
        """The gradients of the embedding LayerNorm, of every table (one deterministic index-add over `dsum` each; the word
        table's `padding_idx` row stays zero) and of `visual_projection`, from the gradient `dy` of the stage's output."""
        E, p, g = self._emb, self.p, self.g
        dy = self._undrop(dy, self._drop(0))
        dsum, _, _ = layernorm_grad(kept["pre"], p[E + "LayerNorm.weight"], dy, self.ln_eps, dgamma=g[E + "LayerNorm.weight"],
                                    dbeta=g[E + "LayerNorm.bias"])
        for t, idx, rows in kept["backward"]:
            out = g[E + t + ".weight"]
            index_add_rows(dsum, idx, out.shape[0], rows, self.pad_token_id if t == "word_embeddings" else -1, out=out)
        if "vf" in kept:
            k = E + "visual_projection"
            linear_backward(gather_rows_f32(dsum, kept["vis_rows"]), kept["vf"], None, g[k + ".weight"], g[k + ".bias"], need_dx=False,
                            prec=self._prec)

    # ---- one step ---------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, model_inputs, options):
        names = self.enc._INPUTS
        if len(model_inputs) > len(names) or any(k not in names[len(model_inputs):] for k in options):
            raise TypeError(f"step takes the model's inputs {names}")
        return tuple(model_inputs) + tuple(options.get(k) for k in names[len(model_inputs):])

    def _head_rows(self, inputs, B, Lx):
        """Host-side -> the row of [B * Lx, H] each example's head reads (int32 numpy, distinct)."""
        if self.pooled:
            return check_scatter_index(np.arange(B, dtype=np.int64) * Lx, B * Lx)
        from .visualbert import qa_gather_index
        return check_scatter_index(qa_gather_index(inputs[2], B, inputs[0].shape[1], inputs[1].shape[1]), B * Lx)

    @torch.no_grad()
    def step(self, *model_inputs, labels, **options):
        """One training step on `model_inputs` (the model's own arguments): the frozen layers' forward in the model's precision,
        the trained layers in fp32 (or in the mixed mode `compute_dtype` names) and the head in fp32, cross-entropy against `labels [B]` (a class each, -100 to leave a row out),
        backward, clipping where asked, one AdamW step over every trained tensor; the schedule advances.  -> the loss before
        the step, an fp32 device scalar.  Labels are checked on the host before any launch, as `HeadTrainer.step` checks them."""
        inputs = self._inputs(model_inputs, options)
        B = inputs[0].shape[0]
        lab, counted = self._check_labels(labels, B)                     # before the encoder launches anything
        enc, dev, p, g = self.enc, self.device, self.p, self.g
        enc._check(*inputs)
        Lx = inputs[0].shape[1] + (0 if self.pooled else inputs[1].shape[1])
        if self.enc_prefix == "layoutlmv3." and inputs[4] is not None:   # the class token and the patch rows behind the text
            Lx += (enc.cfg["input_size"] // enc.cfg["patch_size"]) ** 2 + 1
        idx = torch.from_numpy(self._head_rows(inputs, B, Lx)).to(dev)
        labels_dev = torch.from_numpy(lab).to(dev)
        if self.train_embeddings and not self.pooled and inputs[6] is not None:
            raise ValueError("image_text_alignment with train_embeddings=True: the mean over aligned positions is a weighted lookup, "
                             "whose backward is not built")
        if self._relpos:
            self._lut, self._bias_seen = self._build_lut(), False
        if not self.train_embeddings:
            x, mask = self._frozen_forward(inputs)
            x = x.to(torch.float32).contiguous()                         # the boundary hidden state
        if self._compute_dtype is not None:
            self._cast_weights()
        if self.train_embeddings:
            x, mask, emb = self._embed_forward(inputs, B, Lx)
        kept = []
        for i, lay in enumerate(self._layers):
            x, act = self._layer_forward(lay, x, mask, B, Lx, site=1 + 3 * i)
            kept.append(act)
        # head forward
        kw, kb = self.head + ".weight", self.head + ".bias"
        rows = gather_rows_f32(x, idx)
        if self.pooled:
            pw, pb = self._pool + ".weight", self._pool + ".bias"
            zp = gemm_f32(rows, p[pw], p[pb], trans_b=True)
            feats = act_f32(zp, L.VK_ACT_TANH)
        else:
            feats = rows
        head_drop = self._drop(1 + 3 * len(self._layers))
        feats = self._undrop(feats, head_drop)                           # the head's input rows, dropped
        logits = gemm_f32(feats, p[kw], p[kb], trans_b=True)
        loss, dlogits = loss_and_grad(logits, labels_dev, counted)
        # backward: head
        drows = self._undrop(linear_backward(dlogits, feats, p[kw], g[kw], g[kb]), head_drop)
        if self.pooled:
            drows = linear_backward(act_grad_f32(zp, drows, L.VK_ACT_TANH), rows, p[pw], g[pw], g[pb])
        dy = scatter_rows_f32(drows, idx, B * Lx)
        # backward: layers, top down
        for j in range(len(self._layers) - 1, -1, -1):
            dy = self._layer_backward(self._layers[j], kept[j], dy, mask, B, Lx, need_dx=j > 0 or self.train_embeddings, site=1 + 3 * j)
        if self.train_embeddings:
            self._embed_backward(emb, dy)
        if self.max_grad_norm is not None:
            grad_clip(self._table, len(self.keys), self._max_n, self.max_grad_norm, self._norm_coef, self._clip_work)
        self._adamw()
        torch.cuda.synchronize(dev)
        return loss

    def commit(self):
        """Repack the masters into the model's packed buffers (host-side, the loaders' `pack`; q, k, v concatenated as the loader
        concatenates them), in place with `copy_`, so that a captured graph stays valid: after it `model(...)` answers with the
        trained layers and head.  No tensor of a frozen layer or table is written."""
        lins, lns = [], []
        for lay in self._layers:
            n, P = lay["name"], lay["prefix"]
            lins.append((n + ".attention.self.qkv", *(P + ".attention.self." + t for t in ("query", "key", "value"))))
            lins += [(n + lin, P + lin) for lin in (".attention.output.dense", ".intermediate.dense", ".output.dense")]
            lns += [(n + ln, P + ln) for ln in (".attention.output.LayerNorm", ".output.LayerNorm")]
        head_keys = (self.head + ".weight", self.head + ".bias")
        if self.pooled:                                                  # `pooler.dense` in the encoder, or the head's own `classifier.dense`
            lins.append((self._pool[len(self.enc_prefix):] if self._pool.startswith(self.enc_prefix) else self._pool, self._pool))
            head_keys += tuple(k for k in (self._pool + ".weight", self._pool + ".bias") if k in self.enc._head)
        lins.append((self.head, self.head))
        if self._relpos:                                                 # the model's own table, written here only
            self.enc._lut.copy_(self._build_lut())
        if self.train_embeddings:                                        # the tables: one rounding to the storage type, on the device
            for t in self._tables:
                self.enc._tab[t].copy_(self.p[self._emb + t + ".weight"])
            lns.append(("embeddings.LayerNorm", self._emb + "LayerNorm"))
            if not self.pooled:
                lins.append(("embeddings.visual_projection", self._emb + "visual_projection"))
        return self._commit(lins, lns, head_keys)
