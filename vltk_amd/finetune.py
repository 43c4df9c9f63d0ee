"""N8: fine-tune the top encoder layers and the answer head.  The reference's training script (`vltk/legacy/legacy_train.py`)
trains the whole `VisualBertForQuestionAnswering`; its framework step (`vltk/abc/simple.py:665-682`) is `loss.backward();
clip_grad_norm_(params, config.train.max_norm); optim.step(); scheduler.step()` with `max_norm = 5.0` (`configs.py:88`), and
`freeze_layers` (`vltk/abc/complex.py:109-120`) freezes a prefix of the layers and trains the rest: the recipe on extracted
features.  `EncoderTrainer` is that recipe: the first `L - n` layers run the encoder's own forward in its own precision, the last
`n` layers and the head run in fp32 with every activation the backward needs kept, and are walked backwards.

Forward, loss, backward, clipping and the optimiser step are kernels of csrc/train.hip and csrc/attention_grad.hip
(`vk_gemm_f32`, `vk_attention` in fp32, `vk_attention_grad`, `vk_layernorm`, `vk_layernorm_grad`, `vk_act_f32`, `vk_act_grad_f32`,
`vk_col_sums`, `vk_add_f32` for the residuals, `vk_scatter_rows_f32`, `vk_cross_entropy(_grad)`, `vk_grad_clip`, `vk_adamw_step`)
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

Out of scope: dropout, HIP-graph capture of a step, training the embeddings, ViT (pre-LN layers) and LXMERT (cross-attention top
layers), running the top layer only on the rows the head reads (for `train_layers=1` the FFN is needed on B rows, not B * L:
measure first, then build it as its own change), fp16 as the compute type (its gradients need loss scaling) and producers that
write both precisions at once (the cast passes are measured first).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, bert_layer_spec, to_numpy
from .train import (Precision, _Trainer, act_f32, act_grad_f32, add_f32, attention, attention_grad, cast_16, check_scatter_index,
                    gather_rows_f32, gemm_f32, grad_clip, layernorm_f32, layernorm_grad, linear_backward, loss_and_grad, scatter_rows_f32)


# ---- what is trained ---------------------------------------------------------------------------------------------------------------------
def _describe(model):
    """-> (encoder, its state-dict prefix, head prefix, whether `pooler.dense` stands between the layers and the head)."""
    from .layoutlm import LayoutLMForSequenceClassification
    from .visualbert import VisualBertForQuestionAnswering
    if isinstance(model, VisualBertForQuestionAnswering):
        return model.visual_bert, "visual_bert.", "cls", False
    if isinstance(model, LayoutLMForSequenceClassification):
        return model.layoutlm, "layoutlm.", "classifier", True
    why = {"ViTForImageClassification": ": ViT's layers are pre-LN, the backward here is the post-LN BERT layer's",
           "LxmertForQuestionAnswering": ": LXMERT's top layers are cross-attention layers"}.get(type(model).__name__, "")
    raise TypeError(f"EncoderTrainer takes VisualBertForQuestionAnswering or LayoutLMForSequenceClassification, not {type(model).__name__}{why}")


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


# the weight matrices of a trained layer that the mixed mode keeps a 16-bit copy of (the packed [3H, H] QKV master beside them)
_LAYER_MATRICES = (".attention.output.dense.weight", ".intermediate.dense.weight", ".output.dense.weight")


class EncoderTrainer(_Trainer):
    """`EncoderTrainer(model, state_dict, train_layers=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(),
    schedule=None, max_grad_norm=None)`: trains the last `train_layers` BERT layers and the head of
    `VisualBertForQuestionAnswering` (layers -> the gathered row -> `cls`) or `LayoutLMForSequenceClassification` (layers ->
    `pooler.dense` + tanh on the first token -> `classifier`; `pooler.dense` is trained too) with cross-entropy, optional clipping
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

    The model keeps answering with the weights it was loaded with until `commit()`.  Out of scope: see the module docstring."""

    def __init__(self, model, state_dict, train_layers=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(),
                 schedule=None, max_grad_norm=None, compute_dtype=None):
        self._need_gpu()
        self.enc, self.enc_prefix, self.head, self.pooled = _describe(model)
        self.model = model
        enc, cfg = self.enc, self.enc.cfg
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
        self.train_layers, self.first = n, nl - n
        H, I = cfg["hidden_size"], cfg["intermediate_size"]
        self.H, self.heads = H, cfg["num_attention_heads"]
        self.ln_eps = cfg.get("layer_norm_eps", LN_EPS)
        spec = []
        for i in range(self.first, nl):
            spec += bert_layer_spec(f"{self.enc_prefix}encoder.layer.{i}", H, I)
        if self.pooled:
            spec += [(self.enc_prefix + "pooler.dense.weight", (H, H)), (self.enc_prefix + "pooler.dense.bias", (H,))]
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
        self._w = self._masters if self._compute_dtype is None else {k: torch.empty_like(t, dtype=self._compute_dtype)
                                                                     for k, t in self._masters.items()}
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

    def _cast_weights(self):
        """The mixed mode's 16-bit copies of the trained weight matrices from the fp32 masters; the packed QKV master of a layer is
        one cast."""
        for k, master in self._masters.items():
            cast_16(master, self._compute_dtype, out=self._w[k])

    # ---- one post-LN BERT layer (bert_ops.BertOps._bert_layer), activations kept; fp32, or 16-bit operands under self._prec -----------
    def _layer_forward(self, lay, x, mask, B, Lx):
        """-> (the layer's output, what the backward reads again).  fp32 mode keeps x, qkv, ctx, t1, a, z, h, t2 in fp32.  The mixed
        mode keeps the 16-bit copies of what only a GEMM or the attention backward reads again (x, qkv, ctx, a, h) and the fp32
        inputs of the fp32 backward kernels (t1, t2, z)."""
        P, p, w, pr = lay["prefix"], self.p, self._w, self._prec
        kept = {"x": pr.operand(x)}
        qkv = kept["qkv"] = pr.gemm(kept["x"], w[P + ".qkv"], lay["qkv_bias"], trans_b=True, out16=True)
        ctx = kept["ctx"] = attention(qkv, mask, B, Lx, self.heads)
        t1 = pr.gemm(ctx, w[P + ".attention.output.dense.weight"], p[P + ".attention.output.dense.bias"], trans_b=True)
        kept["t1"] = add_f32(t1, x, out=t1)                              # the residual, fp32
        a = layernorm_f32(t1, p[P + ".attention.output.LayerNorm.weight"], p[P + ".attention.output.LayerNorm.bias"], self.ln_eps)
        kept["a"] = pr.operand(a)
        z = kept["z"] = pr.gemm(kept["a"], w[P + ".intermediate.dense.weight"], p[P + ".intermediate.dense.bias"], trans_b=True)
        kept["h"] = pr.operand(act_f32(z, L.VK_ACT_GELU))
        t2 = pr.gemm(kept["h"], w[P + ".output.dense.weight"], p[P + ".output.dense.bias"], trans_b=True)
        kept["t2"] = add_f32(t2, a, out=t2)
        return layernorm_f32(t2, p[P + ".output.LayerNorm.weight"], p[P + ".output.LayerNorm.bias"], self.ln_eps), kept

    def _layer_backward(self, lay, kept, dy, mask, B, Lx, need_dx):
        """The layer walked backwards under the fp32 gradient `dy` of its output -> the gradient of its input, or None for the
        lowest trained layer (`need_dx=False`: nothing below it is trained).  Each Linear is one `linear_backward`: in the mixed
        mode an fp32 gradient is cast once and feeds both of its GEMMs (dW straight into the fp32 gradient buffer, dX in fp32, or
        in 16 bits where attention reads it); bias gradients are column sums of the fp32 gradient."""
        P, p, g, w, pr = lay["prefix"], self.p, self.g, self._w, self._prec

        def linear(dy, x, k, **kw):
            return linear_backward(dy, x, w[k + ".weight"], g[k + ".weight"], g[k + ".bias"], prec=pr, **kw)

        k = P + ".output.LayerNorm"
        dt2, _, _ = layernorm_grad(kept["t2"], p[k + ".weight"], dy, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        dz = act_grad_f32(kept["z"], linear(dt2, kept["h"], P + ".output.dense"), L.VK_ACT_GELU)
        da = linear(dz, kept["a"], P + ".intermediate.dense")
        add_f32(da, dt2, out=da)                                         # the residual path
        k = P + ".attention.output.LayerNorm"
        dt1, _, _ = layernorm_grad(kept["t1"], p[k + ".weight"], da, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        dctx = linear(dt1, kept["ctx"], P + ".attention.output.dense", dx16=True)
        dqkv = attention_grad(kept["qkv"], mask, kept["ctx"], dctx, B, Lx, self.heads)
        dx = linear_backward(dqkv, kept["x"], w[P + ".qkv"], lay["g_qkv_weight"], lay["g_qkv_bias"], need_dx, prec=pr)
        return add_f32(dx, dt1, out=dx) if need_dx else None             # dX = dQKV . Wqkv + the residual path

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
        idx = torch.from_numpy(self._head_rows(inputs, B, Lx)).to(dev)
        labels_dev = torch.from_numpy(lab).to(dev)
        x, mask = enc._hidden_after(self.first, *inputs)
        x = x.to(torch.float32).contiguous()                             # the boundary hidden state
        if self._compute_dtype is not None:
            self._cast_weights()
        kept = []
        for lay in self._layers:
            x, act = self._layer_forward(lay, x, mask, B, Lx)
            kept.append(act)
        # head forward
        kw, kb = self.head + ".weight", self.head + ".bias"
        rows = gather_rows_f32(x, idx)
        if self.pooled:
            pw, pb = self.enc_prefix + "pooler.dense.weight", self.enc_prefix + "pooler.dense.bias"
            zp = gemm_f32(rows, p[pw], p[pb], trans_b=True)
            feats = act_f32(zp, L.VK_ACT_TANH)
        else:
            feats = rows
        logits = gemm_f32(feats, p[kw], p[kb], trans_b=True)
        loss, dlogits = loss_and_grad(logits, labels_dev, counted)
        # backward: head
        drows = linear_backward(dlogits, feats, p[kw], g[kw], g[kb])
        if self.pooled:
            drows = linear_backward(act_grad_f32(zp, drows, L.VK_ACT_TANH), rows, p[pw], g[pw], g[pb])
        dy = scatter_rows_f32(drows, idx, B * Lx)
        # backward: layers, top down
        for j in range(len(self._layers) - 1, -1, -1):
            dy = self._layer_backward(self._layers[j], kept[j], dy, mask, B, Lx, need_dx=j > 0)
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
        if self.pooled:
            lins.append(("pooler.dense", self.enc_prefix + "pooler.dense"))
        lins.append((self.head, self.head))
        return self._commit(lins, lns, (self.head + ".weight", self.head + ".bias"))
