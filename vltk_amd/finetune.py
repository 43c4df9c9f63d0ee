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

Out of scope: dropout, HIP-graph capture of a step, training the embeddings, ViT (pre-LN layers) and LXMERT (cross-attention top
layers), running the top layer only on the rows the head reads (for `train_layers=1` the FFN is needed on B rows, not B * L:
measure first, then build it as its own change), fp16 as the compute type (its gradients need loss scaling) and producers that
write both precisions at once (the cast passes are measured first).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, bert_layer_spec, to_numpy
from .layers import stream
from .lxmert import IGNORE_INDEX, check_class_labels
from .train import (VK_16, _ptr, act_f32, act_grad_f32, adamw_step, adamw_table, cast_16, col_sums, cross_entropy_grad, gemm_16, gemm_f32,
                    layernorm_f32, layernorm_grad)


# ---- the ops train.py does not have: one call into the C ABI each -----------------------------------------------------------------
def attention_f32(qkv, mask, B, Lx, heads):
    """`vk_attention` in fp32 on a packed projection `qkv [B * Lx, 3H]` -> the context rows [B * Lx, H]."""
    H = qkv.shape[1] // 3
    out = torch.empty((B * Lx, H), dtype=torch.float32, device=qkv.device)
    ld, es = qkv.stride(0), qkv.element_size()
    L.call("vk_attention", qkv.data_ptr(), ld, qkv.data_ptr() + H * es, ld, qkv.data_ptr() + 2 * H * es, ld, _ptr(mask), out.data_ptr(), H,
           B, heads, Lx, Lx, H // heads, L.VK_F32, stream(qkv.device))
    return out


def attention_grad(qkv, mask, ctx, dctx, B, Lx, heads):
    """`vk_attention_grad` on the packed projection the forward kept -> dqkv [B * Lx, 3H] (dQ | dK | dV)."""
    H = qkv.shape[1] // 3
    dqkv = torch.empty_like(qkv)
    ld, es = qkv.stride(0), 4
    nbytes = L.load().vk_attention_grad_workspace_bytes(B, heads, Lx)
    work = torch.empty((nbytes // 4,), dtype=torch.float32, device=qkv.device)
    L.call("vk_attention_grad", qkv.data_ptr(), ld, qkv.data_ptr() + H * es, ld, qkv.data_ptr() + 2 * H * es, ld, _ptr(mask), ctx.data_ptr(),
           ctx.stride(0), dctx.data_ptr(), dctx.stride(0), dqkv.data_ptr(), ld, dqkv.data_ptr() + H * es, ld, dqkv.data_ptr() + 2 * H * es, ld,
           B, heads, Lx, Lx, H // heads, work.data_ptr(), nbytes, stream(qkv.device))
    return dqkv


def attention_16(qkv, mask, B, Lx, heads):
    """`vk_attention_tiled` on a packed bf16 / fp16 projection `qkv [B * Lx, 3H]` -> the context rows [B * Lx, H] in its dtype."""
    H = qkv.shape[1] // 3
    out = torch.empty((B * Lx, H), dtype=qkv.dtype, device=qkv.device)
    ld, es = qkv.stride(0), qkv.element_size()
    L.call("vk_attention_tiled", qkv.data_ptr(), ld, qkv.data_ptr() + H * es, ld, qkv.data_ptr() + 2 * H * es, ld, _ptr(mask), out.data_ptr(),
           H, B, heads, Lx, Lx, H // heads, VK_16[qkv.dtype], stream(qkv.device))
    return out


def attention_grad_16(qkv, mask, ctx, dctx, B, Lx, heads):
    """`vk_attention_grad_16` on the packed 16-bit projection the forward kept, its context rows and their gradient (all of one
    dtype) -> dqkv [B * Lx, 3H] (dQ | dK | dV) in fp32."""
    H = qkv.shape[1] // 3
    assert qkv.dtype in VK_16 and ctx.dtype == dctx.dtype == qkv.dtype
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
    ld, es = qkv.stride(0), qkv.element_size()
    nbytes = L.load().vk_attention_grad_16_workspace_bytes(B, heads, Lx)
    work = torch.empty((nbytes // 4,), dtype=torch.float32, device=qkv.device)
    L.call("vk_attention_grad_16", qkv.data_ptr(), ld, qkv.data_ptr() + H * es, ld, qkv.data_ptr() + 2 * H * es, ld, _ptr(mask),
           ctx.data_ptr(), ctx.stride(0), dctx.data_ptr(), dctx.stride(0), dqkv.data_ptr(), ld, dqkv.data_ptr() + H * 4, ld,
           dqkv.data_ptr() + 2 * H * 4, ld, B, heads, Lx, Lx, H // heads, VK_16[qkv.dtype], work.data_ptr(), nbytes, stream(qkv.device))
    return dqkv


def add_f32(a, b, out=None):
    """a + b (`vk_add_f32`), into `out` (which may be a or b) or a new tensor.  The residual adds: through `vk_gemm_f32`'s
    `accumulate` a residual would take one rounding per step of the K chain, at the residual's magnitude."""
    out = torch.empty_like(a) if out is None else out
    assert a.is_contiguous() and b.is_contiguous() and out.is_contiguous() and a.shape == b.shape == out.shape
    L.call("vk_add_f32", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), stream(a.device))
    return out


def gather_rows_f32(x, idx):
    """Rows `idx` (int32, on the device) of contiguous fp32 `x [M, C]` -> [len(idx), C] (`vk_gather_rows` copies 16-byte lanes)."""
    n, Cn = idx.numel(), x.shape[1]
    if Cn % 4:
        raise ValueError(f"gather of fp32 rows of {Cn} elements: their size must be a multiple of 16 bytes")
    rows = torch.empty((n, Cn), dtype=torch.float32, device=x.device)
    L.call("vk_gather_rows", x.data_ptr(), idx.data_ptr(), n, Cn * 4, rows.data_ptr(), stream(x.device))
    return rows


def check_scatter_index(idx, M):
    """Host-side: `idx` (numpy) holds distinct rows of [0, M), which is what makes `vk_scatter_rows_f32` a single-writer kernel."""
    idx = np.asarray(idx).reshape(-1)
    if idx.size == 0 or idx.min() < 0 or idx.max() >= M:
        raise IndexError(f"scatter rows must lie in [0, {M})")
    if len(np.unique(idx)) != idx.size:
        raise ValueError("scatter rows must be distinct (one per example)")
    return idx.astype(np.int32)


def scatter_rows_f32(src, idx_dev, M):
    """The backward of `gather_rows_f32`: zeros [M, C] with row idx[i] = src[i].  `idx_dev`: int32 on the device, checked by
    `check_scatter_index` on the host."""
    n, Cn = src.shape
    dst = torch.empty((M, Cn), dtype=torch.float32, device=src.device)
    L.call("vk_scatter_rows_f32", src.data_ptr(), src.stride(0), idx_dev.data_ptr(), n, dst.data_ptr(), Cn, M, Cn, stream(src.device))
    return dst


def grad_clip(table, count, max_n, max_norm, norm_coef, work):
    """`clip_grad_norm_` over the table's gradients; `norm_coef` (fp32 [2], device) receives the total norm and the coefficient."""
    L.call("vk_grad_clip", table.data_ptr(), count, max_n, float(max_norm), norm_coef.data_ptr(), work.data_ptr(), work.numel() * 8,
           stream(table.device))


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


class EncoderTrainer:
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
        if not torch.cuda.is_available():
            raise RuntimeError("vltk_amd.EncoderTrainer needs a GPU: there is no CPU fallback")
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
        self.keys = tuple(k for k, _ in spec)
        sd = to_numpy({k: state_dict[k] for k in self.keys if k in state_dict})
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
        self.p, self.g, self._layers = {}, {}, []
        for i in range(self.first, nl):
            P = f"{self.enc_prefix}encoder.layer.{i}.attention.self."
            lay = {"prefix": f"{self.enc_prefix}encoder.layer.{i}", "name": f"encoder.layer.{i}"}
            for part, cat in (("weight", 0), ("bias", 0)):
                full = torch.from_numpy(np.concatenate([sd[P + t + "." + part] for t in ("query", "key", "value")], cat)).to(dev)
                gfull = torch.zeros_like(full)
                lay["qkv_" + part], lay["g_qkv_" + part] = full, gfull
                for j, t in enumerate(("query", "key", "value")):
                    self.p[P + t + "." + part], self.g[P + t + "." + part] = full[j * H:(j + 1) * H], gfull[j * H:(j + 1) * H]
            self._layers.append(lay)
        for k in self.keys:
            if k not in self.p:
                self.p[k] = torch.from_numpy(np.ascontiguousarray(sd[k])).to(dev)
                self.g[k] = torch.zeros_like(self.p[k])
        # the mixed mode's 16-bit copies of the weight matrices, refreshed from the masters at the start of every step
        self._w16 = {}
        if self._compute_dtype is not None:
            for lay in self._layers:
                self._w16[lay["prefix"] + ".qkv"] = torch.empty_like(lay["qkv_weight"], dtype=self._compute_dtype)
                for t in _LAYER_MATRICES:
                    self._w16[lay["prefix"] + t] = torch.empty_like(self.p[lay["prefix"] + t], dtype=self._compute_dtype)
        self.m, self.v = ({k: torch.zeros_like(self.p[k]) for k in self.keys} for _ in range(2))
        self.base_lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.schedule = schedule
        self.steps = 0
        self.num_classes = self.p[head_keys[1]].numel()
        self._table, self._max_n = adamw_table([(self.p[k], self.g[k], self.m[k], self.v[k], not any(f in k for f in no_decay))
                                                for k in self.keys], dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None:
            if not self.max_grad_norm > 0:
                raise ValueError("max_grad_norm must be positive")
            self._norm_coef = torch.zeros((2,), dtype=torch.float32, device=dev)
            self._clip_work = torch.empty((L.load().vk_grad_clip_workspace_bytes(len(self.keys)) // 8,), dtype=torch.float64, device=dev)

    @property
    def lr(self):
        """The rate of the next step."""
        return self.base_lr if self.schedule is None else self.schedule(self.base_lr, self.steps)

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

    # ---- the mixed mode: the same layer with 16-bit operands on the matrix cores, fp32 everywhere else ------------------------------
    def _cast_weights(self):
        """The 16-bit copies of the trained weight matrices from the fp32 masters; the packed QKV master of a layer is one cast."""
        for lay in self._layers:
            P = lay["prefix"]
            cast_16(lay["qkv_weight"], self._compute_dtype, out=self._w16[P + ".qkv"])
            for t in _LAYER_MATRICES:
                cast_16(self.p[P + t], self._compute_dtype, out=self._w16[P + t])

    def _layer_forward_16(self, lay, x, mask, B, Lx):
        """`_layer_forward` with every GEMM and the attention on 16-bit operands.  Kept for the backward: the 16-bit copies of what
        only a GEMM or the attention backward reads again (x, qkv, ctx, a, h) and the fp32 inputs of the fp32 backward kernels
        (t1, t2, z)."""
        P, p, w, dt = lay["prefix"], self.p, self._w16, self._compute_dtype
        kept = {"x": cast_16(x, dt)}
        qkv = kept["qkv"] = gemm_16(kept["x"], w[P + ".qkv"], lay["qkv_bias"], trans_b=True, out_dtype=dt)
        ctx = kept["ctx"] = attention_16(qkv, mask, B, Lx, self.heads)
        t1 = gemm_16(ctx, w[P + ".attention.output.dense.weight"], p[P + ".attention.output.dense.bias"], trans_b=True)
        kept["t1"] = add_f32(t1, x, out=t1)                              # the residual, fp32
        a = layernorm_f32(t1, p[P + ".attention.output.LayerNorm.weight"], p[P + ".attention.output.LayerNorm.bias"], self.ln_eps)
        kept["a"] = cast_16(a, dt)
        z = kept["z"] = gemm_16(kept["a"], w[P + ".intermediate.dense.weight"], p[P + ".intermediate.dense.bias"], trans_b=True)
        kept["h"] = cast_16(act_f32(z, L.VK_ACT_GELU), dt)
        t2 = gemm_16(kept["h"], w[P + ".output.dense.weight"], p[P + ".output.dense.bias"], trans_b=True)
        kept["t2"] = add_f32(t2, a, out=t2)
        return layernorm_f32(t2, p[P + ".output.LayerNorm.weight"], p[P + ".output.LayerNorm.bias"], self.ln_eps), kept

    def _layer_backward_16(self, lay, kept, dy, mask, B, Lx, need_dx):
        """`_layer_backward` in the mixed mode: an fp32 gradient is cast once and feeds both of its GEMMs (dW straight into the fp32
        gradient buffer, dX in fp32, or in 16 bits where attention reads it); bias gradients are column sums of the fp32 gradient."""
        P, p, g, w, dt = lay["prefix"], self.p, self.g, self._w16, self._compute_dtype
        k = P + ".output.LayerNorm"
        dt2, _, _ = layernorm_grad(kept["t2"], p[k + ".weight"], dy, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        k = P + ".output.dense"
        dt2_16 = cast_16(dt2, dt)
        gemm_16(dt2_16, kept["h"], out=g[k + ".weight"], trans_a=True)   # dW = dY^T . X
        col_sums(dt2, out=g[k + ".bias"])
        dz = act_grad_f32(kept["z"], gemm_16(dt2_16, w[k + ".weight"]), L.VK_ACT_GELU)
        k = P + ".intermediate.dense"
        dz_16 = cast_16(dz, dt)
        gemm_16(dz_16, kept["a"], out=g[k + ".weight"], trans_a=True)
        col_sums(dz, out=g[k + ".bias"])
        da = gemm_16(dz_16, w[k + ".weight"])
        add_f32(da, dt2, out=da)                                         # the residual path
        k = P + ".attention.output.LayerNorm"
        dt1, _, _ = layernorm_grad(kept["t1"], p[k + ".weight"], da, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        k = P + ".attention.output.dense"
        dt1_16 = cast_16(dt1, dt)
        gemm_16(dt1_16, kept["ctx"], out=g[k + ".weight"], trans_a=True)
        col_sums(dt1, out=g[k + ".bias"])
        dctx = gemm_16(dt1_16, w[k + ".weight"], out_dtype=dt)
        dqkv = attention_grad_16(kept["qkv"], mask, kept["ctx"], dctx, B, Lx, self.heads)
        dqkv_16 = cast_16(dqkv, dt)
        gemm_16(dqkv_16, kept["x"], out=lay["g_qkv_weight"], trans_a=True)
        col_sums(dqkv, out=lay["g_qkv_bias"])
        if not need_dx:
            return None
        dx = gemm_16(dqkv_16, w[P + ".qkv"])
        return add_f32(dx, dt1, out=dx)

    # ---- one BERT layer in fp32 (bert_ops.BertOps._bert_layer), activations kept ----------------------------------------------------
    def _layer_forward(self, lay, x, mask, B, Lx):
        P, p = lay["prefix"], self.p
        kept = {"x": x}
        qkv = kept["qkv"] = gemm_f32(x, lay["qkv_weight"], lay["qkv_bias"], trans_b=True)
        ctx = kept["ctx"] = attention_f32(qkv, mask, B, Lx, self.heads)
        t1 = gemm_f32(ctx, p[P + ".attention.output.dense.weight"], p[P + ".attention.output.dense.bias"], trans_b=True)
        kept["t1"] = add_f32(t1, x, out=t1)                              # the residual
        a = kept["a"] = layernorm_f32(t1, p[P + ".attention.output.LayerNorm.weight"], p[P + ".attention.output.LayerNorm.bias"], self.ln_eps)
        z = kept["z"] = gemm_f32(a, p[P + ".intermediate.dense.weight"], p[P + ".intermediate.dense.bias"], trans_b=True)
        hact = kept["h"] = act_f32(z, L.VK_ACT_GELU)
        t2 = gemm_f32(hact, p[P + ".output.dense.weight"], p[P + ".output.dense.bias"], trans_b=True)
        kept["t2"] = add_f32(t2, a, out=t2)
        return layernorm_f32(t2, p[P + ".output.LayerNorm.weight"], p[P + ".output.LayerNorm.bias"], self.ln_eps), kept

    def _layer_backward(self, lay, kept, dy, mask, B, Lx, need_dx):
        P, p, g = lay["prefix"], self.p, self.g
        k = P + ".output.LayerNorm"
        dt2, _, _ = layernorm_grad(kept["t2"], p[k + ".weight"], dy, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        k = P + ".output.dense"
        gemm_f32(dt2, kept["h"], out=g[k + ".weight"], trans_a=True)     # dW = dY^T . X
        col_sums(dt2, out=g[k + ".bias"])
        dz = act_grad_f32(kept["z"], gemm_f32(dt2, p[k + ".weight"]), L.VK_ACT_GELU)
        k = P + ".intermediate.dense"
        gemm_f32(dz, kept["a"], out=g[k + ".weight"], trans_a=True)
        col_sums(dz, out=g[k + ".bias"])
        da = gemm_f32(dz, p[k + ".weight"])
        add_f32(da, dt2, out=da)                                         # the residual path
        k = P + ".attention.output.LayerNorm"
        dt1, _, _ = layernorm_grad(kept["t1"], p[k + ".weight"], da, self.ln_eps, dgamma=g[k + ".weight"], dbeta=g[k + ".bias"])
        k = P + ".attention.output.dense"
        gemm_f32(dt1, kept["ctx"], out=g[k + ".weight"], trans_a=True)
        col_sums(dt1, out=g[k + ".bias"])
        dctx = gemm_f32(dt1, p[k + ".weight"])
        dqkv = attention_grad(kept["qkv"], mask, kept["ctx"], dctx, B, Lx, self.heads)
        gemm_f32(dqkv, kept["x"], out=lay["g_qkv_weight"], trans_a=True)
        col_sums(dqkv, out=lay["g_qkv_bias"])
        if not need_dx:                                                  # the lowest trained layer: nothing below it is trained
            return None
        dx = gemm_f32(dqkv, lay["qkv_weight"])                           # dX = dQKV . Wqkv + the residual path
        return add_f32(dx, dt1, out=dx)

    # ---- one step ---------------------------------------------------------------------------------------------------------------------------
    def _check_labels(self, labels, B):
        lab = check_class_labels("labels", labels, (B,), self.num_classes)
        counted = int((lab != IGNORE_INDEX).sum())
        if counted == 0:
            raise ValueError(f"labels: every label is {IGNORE_INDEX}, so no row counts and the mean loss is undefined")
        return lab, counted

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
        mixed = self._compute_dtype is not None
        if mixed:
            self._cast_weights()
        kept = []
        for lay in self._layers:
            x, act = (self._layer_forward_16 if mixed else self._layer_forward)(lay, x, mask, B, Lx)
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
        per_row = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L.call("vk_cross_entropy", logits.data_ptr(), logits.stride(0), B, self.num_classes, labels_dev.data_ptr(), IGNORE_INDEX,
               per_row.data_ptr(), L.VK_F32, stream(dev))
        L.call("vk_loss_reduce", per_row.data_ptr(), None, labels_dev.data_ptr(), IGNORE_INDEX, B, 1.0, loss.data_ptr(), stream(dev))
        # backward: head
        dlogits = cross_entropy_grad(logits, labels_dev, 1.0 / counted)
        gemm_f32(dlogits, feats, out=g[kw], trans_a=True)
        col_sums(dlogits, out=g[kb])
        drows = gemm_f32(dlogits, p[kw])
        if self.pooled:
            dzp = act_grad_f32(zp, drows, L.VK_ACT_TANH)
            gemm_f32(dzp, rows, out=g[pw], trans_a=True)
            col_sums(dzp, out=g[pb])
            drows = gemm_f32(dzp, p[pw])
        dy = scatter_rows_f32(drows, idx, B * Lx)
        # backward: layers, top down
        for j in range(len(self._layers) - 1, -1, -1):
            dy = (self._layer_backward_16 if mixed else self._layer_backward)(self._layers[j], kept[j], dy, mask, B, Lx, need_dx=j > 0)
        if self.max_grad_norm is not None:
            grad_clip(self._table, len(self.keys), self._max_n, self.max_grad_norm, self._norm_coef, self._clip_work)
        adamw_step(self._table, len(self.keys), self._max_n, self.lr, self.betas, self.eps, self.weight_decay, self.steps + 1, dev)
        self.steps += 1
        torch.cuda.synchronize(dev)
        return loss

    # ---- what it holds ---------------------------------------------------------------------------------------------------------------------
    def grads(self):
        """The last step's gradients by key (after clipping, as `.grad` is in torch), fp32 numpy arrays."""
        return {k: self.g[k].cpu().numpy() for k in self.keys}

    def state_dict(self):
        """The trained tensors by transformers' key names, fp32 numpy arrays."""
        return {k: self.p[k].cpu().numpy() for k in self.keys}

    def commit(self):
        """Repack the masters into the model's packed buffers (host-side, the loaders' `pack`; q, k, v concatenated as the loader
        concatenates them), in place with `copy_`, so that a captured graph stays valid: after it `model(...)` answers with the
        trained layers and head.  No tensor of a frozen layer or table is written."""
        enc, sd, pre = self.enc, self.state_dict(), self.enc_prefix

        def put_lin(name, *parts):
            w = np.concatenate([sd[q + ".weight"] for q in parts], 0)
            b = np.concatenate([sd[q + ".bias"] for q in parts], 0)
            wp, bp, _, _ = enc._pack(w, b)
            enc._lin[name][0].copy_(wp)
            enc._lin[name][1].copy_(bp)

        def put_ln(name, key):
            for t, part in zip(enc._ln[name], ("weight", "bias")):
                t.copy_(torch.from_numpy(sd[f"{key}.{part}"]))

        for lay in self._layers:
            n, P = lay["name"], lay["prefix"]
            put_lin(n + ".attention.self.qkv", *(P + ".attention.self." + t for t in ("query", "key", "value")))
            for lin in (".attention.output.dense", ".intermediate.dense", ".output.dense"):
                put_lin(n + lin, P + lin)
            for ln in (".attention.output.LayerNorm", ".output.LayerNorm"):
                put_ln(n + ln, P + ln)
        if self.pooled:
            put_lin("pooler.dense", pre + "pooler.dense")
        put_lin(self.head, self.head)
        for k in (self.head + ".weight", self.head + ".bias"):
            enc._head[k] = sd[k].copy()
        torch.cuda.synchronize(self.device)
        return self.model
