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

Out of scope: dropout, 16-bit training GEMMs, HIP-graph capture of a step, training the embeddings, ViT (pre-LN layers) and LXMERT
(cross-attention top layers), and running the top layer only on the rows the head reads (for `train_layers=1` the FFN is needed
on B rows, not B * L: measure first, then build it as its own change).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS, bert_layer_spec, to_numpy
from .layers import stream
from .lxmert import IGNORE_INDEX, check_class_labels
from .train import _ptr, act_f32, act_grad_f32, adamw_step, adamw_table, col_sums, cross_entropy_grad, gemm_f32, layernorm_f32, layernorm_grad


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

    The model keeps answering with the weights it was loaded with until `commit()`.  Out of scope: see the module docstring."""

    def __init__(self, model, state_dict, train_layers=1, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(),
                 schedule=None, max_grad_norm=None):
        if not torch.cuda.is_available():
            raise RuntimeError("vltk_amd.EncoderTrainer needs a GPU: there is no CPU fallback")
        self.enc, self.enc_prefix, self.head, self.pooled = _describe(model)
        self.model = model
        enc, cfg = self.enc, self.enc.cfg
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
        the trained layers and the head in fp32, cross-entropy against `labels [B]` (a class each, -100 to leave a row out),
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
            dy = self._layer_backward(self._layers[j], kept[j], dy, mask, B, Lx, need_dx=j > 0)
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
