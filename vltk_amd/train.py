"""N7: train an answer head over a frozen encoder.  The reference's only training loop, `vltk/legacy/legacy_train.py`, fine-tunes
a QA model on the extractor's features: cross-entropy on `question_answering_score`, `AdamW(params, 1e-4)`, `StepLR(200, 0.9)`,
and a linear warm-up kept beside it.  `HeadTrainer` is the slice of that loop practitioners run first on extracted features: the
encoder frozen (its existing forward), its head trained in fp32.

Forward, loss, backward and the optimiser step are the kernels of csrc/train.hip (`vk_gemm_f32` in its three transposition forms,
`vk_act_f32`, `vk_col_sums`, `vk_cross_entropy_grad`, `vk_act_grad_f32`, `vk_layernorm_grad`, `vk_adamw_step`) with `vk_layernorm`,
`vk_cross_entropy` and `vk_loss_reduce` in fp32.  All arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No
CPU fallback.

This module is also what both trainers stand on: every op wrapper of the training stack (one call into the C ABI each, the
attention, residual, gather / scatter and clipping wrappers of `EncoderTrainer` among them), `linear_backward` and `loss_and_grad`,
the `Precision` of a trained layer's products, and `_Trainer`, the base that holds masters, gradients, AdamW's state, the
schedule and `commit()`'s repacking.

Out of scope: dropout (the heads here have none in eval mode; the dropout transformers' VisualBERT puts before `cls` is omitted),
gradient clipping, HIP-graph capture of a step, 16-bit training GEMMs, any gradient into an encoder, and the soft-label KL loss of
transformers' VisualBERT-QA (the reference's script passes hard labels).  Gradient clipping and the gradient into the top
encoder layers are `EncoderTrainer`'s (finetune.py).
"""
import numpy as np
import torch

from . import _lib as L
from .bert_ops import LN_EPS
from .layers import stream
from .lxmert import IGNORE_INDEX, check_class_labels


# ---- schedules: plain host functions (base rate, number of steps taken) -> the rate of the next step ----------------------------
def step_lr(step_size, gamma):
    """`torch.optim.lr_scheduler.StepLR(step_size, gamma)`: the rate is multiplied by gamma once per `step_size` steps, one
    multiplication at a time as the scheduler does it (gamma ** k may differ in the last bit)."""
    step_size = int(step_size)
    if step_size < 1:
        raise ValueError("step_size must be >= 1")

    def rate(base, step):
        lr = float(base)
        for _ in range(step // step_size):
            lr *= gamma
        return lr
    return rate


def linear_warmup(num_warmup_steps, num_training_steps):
    """transformers' `get_linear_schedule_with_warmup`: up from 0 over the warm-up steps, then down to 0 at the last step."""
    def factor(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))
    return lambda base, step: float(base) * factor(step)


def bias_corrections(beta1, beta2, step):
    """`1 - beta ** step` of AdamW's step number `step` (1 for the first), in fp64."""
    return 1.0 - beta1 ** step, 1.0 - beta2 ** step


# ---- the ops: one call into the C ABI each, fp32 device tensors with unit column stride ------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def gemm_f32(a, b, bias=None, out=None, trans_a=False, trans_b=False, accumulate=False):
    """out [M, N] = op(a) . op(b) (+ bias) (+ out): `vk_gemm_f32` on 2-D fp32 tensors, whose row strides are the leading
    dimensions."""
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    N = b.shape[0] if trans_b else b.shape[1]
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    for t in (a, b, out):
        assert t.dtype == torch.float32 and t.stride(1) == 1
    L.call("vk_gemm_f32", a.data_ptr(), a.stride(0), int(trans_a), b.data_ptr(), b.stride(0), int(trans_b), _ptr(bias), out.data_ptr(),
           out.stride(0), M, N, K, int(accumulate), stream(a.device))
    return out


# the 16-bit ops of EncoderTrainer's mixed-precision mode (finetune.py): bf16 / fp16 operands, fp32 accumulation
VK_16 = {torch.bfloat16: L.VK_BF16, torch.float16: L.VK_F16}


def cast_16(x, dtype=torch.bfloat16, out=None):
    """Contiguous fp32 `x` rounded to `dtype` (bf16 / fp16, nearest even): `vk_cast_16`, into `out` or a new tensor."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else out
    assert out.dtype == dtype and out.is_contiguous() and out.shape == x.shape
    L.call("vk_cast_16", x.data_ptr(), out.data_ptr(), x.numel(), VK_16[dtype], stream(x.device))
    return out


def gemm_16(a, b, bias=None, out=None, trans_a=False, trans_b=False, out_dtype=torch.float32):
    """out [M, N] = op(a) . op(b) (+ bias): `vk_gemm_16` on 2-D bf16 / fp16 tensors of one dtype, fp32 accumulation; `out` (or
    `out_dtype` for a new tensor) is fp32 or the operands' dtype.  The fp32 bias is added in fp32."""
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    N = b.shape[0] if trans_b else b.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    assert a.dtype == b.dtype and a.dtype in VK_16 and out.dtype in (torch.float32, a.dtype)
    assert bias is None or bias.dtype == torch.float32
    for t in (a, b, out):
        assert t.stride(1) == 1
    L.call("vk_gemm_16", a.data_ptr(), a.stride(0), int(trans_a), b.data_ptr(), b.stride(0), int(trans_b), _ptr(bias), out.data_ptr(),
           out.stride(0), M, N, K, VK_16[a.dtype], L.VK_F32 if out.dtype == torch.float32 else VK_16[a.dtype], stream(a.device))
    return out


def col_sums(x, out=None):
    M, N = x.shape
    out = torch.empty((N,), dtype=torch.float32, device=x.device) if out is None else out
    nbytes = L.load().vk_col_sums_workspace_bytes(M, N)
    work = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device) if nbytes else None
    L.call("vk_col_sums", x.data_ptr(), x.stride(0), M, N, out.data_ptr(), _ptr(work), nbytes, stream(x.device))
    return out


def cross_entropy_grad(logits, labels, scale, out=None):
    M, Cn = logits.shape
    out = torch.empty((M, Cn), dtype=torch.float32, device=logits.device) if out is None else out
    L.call("vk_cross_entropy_grad", logits.data_ptr(), logits.stride(0), M, Cn, labels.data_ptr(), IGNORE_INDEX, float(scale),
           out.data_ptr(), out.stride(0), stream(logits.device))
    return out


def act_f32(x, act):
    y = torch.empty_like(x)
    L.call("vk_act_f32", x.data_ptr(), y.data_ptr(), x.numel(), act, stream(x.device))
    return y


def act_grad_f32(x, dy, act):
    dx = torch.empty_like(x)
    L.call("vk_act_grad_f32", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), act, stream(x.device))
    return dx


def layernorm_f32(x, gamma, beta, eps):
    M, Cn = x.shape
    y = torch.empty_like(x)
    L.call("vk_layernorm", x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y.stride(0), M, Cn, eps, 1.0, 0,
           L.VK_F32, stream(x.device))
    return y


def layernorm_grad(x, gamma, dy, eps, dgamma=None, dbeta=None):
    """-> (dx, dgamma, dbeta) of `LayerNorm(x) * gamma + beta` under the output gradient dy (`vk_layernorm_grad`)."""
    M, Cn = x.shape
    dx = torch.empty((M, Cn), dtype=torch.float32, device=x.device)
    dgamma = torch.empty((Cn,), dtype=torch.float32, device=x.device) if dgamma is None else dgamma
    dbeta = torch.empty((Cn,), dtype=torch.float32, device=x.device) if dbeta is None else dbeta
    nbytes = L.load().vk_layernorm_grad_workspace_bytes(M, Cn)
    work = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    L.call("vk_layernorm_grad", x.data_ptr(), x.stride(0), gamma.data_ptr(), dy.data_ptr(), dy.stride(0), dx.data_ptr(), dx.stride(0),
           dgamma.data_ptr(), dbeta.data_ptr(), M, Cn, float(eps), work.data_ptr(), nbytes, stream(x.device))
    return dx, dgamma, dbeta


def adamw_table(records, device):
    """[(p, g, m, v, decay)] of fp32 device tensors -> (the device table `vk_adamw_step` reads, the largest element count)."""
    tab = (L.vk_adamw_tensor * len(records))()
    for r, (p, g, m, v, decay) in zip(tab, records):
        assert p.numel() == g.numel() == m.numel() == v.numel()
        r.p, r.g, r.m, r.v, r.n, r.decay, r.reserved = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), int(bool(decay)), 0
    host = np.frombuffer(bytes(tab), np.uint8).copy()
    return torch.from_numpy(host).to(device), max(p.numel() for p, *_ in records)


def adamw_step(table, count, max_n, lr, betas, eps, weight_decay, step, device):
    """One `torch.optim.AdamW` step (step number `step`, 1 for the first) over the tensors of the table, in one launch."""
    bc1, bc2 = bias_corrections(betas[0], betas[1], step)
    L.call("vk_adamw_step", table.data_ptr(), count, max_n, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
           bc1, bc2, stream(device))


def packed_qkv(t):
    """A packed `[rows, 3H]` tensor (Q | K | V, or their gradients) -> the six (pointer, row stride) arguments of its three parts."""
    ptr, ld, step = t.data_ptr(), t.stride(0), t.shape[1] // 3 * t.element_size()
    return ptr, ld, ptr + step, ld, ptr + 2 * step, ld


def attention(qkv, mask, B, Lx, heads):
    """Self-attention on a packed projection `qkv [B * Lx, 3H]` -> the context rows [B * Lx, H] in its dtype: `vk_attention` in
    fp32, `vk_attention_tiled` on bf16 / fp16."""
    H = qkv.shape[1] // 3
    out = torch.empty((B * Lx, H), dtype=qkv.dtype, device=qkv.device)
    entry, dt = ("vk_attention", L.VK_F32) if qkv.dtype == torch.float32 else ("vk_attention_tiled", VK_16[qkv.dtype])
    L.call(entry, *packed_qkv(qkv), _ptr(mask), out.data_ptr(), H, B, heads, Lx, Lx, H // heads, dt, stream(qkv.device))
    return out


def attention_grad(qkv, mask, ctx, dctx, B, Lx, heads):
    """The backward of `attention` on the packed projection the forward kept, its context rows and their gradient (all of one
    dtype) -> dqkv [B * Lx, 3H] (dQ | dK | dV) in fp32: `vk_attention_grad` in fp32, `vk_attention_grad_16` on bf16 / fp16."""
    H = qkv.shape[1] // 3
    assert ctx.dtype == dctx.dtype == qkv.dtype
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
    entry, dt = ("vk_attention_grad", ()) if qkv.dtype == torch.float32 else ("vk_attention_grad_16", (VK_16[qkv.dtype],))
    nbytes = getattr(L.load(), entry + "_workspace_bytes")(B, heads, Lx)
    work = torch.empty((nbytes // 4,), dtype=torch.float32, device=qkv.device)
    L.call(entry, *packed_qkv(qkv), _ptr(mask), ctx.data_ptr(), ctx.stride(0), dctx.data_ptr(), dctx.stride(0), *packed_qkv(dqkv),
           B, heads, Lx, Lx, H // heads, *dt, work.data_ptr(), nbytes, stream(qkv.device))
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
    if Cn * x.element_size() % 16:
        raise ValueError(f"gather of fp32 rows of {Cn} elements: their size must be a multiple of 16 bytes")
    rows = torch.empty((n, Cn), dtype=torch.float32, device=x.device)
    L.call("vk_gather_rows", x.data_ptr(), idx.data_ptr(), n, Cn * x.element_size(), rows.data_ptr(), stream(x.device))
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
    L.call("vk_grad_clip", table.data_ptr(), count, max_n, float(max_norm), norm_coef.data_ptr(), work.data_ptr(),
           work.numel() * work.element_size(), stream(table.device))


# ---- what the two trainers compose from the ops ----------------------------------------------------------------------------------------
class Precision:
    """What the fp32 and the mixed mode of a trained layer differ on.  `Precision(None)`: fp32 operands on `vk_gemm_f32`, and
    `operand` is the identity, so the mode issues no cast.  `Precision(torch.bfloat16)`: an fp32 tensor becomes an operand through
    one `vk_cast_16` where it is first used, the products run on `vk_gemm_16`, and `out16=True` has a product written in the
    16-bit type (what attention reads); every other product, and every product of the fp32 mode, is written in fp32."""

    def __init__(self, dtype=None):
        self.dtype = dtype

    def operand(self, t):
        return t if self.dtype is None else cast_16(t, self.dtype)

    def gemm(self, a, b, bias=None, out=None, trans_a=False, trans_b=False, out16=False):
        if self.dtype is None:
            return gemm_f32(a, b, bias, out, trans_a, trans_b)
        return gemm_16(a, b, bias, out, trans_a, trans_b, out_dtype=self.dtype if out16 else torch.float32)


FP32 = Precision()


def linear_backward(dy, x, w, gw, gb, need_dx=True, prec=FP32, dx16=False):
    """The backward of `y = x . w^T + b` under the fp32 gradient `dy`, in three launches: dW = dY^T . X into `gw`, db = the column
    sums of dY into `gb`, then, where asked, dX = dY . W, which is returned (None otherwise).  `x` and `w` are `prec`'s operands
    (the 16-bit copies in the mixed mode); `dy` becomes one once and feeds both of its products, the bias gradient sums the fp32
    `dy`.  `dx16`: dX in the mixed mode's 16-bit type."""
    dyo = prec.operand(dy)
    prec.gemm(dyo, x, out=gw, trans_a=True)
    col_sums(dy, out=gb)
    return prec.gemm(dyo, w, out16=dx16) if need_dx else None


def loss_and_grad(logits, labels_dev, counted):
    """Mean cross-entropy of fp32 `logits [M, C]` over the `counted` rows whose label (int64, on the device) is not IGNORE_INDEX
    (`vk_cross_entropy`, `vk_loss_reduce`) and its gradient (`vk_cross_entropy_grad`) -> (loss, an fp32 device scalar; dlogits)."""
    M, Cn = logits.shape
    dev = logits.device
    rows = torch.empty((M,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    L.call("vk_cross_entropy", logits.data_ptr(), logits.stride(0), M, Cn, labels_dev.data_ptr(), IGNORE_INDEX, rows.data_ptr(), L.VK_F32,
           stream(dev))
    L.call("vk_loss_reduce", rows.data_ptr(), None, labels_dev.data_ptr(), IGNORE_INDEX, M, 1.0, loss.data_ptr(), stream(dev))
    return loss, cross_entropy_grad(logits, labels_dev, 1.0 / counted)


class _Trainer:
    """What `HeadTrainer` and `EncoderTrainer` (finetune.py) share: fp32 masters `p`, gradients `g` and AdamW's `m`, `v` by key, the
    table `vk_adamw_step` reads, the hyper-parameters and the schedule, the label check, the closing optimiser step, `grads()`,
    `state_dict()` and `commit()`'s repacking.  A subclass names its keys, builds its masters and owns its step."""

    def _need_gpu(self):
        if not torch.cuda.is_available():
            raise RuntimeError(f"vltk_amd.{type(self).__name__} needs a GPU: there is no CPU fallback")

    def _hold(self, keys, p, g, lr, betas, eps, weight_decay, no_decay, schedule):
        """`p`: the masters by key, on the device; `g`: their gradient buffers, or None for zeros of their own.  `keys` orders
        the table, `grads()` and `state_dict()`; the last key is the head's bias."""
        self.keys, self.p = tuple(keys), p
        self.g = {k: torch.zeros_like(p[k]) for k in self.keys} if g is None else g
        self.m, self.v = ({k: torch.zeros_like(p[k]) for k in self.keys} for _ in range(2))
        self.base_lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.schedule = schedule
        self.steps = 0                               # optimiser steps taken
        self.num_classes = p[self.keys[-1]].numel()
        self._table, self._max_n = adamw_table([(p[k], self.g[k], self.m[k], self.v[k], not any(f in k for f in no_decay))
                                                for k in self.keys], self.device)

    @property
    def lr(self):
        """The rate of the next step."""
        return self.base_lr if self.schedule is None else self.schedule(self.base_lr, self.steps)

    def _check_labels(self, labels, B):
        """Host-side, before any launch -> (int64 numpy labels, the rows that count)."""
        lab = check_class_labels("labels", labels, (B,), self.num_classes)
        counted = int((lab != IGNORE_INDEX).sum())
        if counted == 0:
            raise ValueError(f"labels: every label is {IGNORE_INDEX}, so no row counts and the mean loss is undefined")
        return lab, counted

    def _adamw(self):
        """One AdamW step over every held tensor at the schedule's rate; the schedule advances."""
        adamw_step(self._table, len(self.keys), self._max_n, self.lr, self.betas, self.eps, self.weight_decay, self.steps + 1, self.device)
        self.steps += 1

    def grads(self):
        """The last step's gradients by key (after clipping where the trainer clips, as `.grad` is in torch), fp32 numpy arrays."""
        return {k: self.g[k].cpu().numpy() for k in self.keys}

    def state_dict(self):
        """The trained tensors by transformers' key names, fp32 numpy arrays."""
        return {k: self.p[k].cpu().numpy() for k in self.keys}

    def _commit(self, lins, lns, head_keys):
        """Repack the masters into the model's packed buffers (host-side, the loaders' `pack`), in place with `copy_`, so that a
        captured graph stays valid.  `lins`: (the name in `enc._lin`, the state-dict prefixes whose weights and biases it
        concatenates, in the loader's order); `lns`: (the name in `enc._ln`, the state-dict prefix); `head_keys`: the tensors
        `enc._head` keeps on the host.  -> the model."""
        enc, sd = self.enc, self.state_dict()
        for name, *parts in lins:
            w, b = (np.concatenate([sd[f"{q}.{t}"] for q in parts], 0) for t in ("weight", "bias"))
            wp, bp, _, _ = enc._pack(w, b)
            enc._lin[name][0].copy_(wp)
            enc._lin[name][1].copy_(bp)
        for name, key in lns:
            for t, part in zip(enc._ln[name], ("weight", "bias")):
                t.copy_(torch.from_numpy(sd[f"{key}.{part}"]))
        for k in head_keys:
            enc._head[k] = sd[k].copy()
        torch.cuda.synchronize(self.device)
        return self.model


# ---- the heads ---------------------------------------------------------------------------------------------------------------------------
LXMERT_HEAD = tuple(f"answer_head.logit_fc.{i}.{t}" for i in (0, 2, 3) for t in ("weight", "bias"))


def _describe(model):
    """-> (encoder, state-dict prefix of a single-Linear head, or None for LXMERT's answer head)."""
    from .layoutlm import LayoutLMForSequenceClassification
    from .lxmert import LxmertForQuestionAnswering
    from .visualbert import VisualBertForQuestionAnswering
    from .vit import ViTForImageClassification
    if isinstance(model, LxmertForQuestionAnswering):
        return model.lxmert, None
    if isinstance(model, VisualBertForQuestionAnswering):
        return model.visual_bert, "cls"
    if isinstance(model, ViTForImageClassification):
        return model.vit, "classifier"
    if isinstance(model, LayoutLMForSequenceClassification):
        return model.layoutlm, "classifier"
    raise TypeError(f"HeadTrainer takes LxmertForQuestionAnswering, VisualBertForQuestionAnswering, ViTForImageClassification or "
                    f"LayoutLMForSequenceClassification, not {type(model).__name__}")


class HeadTrainer(_Trainer):
    """`HeadTrainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(), schedule=None)`: trains the head
    of `LxmertForQuestionAnswering` (Linear -> GELU -> LayerNorm -> Linear), `VisualBertForQuestionAnswering` (`cls`),
    `ViTForImageClassification` or `LayoutLMForSequenceClassification` (`classifier`) with cross-entropy and `torch.optim.AdamW`'s
    rule, the encoder frozen.  Any other model: TypeError.

    The trainer holds fp32 masters of the head's tensors, their gradients and AdamW's `m` and `v` under transformers' key names,
    initialised from the state dict the model was loaded with.  `no_decay`: name fragments (e.g. `("bias", "logit_fc.2")`) whose
    tensors take no weight decay; the default decays every tensor, as `AdamW(model.parameters())` in the reference's script.
    `schedule`: `step_lr(..)`, `linear_warmup(..)` or None for a constant rate.

    The model keeps answering with the head it was loaded with until `commit()`."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, no_decay=(), schedule=None):
        self._need_gpu()
        self.enc, self.prefix = _describe(model)
        self.model = model
        enc = self.enc
        keys = LXMERT_HEAD if self.prefix is None else (self.prefix + ".weight", self.prefix + ".bias")
        missing = [k for k in keys if k not in getattr(enc, "_head", {})]
        if missing:
            raise RuntimeError(f"{type(model).__name__}: load_state_dict() first (no head tensor {missing[0]})")
        dev = self.device = enc.device
        self._hold(keys, {k: torch.from_numpy(enc._head[k]).to(dev) for k in keys}, None, lr, betas, eps, weight_decay, no_decay, schedule)
        self.ln_eps = enc.cfg.get("layer_norm_eps", LN_EPS)

    # ---- one step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _step(self, x, lab, counted):
        dev, p, g = self.device, self.p, self.g
        labels = torch.from_numpy(lab).to(dev)
        x = x.to(dev, torch.float32).contiguous()
        if self.prefix is None:
            w0, b0, gam, bet, w3, b3 = (p[k] for k in self.keys)
            z = gemm_f32(x, w0, b0, trans_b=True)                      # the pre-activation, kept for the backward
            a = act_f32(z, L.VK_ACT_GELU)
            h = layernorm_f32(a, gam, bet, self.ln_eps)
            logits = gemm_f32(h, w3, b3, trans_b=True)
        else:
            w3, b3 = (p[k] for k in self.keys)
            h = x
            logits = gemm_f32(h, w3, b3, trans_b=True)
        loss, dlogits = loss_and_grad(logits, labels, counted)
        # backward
        dh = linear_backward(dlogits, h, w3, g[self.keys[-2]], g[self.keys[-1]], need_dx=self.prefix is None)
        if self.prefix is None:
            da, _, _ = layernorm_grad(a, gam, dh, self.ln_eps, dgamma=g[self.keys[2]], dbeta=g[self.keys[3]])
            dz = act_grad_f32(z, da, L.VK_ACT_GELU)
            linear_backward(dz, x, w0, g[self.keys[0]], g[self.keys[1]], need_dx=False)
        self._adamw()
        return loss

    def step_features(self, feats, labels):
        """One training step on what the head consumes: `feats [B, H]` (the pooled output, the gathered row or the class token;
        any float type, cast to fp32), `labels [B]` (a class each, -100 to leave a row out).  Forward, cross-entropy, backward, one
        AdamW step; the schedule advances.  -> the loss before the step, an fp32 device scalar.  Labels are checked on the host
        before any launch: a wrong shape or type, or labels that are all -100, ValueError; a label outside the classes IndexError."""
        if feats.dim() != 2 or feats.shape[1] != self.p[self.keys[0]].shape[1] or not feats.is_floating_point():
            raise ValueError(f"feats must be a float [B, {self.p[self.keys[0]].shape[1]}] tensor, got {feats.dtype} {tuple(feats.shape)}")
        lab, counted = self._check_labels(labels, feats.shape[0])
        loss = self._step(feats, lab, counted)
        torch.cuda.synchronize(self.device)
        return loss

    def step(self, *model_inputs, labels, **options):
        """The frozen encoder's forward on `model_inputs` (the model's own arguments; `model.head_features`), then
        `step_features` on its output."""
        B = model_inputs[0].shape[0]
        lab, counted = self._check_labels(labels, B)                   # before the encoder launches anything
        feats = self.model.head_features(*model_inputs, **options)
        loss = self._step(feats, lab, counted)
        torch.cuda.synchronize(self.device)
        return loss

    def commit(self):
        """Repack the masters into the model's packed head weights (host-side, the loaders' `pack`), in place: after it `model(...)`
        answers with the trained head.  No encoder tensor is written."""
        if self.prefix is None:
            lins = (("answer.fc0", "answer_head.logit_fc.0"), ("answer.fc3", "answer_head.logit_fc.3"))
            return self._commit(lins, (("answer_head.logit_fc.2", "answer_head.logit_fc.2"),), self.keys)
        return self._commit(((self.prefix, self.prefix),), (), self.keys)
