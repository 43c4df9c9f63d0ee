"""N7: train an answer head over a frozen encoder.  The reference's only training loop, `vltk/legacy/legacy_train.py`, fine-tunes
a QA model on the extractor's features: cross-entropy on `question_answering_score`, `AdamW(params, 1e-4)`, `StepLR(200, 0.9)`,
and a linear warm-up kept beside it.  `HeadTrainer` is the slice of that loop practitioners run first on extracted features: the
encoder frozen (its existing forward), its head trained in fp32.

Forward, loss, backward and the optimiser step are the kernels of csrc/train.hip (`vk_gemm_f32` in its three transposition forms,
`vk_act_f32`, `vk_col_sums`, `vk_cross_entropy_grad`, `vk_act_grad_f32`, `vk_layernorm_grad`, `vk_adamw_step`) with `vk_layernorm`,
`vk_cross_entropy` and `vk_loss_reduce` in fp32.  All arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No
CPU fallback.

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


class HeadTrainer:
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
        if not torch.cuda.is_available():
            raise RuntimeError("vltk_amd.HeadTrainer needs a GPU: there is no CPU fallback")
        self.enc, self.prefix = _describe(model)
        self.model = model
        enc = self.enc
        self.keys = LXMERT_HEAD if self.prefix is None else (self.prefix + ".weight", self.prefix + ".bias")
        missing = [k for k in self.keys if k not in getattr(enc, "_head", {})]
        if missing:
            raise RuntimeError(f"{type(model).__name__}: load_state_dict() first (no head tensor {missing[0]})")
        dev = self.device = enc.device
        self.p = {k: torch.from_numpy(enc._head[k]).to(dev) for k in self.keys}
        self.g, self.m, self.v = ({k: torch.zeros_like(t) for k, t in self.p.items()} for _ in range(3))
        self.base_lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.schedule = schedule
        self.steps = 0                               # optimiser steps taken
        self.num_classes = self.p[self.keys[-1]].numel()
        self.ln_eps = enc.cfg.get("layer_norm_eps", LN_EPS)
        self._table, self._max_n = adamw_table([(self.p[k], self.g[k], self.m[k], self.v[k], not any(f in k for f in no_decay))
                                                for k in self.keys], dev)

    @property
    def lr(self):
        """The rate of the next step."""
        return self.base_lr if self.schedule is None else self.schedule(self.base_lr, self.steps)

    # ---- one step ---------------------------------------------------------------------------------------------------------------
    def _check_labels(self, labels, B):
        """Host-side, before any launch -> (int64 numpy labels, the rows that count)."""
        lab = check_class_labels("labels", labels, (B,), self.num_classes)
        counted = int((lab != IGNORE_INDEX).sum())
        if counted == 0:
            raise ValueError(f"labels: every label is {IGNORE_INDEX}, so no row counts and the mean loss is undefined")
        return lab, counted

    @torch.no_grad()
    def _step(self, x, lab, counted):
        dev, p, g = self.device, self.p, self.g
        labels = torch.from_numpy(lab).to(dev)
        x = x.to(dev, torch.float32).contiguous()
        B = x.shape[0]
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
        rows = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L.call("vk_cross_entropy", logits.data_ptr(), logits.stride(0), B, self.num_classes, labels.data_ptr(), IGNORE_INDEX, rows.data_ptr(),
               L.VK_F32, stream(dev))
        L.call("vk_loss_reduce", rows.data_ptr(), None, labels.data_ptr(), IGNORE_INDEX, B, 1.0, loss.data_ptr(), stream(dev))
        # backward
        dlogits = cross_entropy_grad(logits, labels, 1.0 / counted)
        kw, kb = self.keys[-2], self.keys[-1]
        gemm_f32(dlogits, h, out=g[kw], trans_a=True)                  # dW = dY^T . X
        col_sums(dlogits, out=g[kb])
        if self.prefix is None:
            dh = gemm_f32(dlogits, w3)                                 # dX = dY . W
            da, _, _ = layernorm_grad(a, gam, dh, self.ln_eps, dgamma=g[self.keys[2]], dbeta=g[self.keys[3]])
            dz = act_grad_f32(z, da, L.VK_ACT_GELU)
            gemm_f32(dz, x, out=g[self.keys[0]], trans_a=True)
            col_sums(dz, out=g[self.keys[1]])
        adamw_step(self._table, len(self.keys), self._max_n, self.lr, self.betas, self.eps, self.weight_decay, self.steps + 1, dev)
        self.steps += 1
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

    # ---- what it holds ---------------------------------------------------------------------------------------------------------------
    def grads(self):
        """The last step's gradients by key, fp32 numpy arrays."""
        return {k: t.cpu().numpy() for k, t in self.g.items()}

    def state_dict(self):
        """The head's tensors by transformers' key names, fp32 numpy arrays."""
        return {k: t.cpu().numpy() for k, t in self.p.items()}

    def commit(self):
        """Repack the masters into the model's packed head weights (host-side, the loaders' `pack`), in place: after it `model(...)`
        answers with the trained head.  No encoder tensor is written."""
        enc, sd = self.enc, self.state_dict()
        if self.prefix is None:
            lins, lns = (("answer.fc0", "answer_head.logit_fc.0"), ("answer.fc3", "answer_head.logit_fc.3")), ("answer_head.logit_fc.2",)
        else:
            lins, lns = ((self.prefix, self.prefix),), ()
        for name, key in lins:
            w, b, _, _ = enc._pack(sd[key + ".weight"], sd[key + ".bias"])
            enc._lin[name][0].copy_(w)
            enc._lin[name][1].copy_(b)
        for key in lns:
            for t, part in zip(enc._ln[key], ("weight", "bias")):
                t.copy_(torch.from_numpy(sd[f"{key}.{part}"]))
        for k in self.keys:
            enc._head[k] = sd[k].copy()
        torch.cuda.synchronize(self.device)
        return self.model
