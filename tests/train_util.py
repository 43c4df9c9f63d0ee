"""TEST INFRASTRUCTURE ONLY -- float64 restatements of what csrc/train.hip and vltk_amd/train.py compute, and the per-element bounds
derived from the kernels' rounding points (the comment at the head of csrc/train.hip).  Nothing here touches a GPU.

u = 2^-24 (half an ulp of fp32, relative), w = 2^-50 (eight ulps of fp64: the allowance for fp64 arithmetic and the device library's
erfc / exp / cosh / sqrt, which the kernels that compute in fp64 spend before their one rounding to fp32).

gemm, real data      one fmaf chain of K terms per element: |out - ref| <= K u sum_k |a_k b_k| (each partial sum is bounded by the
                     sum of the sizes; one rounding per step).
ce_grad              a_j = x_j - max is rounded (u |a_j|), expf is good to an ulp (2 u): e_j is off by r_j = u |a_j| + 2 u relative;
                     the fp64 sum s by the p-weighted mean rbar of the r_j; p_j = fl(e_j / s) by r_j + rbar + u; p_j - onehot and
                     the product with scale are rounded once each:
                         |out - ref| <= scale (p_j (r_j + rbar + u) + 2 u |p_j - y_j|) (1 + 2^-10) + scale 2^-126 + 2^-149
                     (an exponential below the normal range may be flushed; the result may be subnormal).  A counted row's true sum
                     is zero, so the row's sum is bounded by the sum of its elements' bounds.
act, act_grad        fp64, one rounding: u |ref| + w (|x| + 1) |dy| + 2^-149.
layernorm_grad       fp64, one rounding.  dx = rstd (g - s1 - xh s2): u |ref| + (C + 8) w rstd (|g| + |s1| + |xh s2| +
                     rstd max|x| (|s2| + |s1| + |g|)); the last term is the mean's own fp64 error reaching xh.  dgamma, dbeta:
                     u |ref| + (M + C + 8) w sum_m |dy xh| (or |dy|).
adamw                fp64, one rounding each: u |ref| + w (|p| + |update|) for p, u |ref| (1 + 2^-20) + 2^-149 for m and v.

torch's LayerNorm backward on a constant row (float64): the mean is exact, xhat = 0, rstd = 1 / sqrt(eps), and
dx = (g - mean(g)) / sqrt(eps) with g = dy * gamma: 10^6 times the centred gradient at eps = 1e-12.  The kernel's fp64 row sum of
C equal floats is exact too, so it gives the same.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
W64 = 2.0 ** -50
IGNORE_INDEX = -100
LXMERT_KEYS = tuple(f"answer_head.logit_fc.{i}.{t}" for i in (0, 2, 3) for t in ("weight", "bias"))


def maxnorm_rel(a, ref):
    """max |a - ref| / max |ref| in float64 (0 / 0 counts as 0)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    d, n = np.abs(a - ref).max(), np.abs(ref).max()
    return 0.0 if d == 0 else d / n


# ---- the schedules and the rule --------------------------------------------------------------------------------------------------
def adamw_f64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decay=True):
    """torch.optim.AdamW's step, written out, in float64 -> (p, m, v, update)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    upd = (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    if decay:
        p = p * (1 - lr * weight_decay)
    return p - upd, m, v, upd


def adamw_bounds(p_in, p_ref, m_ref, v_ref, upd):
    tiny = 2.0 ** -149
    return (U32 * np.abs(p_ref) + W64 * (np.abs(p_in) + np.abs(upd)) + tiny, U32 * np.abs(m_ref) * (1 + 2.0 ** -20) + tiny,
            U32 * np.abs(v_ref) * (1 + 2.0 ** -20) + tiny)


# ---- kernels in float64 -------------------------------------------------------------------------------------------------------------
def gemm_reference(A, B, transA, transB, bias=None, C0=None):
    """-> (float64 product, sum_k |a_k b_k| per element) of the stored operands."""
    a = np.asarray(A, np.float64).T if transA else np.asarray(A, np.float64)
    b = np.asarray(B, np.float64).T if transB else np.asarray(B, np.float64)
    ref = a @ b
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)[None]
    if C0 is not None:
        ref = ref + np.asarray(C0, np.float64)
    return ref, np.abs(a) @ np.abs(b)


def ce_grad_reference(x, labels, scale):
    """-> (float64 dlogits, its per-element bound); ignored rows are zero with a zero bound."""
    x, labels = np.asarray(x, np.float64), np.asarray(labels).reshape(-1)
    a = x - x.max(1, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(1, keepdims=True)
    keep = labels != IGNORE_INDEX
    y = np.zeros_like(p)
    y[np.flatnonzero(keep), labels[keep]] = 1.0
    r = U32 * np.abs(a) + 2 * U32
    rbar = (p * r).sum(1, keepdims=True)
    bound = scale * (p * (r + rbar + U32) + 2 * U32 * np.abs(p - y)) * (1 + 2.0 ** -10) + scale * 2.0 ** -126 + 2.0 ** -149
    return np.where(keep[:, None], (p - y) * scale, 0.0), np.where(keep[:, None], bound, 0.0)


def act_reference(x, act):
    x = torch.as_tensor(np.asarray(x, np.float64))
    if act == "gelu":
        return (x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))).numpy()
    return torch.tanh(x).numpy()


def act_grad_reference(x, dy, act):
    """-> (float64 dx, its bound)."""
    xt = torch.as_tensor(np.asarray(x, np.float64))
    if act == "gelu":
        d = 0.5 * torch.special.erfc(-xt / math.sqrt(2.0)) + xt * torch.exp(-0.5 * xt * xt) / math.sqrt(2.0 * math.pi)
    else:
        d = 1.0 / torch.cosh(xt) ** 2
    dy = np.asarray(dy, np.float64)
    ref = dy * d.numpy()
    return ref, U32 * np.abs(ref) + W64 * (np.abs(np.asarray(x, np.float64)) + 1) * np.abs(dy) + 2.0 ** -149


def layernorm_grad_reference(x, gamma, dy, eps):
    """float64 autograd through F.layer_norm -> dict(dx, dgamma, dbeta and the three bounds)."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    gt = torch.tensor(np.asarray(gamma, np.float64), requires_grad=True)
    bt = torch.zeros_like(gt, requires_grad=True)
    F.layer_norm(xt, (xt.shape[1],), gt, bt, eps).backward(torch.tensor(np.asarray(dy, np.float64)))
    x64, g64, dy64 = xt.detach().numpy(), gt.detach().numpy(), np.asarray(dy, np.float64)
    M, C = x64.shape
    mean = x64.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x64 - mean) ** 2).mean(1, keepdims=True) + eps)
    xh, g = (x64 - mean) * rstd, dy64 * g64[None]
    s1, s2 = g.mean(1, keepdims=True), (g * xh).mean(1, keepdims=True)
    dx, dgamma, dbeta = xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()
    amax = np.abs(x64).max(1, keepdims=True)
    b_dx = U32 * np.abs(dx) + (C + 8) * W64 * rstd * (np.abs(g) + np.abs(s1) + np.abs(xh * s2) + rstd * amax * (np.abs(s2) + np.abs(s1) + np.abs(g)))
    b_dg = U32 * np.abs(dgamma) + (M + C + 8) * W64 * (np.abs(dy64 * xh).sum(0) + (np.abs(dy64) * rstd * amax).sum(0)) + 2.0 ** -149
    b_db = U32 * np.abs(dbeta) + (M + C + 8) * W64 * np.abs(dy64).sum(0) + 2.0 ** -149
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, b_dx=b_dx + 2.0 ** -149, b_dgamma=b_dg, b_dbeta=b_db)


# ---- the heads and a training run, by torch on the CPU ---------------------------------------------------------------------------------
def head_logits(params, x, keys):
    """params: {key: tensor}; the LXMERT answer head (six keys) or one Linear (two keys)."""
    if len(keys) == 6:
        w0, b0, gam, bet, w3, b3 = (params[k] for k in keys)
        h = F.layer_norm(F.gelu(F.linear(x, w0, b0)), (w0.shape[0],), gam, bet, 1e-12)
        return F.linear(h, w3, b3)
    return F.linear(x, params[keys[0]], params[keys[1]])


def torch_run(sd, keys, feats, labels, steps, dtype, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, step_lr=None):
    """`steps` steps of the reference's loop on the CPU in `dtype`: CrossEntropyLoss, torch.optim.AdamW, StepLR(*step_lr).
    -> (losses [steps] float64, the tensors after the last step, the gradients of the FIRST step), numpy float64."""
    params = {k: torch.tensor(np.asarray(sd[k]), dtype=dtype, requires_grad=True) for k in keys}
    x = torch.tensor(np.asarray(feats, np.float32)).to(dtype)
    y = torch.tensor(np.asarray(labels, np.int64))
    opt = torch.optim.AdamW([params[k] for k in keys], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.StepLR(opt, *step_lr) if step_lr else None
    losses, first = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = F.cross_entropy(head_logits(params, x, keys), y, ignore_index=IGNORE_INDEX)
        loss.backward()
        if first is None:
            first = {k: params[k].grad.detach().double().numpy().copy() for k in keys}
        opt.step()
        if sched:
            sched.step()
        losses.append(float(loss.detach().double()))
    return np.array(losses), {k: params[k].detach().double().numpy() for k in keys}, first


def head_fixture(hidden=32, answers=16, batch=64, seed=0, kind="lxmert", prefix="cls"):
    """Seeded N(0, 0.02) weights (LayerNorm gamma around 1), N(0, 1) features, labels with every ninth -100.
    -> (keys, {key: fp32 array}, feats fp32 [batch, hidden], labels int64 [batch])."""
    r = np.random.Generator(np.random.PCG64(seed))
    n = lambda *s: (r.standard_normal(s) * 0.02).astype(np.float32)
    if kind == "lxmert":
        keys = LXMERT_KEYS
        sd = dict(zip(keys, (n(2 * hidden, hidden), n(2 * hidden), 1 + n(2 * hidden), n(2 * hidden), n(answers, 2 * hidden), n(answers))))
    else:
        keys = (prefix + ".weight", prefix + ".bias")
        sd = dict(zip(keys, (n(answers, hidden), n(answers))))
    feats = r.standard_normal((batch, hidden)).astype(np.float32)
    labels = r.integers(0, answers, batch).astype(np.int64)
    labels[::9] = IGNORE_INDEX
    return keys, sd, feats, labels
