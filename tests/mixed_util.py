"""TEST INFRASTRUCTURE ONLY -- what the tests of the mixed-precision fine-tuning mode share (`vk_cast_16`, `vk_gemm_16`,
`vk_attention_grad_16`, `EncoderTrainer(compute_dtype=torch.bfloat16)`): 16-bit rounding on the host, the per-element bounds of the
16-bit attention backward, and the yardstick, a torch restatement of the trained layers on the CPU in float64 with custom autograd
functions that round where the mode rounds.  Nothing here touches a GPU, and nothing here is the code under test.

The per-element bounds of `vk_attention_grad_16` extend the derivation at the head of tests/finetune_util.py (read that first) by the
rounding points at the head of csrc/attention_grad16.hip.  u = 2^-24, u16 = the unit roundoff of the 16-bit type (2^-8 for bf16, 2^-11 for
fp16: half its epsilon), t16 = half its smallest subnormal (2^-134 / 2^-25: the absolute error of a rounding below the normal range).  The inputs are
16-bit values, so every product q k, dO v, dO o, dS k, P dO is exact in fp32 and only the sums round.  First order, then a factor
(1 + 2^-6) for the second order: each first-order relative error is a few u16 <= 2^-6 at most, and they multiply in pairs.  Per (batch, head), row r, keys j:

  s_j      the instruction's sum of d exact products, then fmaf(s, scale, mask): es_j = (d + 1) u scale sum_c |q_c k_jc| + u |s_j|;
           0 for an absorbing mask.
  a_j, e_j = s_j - m rounded, times log2(e) rounded, v_exp_f32 (1 ulp): r_j = es_j + es_jmax + 3 u |a_j| + 3 u
  l, p_j   as the fp32 kernel: rp_j = r_j + rbar + (8 + 5 T) u, T = ceil(Lk / 64) tiles, is the relative error of the fp32 p_j
  D        from the O the kernel is GIVEN (a 16-bit tensor): eD = |sum_c dO_c (O_given - O_ref)_c| + (d / 4 + 2) u sum_c |dO_c O_c|.
           The first term is computed, and it leads: O_given is a 16-bit rounding.
  dP_j     eP_j = d u sum_c |dO_c v_jc|
  dS_j     = p_j (dP_j - D) in fp32, then ONE ROUNDING TO 16 BITS:  with x_j = dP_j - D,
           eS_j = p_j (eP_j + eD + u |x_j|) + (rp_j + u) p_j |x_j| + u16 |dS_j| + t16
  dQ_c     = scale sum_j dS16_j k_jc:  scale (sum_j eS_j |k_jc| + (Lk / 32 + 1) u sum_j |dS_j k_jc|) + u |dQ_c|
  dK_jc    the same over the queries
  dV_jc    = sum_r P16_rj dO_rc, P16 the 16-bit rounding of p:  sum_r ((rp_rj + u16) p_rj + t16) |dO_rc| + (Lq / 32 + 1) u sum_r |p_rj dO_rc|
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import finetune_util as U

U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}              # unit roundoff
EPS16 = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}            # torch.finfo(dtype).eps
T16 = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def round16(a, dtype):
    """numpy (any float type) -> the values rounded to `dtype` by torch's CPU cast from fp32, as float64."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype).double().numpy()


def bits16(a, dtype):
    """numpy -> the uint16 bit patterns of the values rounded to `dtype` (torch's CPU cast from fp32)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype).view(torch.int16).numpy().view(np.uint16)


def from_bits16(b, dtype):
    """uint16 bit patterns -> float64 values."""
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(dtype).double().numpy()


def is16(a, dtype):
    """Whether every value of `a` is a number of `dtype`."""
    a = np.asarray(a, np.float64)
    return bool((round16(a, dtype) == a).all()) and bool((a.astype(np.float32).astype(np.float64) == a).all())


# ---- the attention backward ------------------------------------------------------------------------------------------------------------
def attention_grad16_reference(q, k, v, mask, dout, heads, dtype, o_given=None, scale=None):
    """The float64 reference of tests/finetune_util.py on 16-bit inputs (float64 arrays holding numbers of `dtype`), with the
    bounds of this module's docstring.  `o_given`: the 16-bit O the kernel receives (default: the reference's, rounded to `dtype`)."""
    B, Lq, H = q.shape
    Lk, d = k.shape[1], H // heads
    if o_given is None:
        o_given = round16(U.attention_grad_reference(q, k, v, mask, dout, heads, scale=scale)["o"], dtype)
    ref = U.attention_grad_reference(q, k, v, mask, dout, heads, o_given=o_given, scale=scale)
    t = ref["terms"]
    p, dS, x, kh, qh, vh, doh, og = (t[n] for n in ("p", "dS", "x", "kh", "qh", "vh", "doh", "og"))
    sc = 1.0 / math.sqrt(d) if scale is None else float(scale)
    split = lambda w: w.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)
    join = lambda w: w.transpose(0, 2, 1, 3).reshape(B, -1, H)
    tr = lambda w: w.transpose(0, 1, 3, 2)
    o = split(ref["o"])
    mk = np.zeros((B, Lk)) if mask is None else np.asarray(mask, np.float64)
    absorbed = (mk < -1e30)[:, None, None, :]
    s = np.where(absorbed, mk[:, None, None, :], qh @ tr(kh) * sc + mk[:, None, None, :])
    a = s - s.max(-1, keepdims=True)
    u, u16, t16, T = U.U32, U16[dtype], T16[dtype], -(-Lk // 64)
    es = np.where(absorbed, 0.0, (d + 1) * u * sc * (np.abs(qh) @ tr(np.abs(kh))) + u * np.abs(s))
    es_max = np.take_along_axis(es, s.argmax(-1)[..., None], -1)
    r = es + es_max + 3 * u * np.abs(a) + 3 * u
    rp = r + (p * r).sum(-1, keepdims=True) + (8 + 5 * T) * u
    eD = np.abs((doh * (og - o)).sum(-1, keepdims=True)) + (d / 4 + 2) * u * (np.abs(doh) * np.abs(og)).sum(-1, keepdims=True)
    eP = d * u * (np.abs(doh) @ tr(np.abs(vh)))
    eS = p * (eP + eD + u * np.abs(x)) + (rp + u) * p * np.abs(x) + u16 * np.abs(dS) + t16
    second, tiny = 1 + 2.0 ** -6, 2.0 ** -149
    b_dq = (sc * (eS @ np.abs(kh) + (Lk / 32 + 1) * u * (np.abs(dS) @ np.abs(kh))) + u * np.abs(split(ref["dq"]))) * second + Lk * 2.0 ** -126 + tiny
    b_dk = (sc * (tr(eS) @ np.abs(qh) + (Lq / 32 + 1) * u * (tr(np.abs(dS)) @ np.abs(qh))) + u * np.abs(split(ref["dk"]))) * second + Lq * 2.0 ** -126 + tiny
    b_dv = (tr((rp + u16) * p + t16) @ np.abs(doh) + (Lq / 32 + 1) * u * (tr(p) @ np.abs(doh))) * second + Lq * 2.0 ** -126 + tiny
    return dict(ref, o_given=np.asarray(o_given, np.float64), b_dq=join(b_dq), b_dk=join(b_dk), b_dv=join(b_dv))


def exact_in_16(ref, dtype, inputs):
    """Whether an exact case's data is exact for the 16-bit kernel whatever the order of its sums: the inputs, the O it is given, P
    and dS are numbers of `dtype` (so the two roundings of the kernel change nothing), and `exact_in_fp32` holds (every fp32
    intermediate is an fp32 number and every sum stays below 2^24 grains)."""
    t = ref["terms"]
    return (all(is16(a, dtype) for a in inputs) and is16(t["og"], dtype) and is16(t["p"], dtype) and is16(t["dS"], dtype)
            and U.exact_in_fp32(ref))


# ---- the yardstick: the trained layers in float64 with the mode's roundings ------------------------------------------------------------
def _r(t, dtype):
    return t.to(torch.float32).to(dtype).to(torch.float64)


class Linear16(torch.autograd.Function):
    """y = r(x) r(W)^T + b with fp64 sums (`vk_gemm_16` behind `vk_cast_16`); y rounded where the mode writes it in 16 bits.
    Backward: dY is rounded once and feeds both products; dX is rounded where the mode writes it in 16 bits; db sums the
    unrounded dY (`vk_col_sums` of the fp32 gradient)."""

    @staticmethod
    def forward(ctx, x, w, b, dtype, round_y, round_dx):
        x16, w16 = _r(x, dtype), _r(w, dtype)
        ctx.save_for_backward(x16, w16)
        ctx.cfg = (dtype, round_dx)
        y = x16 @ w16.T + b
        return _r(y, dtype) if round_y else y

    @staticmethod
    def backward(ctx, dy):
        x16, w16 = ctx.saved_tensors
        dtype, round_dx = ctx.cfg
        dy16 = _r(dy, dtype)
        dx = dy16 @ w16
        dw = dy16.reshape(-1, dy16.shape[-1]).T @ x16.reshape(-1, x16.shape[-1])
        return (_r(dx, dtype) if round_dx else dx), dw, dy.reshape(-1, dy.shape[-1]).sum(0), None, None, None


class Attention16(torch.autograd.Function):
    """The attention pair of the mode on 16-bit q, k, v [B, L, H]: forward O = r(r(P) V) (`vk_attention_tiled` rounds the
    probabilities before the second product, and its output); backward from the kept 16-bit O and a 16-bit dO:
    dV = r(P)^T dO, D = sum_c dO O, dS = P (dO V^T - D) rounded, dQ = scale r(dS) K, dK = scale r(dS)^T Q."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, dtype):
        B, Lq, H = q.shape
        d = H // heads
        qh, kh, vh = (t.view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
        if mask is not None:
            s = s + mask[:, None, None, :]
        p = torch.softmax(s, -1)
        o = _r(_r(p, dtype) @ vh, dtype)
        ctx.save_for_backward(qh, kh, vh, p, o)
        ctx.cfg = (dtype, d, (B, Lq, H))
        return o.transpose(1, 2).reshape(B, Lq, H)

    @staticmethod
    def backward(ctx, do):
        qh, kh, vh, p, o = ctx.saved_tensors
        dtype, d, (B, Lq, H) = ctx.cfg
        doh = _r(do, dtype).view(B, Lq, -1, d).transpose(1, 2)
        dv = _r(p, dtype).transpose(-1, -2) @ doh
        D = (doh * o).sum(-1, keepdim=True)
        ds = _r(p * (doh @ vh.transpose(-1, -2) - D), dtype)
        scale = 1.0 / math.sqrt(d)
        dq, dk = ds @ kh * scale, ds.transpose(-1, -2) @ qh * scale
        back = lambda t: t.transpose(1, 2).reshape(B, -1, H)
        return back(dq), back(dk), back(dv), None, None, None


def bert_layer_16(p, P, x, mask, heads, eps, dtype, taps=None):
    """`finetune_util.bert_layer` with the mode's roundings: every linear is `Linear16` (the QKV projection writes 16 bits, the
    attention output projection's dX is written in 16 bits), attention is `Attention16`; LayerNorm, GELU, residuals in float64."""
    H = x.shape[-1]
    a = P + ".attention.self."
    q, k, v = (Linear16.apply(x, p[a + t + ".weight"], p[a + t + ".bias"], dtype, True, False) for t in ("query", "key", "value"))
    if taps is not None:
        k.retain_grad()
        taps.append(k)
    ctx = Attention16.apply(q, k, v, mask, heads, dtype)
    o = P + ".attention.output."
    h1 = F.layer_norm(Linear16.apply(ctx, p[o + "dense.weight"], p[o + "dense.bias"], dtype, False, True) + x, (H,), p[o + "LayerNorm.weight"],
                      p[o + "LayerNorm.bias"], eps)
    i, o = P + ".intermediate.dense.", P + ".output."
    z = F.gelu(Linear16.apply(h1, p[i + "weight"], p[i + "bias"], dtype, False, False))
    return F.layer_norm(Linear16.apply(z, p[o + "dense.weight"], p[o + "dense.bias"], dtype, False, False) + h1, (H,), p[o + "LayerNorm.weight"],
                        p[o + "LayerNorm.bias"], eps)


def tail_logits_16(p, x, mask, layers, heads, eps, kind, rows, enc_prefix, dtype, taps=None):
    """`finetune_util.tail_logits` with the layers in the mode's arithmetic and the head as it is (fp32 in the mode: float64 here)."""
    for P in layers:
        x = bert_layer_16(p, P, x, mask, heads, eps, dtype, taps)
    return U.head_logits(p, x, kind, rows, enc_prefix)


def finetune_run(sd, keys, x0, mask01, labels, steps, layers, heads, eps, kind, rows=None, enc_prefix="", lr=1e-3, betas=(0.9, 0.999),
                 adam_eps=1e-8, weight_decay=0.01, step_lr=None, max_norm=None, compute_dtype=None):
    """`finetune_util.torch_finetune_run` in float64 with torch's own AdamW, clipping and StepLR: compute_dtype None is the
    pure-fp64 run, torch.bfloat16 the yardstick (the mode's roundings, everything else in fp64).  The same dict."""
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=torch.float64, requires_grad=True) for k in keys}
    x = torch.tensor(np.asarray(x0, np.float32)).double()
    mask = U.additive(mask01, torch.float64)
    y = torch.tensor(np.asarray(labels, np.int64))
    rows_t = None if rows is None else torch.as_tensor(np.asarray(rows, np.int64))
    opt = torch.optim.AdamW([p[k] for k in keys], lr=lr, betas=betas, eps=adam_eps, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.StepLR(opt, *step_lr) if step_lr else None
    out = dict(losses=[], norms=[], dk=[], keybias=[], first=None)
    for _ in range(steps):
        opt.zero_grad()
        taps = []
        if compute_dtype is None:
            logits = U.tail_logits(p, x, mask, layers, heads, eps, kind, rows_t, enc_prefix, taps)
        else:
            logits = tail_logits_16(p, x, mask, layers, heads, eps, kind, rows_t, enc_prefix, compute_dtype, taps)
        loss = F.cross_entropy(logits, y, ignore_index=U.IGNORE_INDEX)
        loss.backward()
        if max_norm is not None:
            out["norms"].append(float(torch.nn.utils.clip_grad_norm_([p[k] for k in keys], max_norm).double()))
        out["dk"].append([t.grad.detach().double().abs().sum((0, 1)).numpy() for t in taps])
        out["keybias"].append({k: p[k].grad.detach().double().numpy().copy() for k in keys if k.endswith("key.bias")})
        if out["first"] is None:
            out["first"] = {k: p[k].grad.detach().double().numpy().copy() for k in keys}
        opt.step()
        if sched:
            sched.step()
        out["losses"].append(float(loss.detach().double()))
    out["losses"] = np.array(out["losses"])
    out["tensors"] = {k: p[k].detach().double().numpy() for k in keys}
    return out


def fixture_run(n, steps, x0, compute_dtype, wide=False, long=False, max_norm=None, base=False):
    """`finetune_run` on the trajectory fixture (wide: hidden 128, 4 heads of d = 32; long: 2 heads of d = 64, 140 rows; base:
    BERT-base width, 12 heads of d = 64, 896 rows) with the last n layers trained, from the boundary state x0."""
    cfg, sd, inputs, labels = U.trajectory_fixture(wide=wide, long=long, base=base)
    nl = cfg["num_hidden_layers"]
    layers = [f"visual_bert.encoder.layer.{i}" for i in range(nl - n, nl)]
    keys = U.trained_keys("visual_bert.", range(nl - n, nl), "cls")
    rows = inputs["attention_mask"].sum(1) - 2
    mask01 = np.concatenate((inputs["attention_mask"], inputs["visual_attention_mask"]), 1)
    return keys, finetune_run(sd, keys, x0, mask01, labels, steps, layers, cfg["num_attention_heads"], cfg["layer_norm_eps"], "cls", rows,
                              "visual_bert.", lr=U.FIXTURE_LR, step_lr=U.FIXTURE_STEP_LR, max_norm=max_norm, compute_dtype=compute_dtype)
