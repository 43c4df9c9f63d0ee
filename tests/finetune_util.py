"""TEST INFRASTRUCTURE ONLY -- what the tests of `vltk_amd.EncoderTrainer`, `vk_attention_grad`, `vk_scatter_rows_f32` and
`vk_grad_clip` share: a dtype-parametric, differentiable plain-torch restatement of the post-LN BERT layer, the two heads and the
gather / pooler in front of them; a float64 numpy reference of the attention backward with its per-element bounds; the
yardstick runner (the same steps in torch on the CPU); the clip rule; and the fixtures.  Nothing here touches a GPU.

The per-element bounds of `vk_attention_grad`, from the rounding points at the head of csrc/attention_grad.hip.  u = 2^-24; first
order, then a factor (1 + 2^-10) for the second order, as tests/train_util.py does it.  Per (batch, head) and query row r, keys j:

  s_j      one fmaf chain of d terms, then fmaf(s, scale, mask):  es_j = (d + 1) u scale sum_c |q_c k_jc| + u |s_j|.  A key whose
           additive mask is below -1e30 absorbs q . k in fp32 and in fp64 alike (both give the mask exactly): es_j = 0 there.
  a_j      = s_j - m, rounded: its absolute error ea_j = es_j + es_jmax + u |a_j| is the RELATIVE error of e_j = expf(a_j), which
           adds an ulp of its own: r_j = ea_j + 2 u.
  l        the sum of the e_j: their own errors weigh in as rbar = sum_j p_j r_j; the order (a 64-lane tree per tile, one
           fmaf(alpha, l, sum) per tile with alpha = expf(m_old - m_new), whose exponent's rounding counts at most u because
           x exp(-x) < 1) adds at most (6 + 5 T) u over T = ceil(Lk / 64) tiles; 1 / l and the product with e_j one u each:
           rp_j = r_j + rbar + (8 + 5 T) u is the relative error of p_j.
  D        the kernel forms sum_c dO_c O_c from the O it is GIVEN, in at most 2 chained fmaf per lane and a 6-level tree:
           eD = |sum_c dO_c (O_given - O_ref)_c| + 8 u sum_c |dO_c O_c|.  The first term is computed, not bounded: the tests pass
           O = fp32(reference O), so it is one rounding of the reference.
  dP_j     one fmaf chain:  eP_j = d u sum_c |dO_c v_jc|
  dS_j     = p_j (dP_j - D), two roundings:  eS_j = p_j (eP_j + eD + u |x_j|) + (rp_j + u) p_j |x_j|,  x_j = dP_j - D
  dQ_c     = scale sum_j dS_j k_jc, a chain of Lk terms and one product:
           scale (sum_j eS_j |k_jc| + Lk u sum_j |dS_j k_jc|) + u |dQ_c|
  dK_jc    the same over the queries r (chain of Lq);   dV_jc = sum_r p_rj dO_rc:  sum_r rp_rj p_rj |dO_rc| + Lq u sum_r |p_rj dO_rc|
and L 2^-126 + 2^-149 on each for results or terms below the normal range.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from train_util import IGNORE_INDEX, U32, maxnorm_rel          # noqa: F401

FMIN = float(torch.finfo(torch.float32).min)
AG_OWN, AG_STEP = 16, 64                                       # csrc/attention_grad.hip: rows a workgroup owns, rows it walks per tile


# ---- the layer, the heads, the gather / pooler: plain torch in the dtype of its arguments --------------------------------------------
def attention(q, k, v, mask, heads):
    """q, k, v [B, L, H]; mask additive [B, Lk] or None -> the context [B, Lq, H] (BertSelfAttention, no dropout)."""
    B, Lq, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        s = s + mask[:, None, None, :]
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, H)


def bert_layer(p, P, x, mask, heads, eps, taps=None):
    """The post-LN BERT layer of `BertOps._bert_layer` under state-dict prefix P.  `taps`: a list that receives the key
    projection's output with its gradient retained (the key.bias rule needs sum_m |dK[m, c]|)."""
    H = x.shape[-1]
    a = P + ".attention.self."
    q, k, v = (F.linear(x, p[a + t + ".weight"], p[a + t + ".bias"]) for t in ("query", "key", "value"))
    if taps is not None:
        k.retain_grad()
        taps.append(k)
    ctx = attention(q, k, v, mask, heads)
    o = P + ".attention.output."
    h1 = F.layer_norm(F.linear(ctx, p[o + "dense.weight"], p[o + "dense.bias"]) + x, (H,), p[o + "LayerNorm.weight"], p[o + "LayerNorm.bias"], eps)
    i, o = P + ".intermediate.dense.", P + ".output."
    z = F.gelu(F.linear(h1, p[i + "weight"], p[i + "bias"]))
    return F.layer_norm(F.linear(z, p[o + "dense.weight"], p[o + "dense.bias"]) + h1, (H,), p[o + "LayerNorm.weight"], p[o + "LayerNorm.bias"], eps)


def head_logits(p, x, kind, rows, enc_prefix):
    """x [B, L, H] -> logits.  kind "cls": `cls` on row rows[b] of each sequence (VisualBertForQuestionAnswering); "classifier":
    `classifier` on tanh(pooler.dense(first token)) (LayoutLMForSequenceClassification)."""
    if kind == "cls":
        return F.linear(x[torch.arange(x.shape[0]), rows], p["cls.weight"], p["cls.bias"])
    pooled = torch.tanh(F.linear(x[:, 0], p[enc_prefix + "pooler.dense.weight"], p[enc_prefix + "pooler.dense.bias"]))
    return F.linear(pooled, p["classifier.weight"], p["classifier.bias"])


def tail_logits(p, x, mask, layers, heads, eps, kind, rows, enc_prefix, taps=None):
    for P in layers:
        x = bert_layer(p, P, x, mask, heads, eps, taps)
    return head_logits(p, x, kind, rows, enc_prefix)


def additive(mask01, dtype):
    """[B, L] 1 / 0 -> (1 - m) * finfo(float32).min in `dtype`, or None."""
    return None if mask01 is None else ((1.0 - torch.as_tensor(np.asarray(mask01, np.float64))) * FMIN).to(dtype)


def trained_keys(enc_prefix, layers, kind):
    """The trainer's keys in its order: the layers' tensors in transformers' order, `pooler.dense` where trained, the head."""
    from vltk_amd.bert_ops import bert_layer_spec
    keys = []
    for i in layers:
        keys += [k for k, _ in bert_layer_spec(f"{enc_prefix}encoder.layer.{i}", 1, 1)]
    if kind == "classifier":
        keys += [enc_prefix + "pooler.dense.weight", enc_prefix + "pooler.dense.bias"]
    return tuple(keys + [kind + ".weight", kind + ".bias"])


# ---- the clip rule ---------------------------------------------------------------------------------------------------------------------
def clip_rule(grads, max_norm):
    """`clip_grad_norm_` written out in float64 -> (total norm, coef = min(1, max_norm / (norm + 1e-6)))."""
    norm = math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads))
    return norm, min(1.0, max_norm / (norm + 1e-6))


# ---- the yardstick: the same steps by torch on the CPU ------------------------------------------------------------------------------
def torch_finetune_run(sd, keys, x0, mask01, labels, steps, dtype, layers, heads, eps, kind, rows=None, enc_prefix="", lr=1e-3,
                       betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=0.01, step_lr=None, max_norm=None):
    """`steps` steps of loss.backward(); clip_grad_norm_; AdamW.step(); StepLR.step() on the tensors `keys` from the boundary
    hidden state x0 [B, L, H].  -> dict(losses [steps], tensors after the last step, grads of the FIRST step (after clipping),
    norms [steps] (before clipping; None without clipping), dk [steps][layer] = sum_m |dK[m, c]|, keybias [steps] = each
    step's key.bias gradients), numpy float64."""
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=dtype, requires_grad=True) for k in keys}
    x = torch.tensor(np.asarray(x0, np.float32)).to(dtype)
    mask = additive(mask01, dtype)
    y = torch.tensor(np.asarray(labels, np.int64))
    rows_t = None if rows is None else torch.as_tensor(np.asarray(rows, np.int64))
    opt = torch.optim.AdamW([p[k] for k in keys], lr=lr, betas=betas, eps=adam_eps, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.StepLR(opt, *step_lr) if step_lr else None
    out = dict(losses=[], norms=[], dk=[], keybias=[], first=None)
    for _ in range(steps):
        opt.zero_grad()
        taps = []
        loss = F.cross_entropy(tail_logits(p, x, mask, layers, heads, eps, kind, rows_t, enc_prefix, taps), y, ignore_index=IGNORE_INDEX)
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


# ---- the trajectory fixture: VisualBERT-QA, hidden 32, 4 heads, I = 64, 2 layers, Lt = 9, V = 7, visual dim 64, 16 labels, B = 16 ----
FIXTURE_CFG = dict(vocab_size=64, hidden_size=32, num_attention_heads=4, num_hidden_layers=2, intermediate_size=64,
                   max_position_embeddings=16, type_vocab_size=2, visual_embedding_dim=64)
FIXTURE_LABELS, FIXTURE_SEED, FIXTURE_LR, FIXTURE_STEP_LR = 16, 3, 1e-3, (20, 0.9)


WIDE = dict(hidden_size=128, num_attention_heads=4, intermediate_size=256)      # a 16-bit model's pooler needs hidden % 64 == 0


# Where the trainer's fp32 forward streams: Lx = 24 + 116 = 140 rows of d = 64 are past the LDS kernel's image (187 600 bytes).
LONG = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=24)
LONG_SHAPE = (2, 24, 116)                                                       # B, Lt, V

# BERT-base width: 12 heads of d = 64, I = 3072; 16 sequences of Lx = 20 + 36 = 56 rows are 896 rows, where vk_gemm_f32 and
# vk_gemm_16 pick the 128 x 128 tile for some of a layer's products and the 64 x 64 tile for the others.
BASE = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=24)
BASE_SHAPE = (16, 20, 36)                                                       # B, Lt, V


def trajectory_fixture(seed=FIXTURE_SEED, wide=False, long=False, base=False):
    """-> (cfg, state dict, inputs {name: numpy}, labels int64 [B]): partial text and visual masks (every text mask keeps at
    least 3 tokens, so the gathered row exists), every ninth label -100.  `wide`: the same fixture at hidden 128, I = 256, which
    a bf16 model can run (its own forward ends in the pooler, whose kernel takes channels in multiples of 64 in 16-bit types).
    `long`: hidden 128 in 2 heads (d = 64), B = 2, Lt = 24, V = 116, drawn in the same order from the same generator.
    `base`: BASE at B = 16, Lt = 20, V = 36, likewise."""
    from vltk_amd.visualbert import make_visualbert_qa_state_dict, visualbert_config
    cfg = visualbert_config(**dict(FIXTURE_CFG, **(WIDE if wide else {}), **(LONG if long else {}), **(BASE if base else {})))
    sd = make_visualbert_qa_state_dict(cfg, FIXTURE_LABELS, seed)
    r = np.random.Generator(np.random.PCG64([seed, 77]))
    B, Lt, V = LONG_SHAPE if long else BASE_SHAPE if base else (16, 9, 7)
    ids = r.integers(1, cfg["vocab_size"], (B, Lt)).astype(np.int64)
    feats = (np.maximum(r.standard_normal((B, V, cfg["visual_embedding_dim"])), 0) * 2.0).astype(np.float32)
    am = (np.arange(Lt)[None] < r.integers(3, Lt + 1, (B, 1))).astype(np.int64)
    vm = (np.arange(V)[None] < r.integers(2, V + 1, (B, 1))).astype(np.int64)
    labels = r.integers(0, FIXTURE_LABELS, B).astype(np.int64)
    labels[::9] = IGNORE_INDEX
    return cfg, sd, dict(input_ids=ids, visual_embeds=feats, attention_mask=am, visual_attention_mask=vm), labels


def fixture_boundary_cpu(cfg, sd, inputs, first):
    """The boundary hidden state of the fixture by the CPU oracle in fp32 (host tests only; the GPU tests take the model's own):
    the embeddings, then `first` layers.  -> [B, L, H] float32 numpy."""
    from visualbert_util import VisualBertOracle
    enc_sd = {k[len("visual_bert."):]: v for k, v in sd.items() if k.startswith("visual_bert.")}
    o = VisualBertOracle(cfg, enc_sd)
    with torch.no_grad():
        x = o.embeddings(inputs["input_ids"], inputs["visual_embeds"])
        mask = additive(np.concatenate((inputs["attention_mask"], inputs["visual_attention_mask"]), 1), torch.float32)[:, None, None, :]
        for i in range(first):
            x = o.bert_layer(x, mask, f"encoder.layer.{i}")
    return x.numpy()


def fixture_run(n, steps, dtype, x0, max_norm=None, seed=FIXTURE_SEED, long=False, base=False):
    """The yardstick on the trajectory fixture with the last n layers trained, from the boundary state x0."""
    cfg, sd, inputs, labels = trajectory_fixture(seed, long=long, base=base)
    nl = cfg["num_hidden_layers"]
    layers = [f"visual_bert.encoder.layer.{i}" for i in range(nl - n, nl)]
    keys = trained_keys("visual_bert.", range(nl - n, nl), "cls")
    rows = inputs["attention_mask"].sum(1) - 2
    mask01 = np.concatenate((inputs["attention_mask"], inputs["visual_attention_mask"]), 1)
    return keys, torch_finetune_run(sd, keys, x0, mask01, labels, steps, dtype, layers, cfg["num_attention_heads"], cfg["layer_norm_eps"],
                                    "cls", rows, "visual_bert.", lr=FIXTURE_LR, step_lr=FIXTURE_STEP_LR, max_norm=max_norm)


# ---- the attention backward in float64 numpy, with the per-element bounds ----------------------------------------------------------------
def launcher_scale(d):
    """The scale vk_attention_grad's launcher passes to its kernels, 1.0f / sqrtf((float)d), as a float64."""
    return float(np.float32(1.0) / np.sqrt(np.float32(d)))


def attention_grad_reference(q, k, v, mask, dout, heads, o_given=None, scale=None):
    """q, dout [B, Lq, heads * d]; k, v [B, Lk, heads * d]; mask additive [B, Lk] or None; all float64 (the stored fp32 values).
    -> dict(o, dq, dk, dv, b_dq, b_dk, b_dv): the reference and the bounds of the module docstring.  `o_given`: the O the kernel
    receives (default: the reference's own, rounded to fp32).  `scale`: the factor in place of 1 / sqrt(d) (the exact cases at a
    head dim that is no power of four pass `launcher_scale(d)`: dQ and dK are then S * scale with S the exact sum, a product of
    two 24-bit numbers, exact in float64, which one rounding takes to the kernel's bits)."""
    q, k, v, dout = (np.asarray(t, np.float64) for t in (q, k, v, dout))
    B, Lq, H = q.shape
    Lk, d = k.shape[1], H // heads
    scale = 1.0 / math.sqrt(d) if scale is None else float(scale)
    split = lambda t: t.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)          # [B, heads, L, d]
    join = lambda t: t.transpose(0, 2, 1, 3).reshape(B, -1, H)
    qh, kh, vh, doh = split(q), split(k), split(v), split(dout)
    mk = np.zeros((B, Lk)) if mask is None else np.asarray(mask, np.float64)
    absorbed = (mk < -1e30)[:, None, None, :]
    t = qh @ kh.transpose(0, 1, 3, 2) * scale
    assert np.abs(t).max() < 1e20
    s = np.where(absorbed, mk[:, None, None, :], t + mk[:, None, None, :])
    m = s.max(-1, keepdims=True)
    a = s - m
    e = np.exp(a)
    p = e / e.sum(-1, keepdims=True)
    o = p @ vh
    og = split(np.asarray(o_given, np.float64)) if o_given is not None else o.astype(np.float32).astype(np.float64)
    dP = doh @ vh.transpose(0, 1, 3, 2)
    D = (doh * o).sum(-1, keepdims=True)                                         # == sum_j p dP
    x = dP - D
    dS = p * x
    dq, dk, dv = dS @ kh * scale, dS.transpose(0, 1, 3, 2) @ qh * scale, p.transpose(0, 1, 3, 2) @ doh
    # the bounds
    u, T = U32, -(-Lk // AG_STEP)
    es = np.where(absorbed, 0.0, (d + 1) * u * scale * (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)) + u * np.abs(s))
    es_max = np.take_along_axis(es, s.argmax(-1)[..., None], -1)
    r = es + es_max + u * np.abs(a) + 2 * u
    rp = r + (p * r).sum(-1, keepdims=True) + (8 + 5 * T) * u
    eD = np.abs((doh * (og - o)).sum(-1, keepdims=True)) + 8 * u * (np.abs(doh) * np.abs(og)).sum(-1, keepdims=True)
    eP = d * u * (np.abs(doh) @ np.abs(vh).transpose(0, 1, 3, 2))
    eS = p * (eP + eD + u * np.abs(x)) + (rp + u) * p * np.abs(x)
    second, tiny = 1 + 2.0 ** -10, 2.0 ** -149
    b_dq = (scale * (eS @ np.abs(kh) + Lk * u * (np.abs(dS) @ np.abs(kh))) + u * np.abs(dq)) * second + Lk * 2.0 ** -126 + tiny
    eSt, dSt, pt = (w.transpose(0, 1, 3, 2) for w in (eS, dS, p))
    b_dk = (scale * (eSt @ np.abs(qh) + Lq * u * (np.abs(dSt) @ np.abs(qh))) + u * np.abs(dk)) * second + Lq * 2.0 ** -126 + tiny
    b_dv = ((rp * p).transpose(0, 1, 3, 2) @ np.abs(doh) + Lq * u * (pt @ np.abs(doh))) * second + Lq * 2.0 ** -126 + tiny
    return dict(o=join(o), dq=join(dq), dk=join(dk), dv=join(dv), b_dq=join(b_dq), b_dk=join(b_dk), b_dv=join(b_dv),
                terms=dict(dS=dS, p=p, kh=kh, qh=qh, vh=vh, doh=doh, og=og, dP=dP, D=D, x=x))


def torch_attention_grads(q, k, v, mask, dout, heads, dtype):
    """torch autograd through `attention` on the CPU in `dtype` -> (dq, dk, dv) float64 numpy."""
    ts = [torch.tensor(np.asarray(t, np.float64), dtype=dtype, requires_grad=True) for t in (q, k, v)]
    mk = None if mask is None else torch.tensor(np.asarray(mask, np.float64), dtype=dtype)
    attention(*ts, mk, heads).backward(torch.tensor(np.asarray(dout, np.float64), dtype=dtype))
    return tuple(t.grad.double().numpy() for t in ts)


def _grain(a):
    """The largest power of two every entry of `a` is a whole multiple of (1 for an all-zero array, 0 if there is none above 2^-80)."""
    a = np.abs(a[a != 0])
    for k in range(81 if a.size else 1):
        s = a * 2.0 ** k
        if (s == np.round(s)).all():
            return 2.0 ** -k
    return 0.0


def exact_in_fp32(ref):
    """Whether the data of an exact case is exact in fp32 whatever the order of the sums: p, dP, D, dP - D and dS are fp32 values,
    and for every sum the kernels form (dP, D, dQ, dK, dV) the sum of the absolute terms is below 2^24 times the terms' common
    grain (the product of the factors' grains).  The exact cases assert it of their own data before they ask for equal bits."""
    t = ref["terms"]
    if not all((t[k].astype(np.float32).astype(np.float64) == t[k]).all() for k in ("p", "dP", "D", "x", "dS")):
        return False

    def ok(abs_sums, *factors):
        g = float(np.prod([_grain(f) for f in factors]))
        return g > 0 and abs_sums.max() < 2.0 ** 24 * g

    dS, p, kh, qh, vh, doh, og = (t[k] for k in ("dS", "p", "kh", "qh", "vh", "doh", "og"))
    tr = lambda w: w.transpose(0, 1, 3, 2)
    return (ok(np.abs(doh) @ tr(np.abs(vh)), doh, vh) and ok((np.abs(doh) * np.abs(og)).sum(-1), doh, og) and
            ok(np.abs(dS) @ np.abs(kh), dS, kh) and ok(tr(np.abs(dS)) @ np.abs(qh), dS, qh) and ok(tr(p) @ np.abs(doh), p, doh))
