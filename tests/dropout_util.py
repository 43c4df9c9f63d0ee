"""TEST INFRASTRUCTURE ONLY -- what the dropout tests share: csrc/philox.h restated in numpy (Philox4x32-10, the byte rule, the two
granule maps), `vk_dropout_add_f32` restated in fp32, the float64 attention reference of tests/finetune_util.py with a keep mask,
and `Attention16` / `bert_layer_16` of tests/mixed_util.py with the trainer's masks.  No GPU, and not the code under test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import finetune_util as U
import mixed_util as X

M32 = 0xFFFFFFFF
# Random123's known answers for philox4x32_10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(seed, stream, granule):
    """-> uint32 [n, 4]: key (seed_lo, seed_hi), counter (granule_lo, granule_hi, stream_lo, stream_hi)."""
    g = np.asarray(granule, np.uint64).reshape(-1)
    c = [g & M32, g >> 32, np.full_like(g, stream & M32), np.full_like(g, stream >> 32)]
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, -1).astype(np.uint32)


def rule(p):
    """-> (t, rs as the fp32 number the kernels use)."""
    t = int(np.rint(np.float32(p) * np.float32(256)))
    return t, float(np.float32(256.0) / np.float32(256 - t))


def keep_elements(n, p, seed, stream):
    """bool [n]: element i is byte i & 15 of granule i >> 4."""
    return philox(seed, stream, np.arange((n + 15) // 16)).view(np.uint8).reshape(-1)[:n] >= rule(p)[0]


def keep_attention(B, heads, Lq, Lk, p, seed, stream):
    """bool [B, heads, Lq, Lk]: byte 4 (q & 3) + (k & 3) of granule ((b heads + h) ceil(Lq / 4) + (q >> 2)) ceil(Lk / 4) + (k >> 2)."""
    nq, nk = (Lq + 3) // 4, (Lk + 3) // 4
    g = (np.arange(B * heads, dtype=np.uint64)[:, None, None] * nq + np.arange(nq, dtype=np.uint64)[None, :, None]) * nk + np.arange(nk, dtype=np.uint64)
    b = philox(seed, stream, g).view(np.uint8).reshape(B * heads, nq, nk, 4, 4).transpose(0, 1, 3, 2, 4)
    return b.reshape(B, heads, nq * 4, nk * 4)[:, :, :Lq, :Lk] >= rule(p)[0]


def dropout_add(x, res, p, seed, stream):
    """fp32: (keep ? x * rs : 0) + res, one rounding per product and per sum."""
    y = np.where(keep_elements(x.size, p, seed, stream), x * np.float32(rule(p)[1]), np.float32(0))
    return y if res is None else y + res


def attention_reference(q, k, v, mask, dout, heads, dtype, keep, rs, o_given=None, scale=None):
    """`finetune_util.attention_grad_reference` under dropout(softmax(s)) with the mask `keep` and the scale `rs`, from its own `terms`:
    o, dq, dk, dv in float64, and the terms `exact_in_16` reads (P~ in place of P; `og`: the 16-bit O the kernel is given)."""
    t = U.attention_grad_reference(q, k, v, mask, dout, heads, scale=scale)["terms"]
    p, kh, qh, vh, doh = (t[n] for n in ("p", "kh", "qh", "vh", "doh"))
    B, _, H = q.shape
    sc = 1.0 / math.sqrt(H // heads) if scale is None else float(scale)
    join = lambda w: w.transpose(0, 2, 1, 3).reshape(B, -1, H)
    tr = lambda w: w.transpose(0, 1, 3, 2)
    pt = keep * rs * p
    o = pt @ vh
    og = X.round16(o, dtype) if o_given is None else np.asarray(o_given, np.float64).reshape(B, -1, heads, H // heads).transpose(0, 2, 1, 3)
    dP = keep * rs * (doh @ tr(vh))
    D = (doh * o).sum(-1, keepdims=True)
    dS = p * (dP - D)
    return dict(o=join(o), dq=join(dS @ kh * sc), dk=join(tr(dS) @ qh * sc), dv=join(tr(pt) @ doh),
                terms=dict(t, p=pt, p_undropped=p, dS=dS, og=og, dP=dP, D=D, x=dP - D))


# ---- the trainer's yardstick: the layers of mixed_util.py (dtype bf16) or finetune_util.py (dtype None) with the dropout sites ------------
def _r(t, dtype):
    return t if dtype is None else X._r(t, dtype)


class Attention16(torch.autograd.Function):
    """`mixed_util.Attention16` with `kr` = keep * rs on the probabilities (dtype None: nothing rounds): O = r((r(P) keep) V rs);
    dV = r(P kr)^T dO, dS = r(P (kr dO V^T - D))."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, dtype, kr):
        B, Lq, H = q.shape
        d = H // heads
        qh, kh, vh = (t.view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d) + mask[:, None, None, :], -1)
        o = _r(_r(p, dtype) * kr @ vh, dtype)
        ctx.save_for_backward(qh, kh, vh, p, o, kr)
        ctx.cfg = (dtype, d, (B, Lq, H))
        return o.transpose(1, 2).reshape(B, Lq, H)

    @staticmethod
    def backward(ctx, do):
        qh, kh, vh, p, o, kr = ctx.saved_tensors
        dtype, d, (B, Lq, H) = ctx.cfg
        doh = _r(do, dtype).view(B, Lq, -1, d).transpose(1, 2)
        ds = _r(p * (kr * (doh @ vh.transpose(-1, -2)) - (doh * o).sum(-1, keepdim=True)), dtype)
        back = lambda t: t.transpose(1, 2).reshape(B, -1, H)
        return back(ds @ kh / math.sqrt(d)), back(ds.transpose(-1, -2) @ qh / math.sqrt(d)), back(_r(p * kr, dtype).transpose(-1, -2) @ doh), None, None, None, None


def bert_layer(p, P, x, mask, heads, eps, dtype, kr_att, kr1, kr2, taps):
    """`mixed_util.bert_layer_16` (dtype None: `finetune_util.bert_layer`) with the three masks, each keep * rs."""
    lin = (lambda t, k, ry=False, rdx=False: F.linear(t, p[k + ".weight"], p[k + ".bias"])) if dtype is None else \
          (lambda t, k, ry=False, rdx=False: X.Linear16.apply(t, p[k + ".weight"], p[k + ".bias"], dtype, ry, rdx))
    H = x.shape[-1]
    q, k, v = (lin(x, P + ".attention.self." + t, True) for t in ("query", "key", "value"))
    k.retain_grad()
    taps.append(k)
    ctx = Attention16.apply(q, k, v, mask, heads, dtype, kr_att)
    o = P + ".attention.output."
    h1 = F.layer_norm(lin(ctx, o + "dense", False, True) * kr1 + x, (H,), p[o + "LayerNorm.weight"], p[o + "LayerNorm.bias"], eps)
    z = F.gelu(lin(h1, P + ".intermediate.dense"))
    o = P + ".output."
    return F.layer_norm(lin(z, o + "dense") * kr2 + h1, (H,), p[o + "LayerNorm.weight"], p[o + "LayerNorm.bias"], eps)


def trainer_run(n, steps, x0, mode, hidden, attention, seed, max_norm=None):
    """`mixed_util.fixture_run` on the wide fixture with the trainer's dropout sites (stream = step * 2^16 + site; sites 1 + 3 i,
    2 + 3 i, 3 + 3 i of trained layer i, 1 + 3 n the head's rows) -> (keys, its dict).  mode: torch.bfloat16 the mixed mode's
    yardstick, None the pure-float64 run, torch.float32 torch's own fp32 run."""
    cfg, sd, inputs, labels = U.trajectory_fixture(wide=True)
    real, dtype = (torch.float32, None) if mode == torch.float32 else (torch.float64, mode)
    heads, eps, nl = cfg["num_attention_heads"], cfg["layer_norm_eps"], cfg["num_hidden_layers"]
    layers, keys = [f"visual_bert.encoder.layer.{i}" for i in range(nl - n, nl)], U.trained_keys("visual_bert.", range(nl - n, nl), "cls")
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=real, requires_grad=True) for k in keys}
    x0 = torch.tensor(np.asarray(x0, np.float32)).to(real)
    B, Lx, H = x0.shape
    mask = U.additive(np.concatenate((inputs["attention_mask"], inputs["visual_attention_mask"]), 1), real)
    rows, y = torch.as_tensor(inputs["attention_mask"].sum(1) - 2), torch.tensor(labels)
    opt = torch.optim.AdamW([p[k] for k in keys], lr=U.FIXTURE_LR, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.StepLR(opt, *U.FIXTURE_STEP_LR)
    grads = lambda ks: {k: p[k].grad.detach().double().numpy().copy() for k in ks}
    out = dict(losses=[], dk=[], keybias=[], first=None)
    for step in range(steps):
        def kr(site, rate, shape):
            keep = keep_attention(B, heads, Lx, Lx, rate, seed, (step << 16) + site) if len(shape) == 4 else \
                keep_elements(int(np.prod(shape)), rate, seed, (step << 16) + site).reshape(shape)
            return torch.tensor(keep * rule(rate)[1], dtype=real)
        opt.zero_grad()
        x, taps = x0, []
        for i, P in enumerate(layers):
            x = bert_layer(p, P, x, mask, heads, eps, dtype, kr(1 + 3 * i, attention, (B, heads, Lx, Lx)), kr(2 + 3 * i, hidden, x.shape),
                           kr(3 + 3 * i, hidden, x.shape), taps)
        head = torch.ones_like(x)
        head[torch.arange(B), rows] = kr(1 + 3 * n, hidden, (B, H))              # the gathered rows alone reach the head
        loss = F.cross_entropy(U.head_logits(p, x * head, "cls", rows, "visual_bert."), y, ignore_index=U.IGNORE_INDEX)
        loss.backward()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p[k] for k in keys], max_norm)
        out["dk"].append([t.grad.detach().double().abs().sum((0, 1)).numpy() for t in taps])
        out["keybias"].append(grads(k for k in keys if k.endswith("key.bias")))
        out["first"] = out["first"] or grads(keys)
        opt.step()
        sched.step()
        out["losses"].append(float(loss.detach().double()))
    return keys, dict(out, losses=np.array(out["losses"]), tensors={k: p[k].detach().double().numpy() for k in keys})
