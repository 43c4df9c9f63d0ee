"""LayoutLMv3's attention on the HIP path: the per-(head, query, key) relative-position bias of every v3 layer
formed inside the attention kernel, never materialised as [B, heads, L, L].  Restated from
transformers/models/layoutlmv3/modeling_layoutlmv3.py (v5.15): `LayoutLMv3Encoder.relative_position_bucket`, `_cal_1d_pos_emb`,
`_cal_2d_pos_emb`, `LayoutLMv3SelfAttention.forward`.

  relpos_lut             the three bias matrices of a model -> the kernel's table, once per model, on the CPU
  relpos_triples         position ids and boxes -> the kernel's per-token (pos, x, y)
  attention_relpos       one launch of vk_attention_relpos on device tensors
  attention_relpos_form  which kernel that launch runs on, and the queries a workgroup of it serves

All arithmetic of the attention runs in `libvltk_hip.so`; torch owns the buffers.  No CPU fallback.
"""
import math

import torch

from . import _lib as L
from .layers import DTYPES, stream

FORMS = ("mfma", "strict")          # VK_RELPOS_FORM_* by value
_DT = {td: dt for dt, td in DTYPES.values()}


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """transformers' bidirectional bucket of a tensor of integer differences, by its own float32 expression (so the same buckets):
    half the buckets per sign, exact below num_buckets / 4, logarithmic up to max_distance, constant from there on."""
    num_buckets //= 2
    ret = (relative_position > 0).long() * num_buckets
    n = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    return ret + torch.where(is_small, n, val_if_large)


def relpos_lut(rel_pos_bias, rel_pos_x_bias, rel_pos_y_bias, max_rel_pos=128, max_rel_2d_pos=256):
    """`encoder.rel_pos_bias.weight [heads, rel_pos_bins]`, `encoder.rel_pos_x_bias.weight` and `encoder.rel_pos_y_bias.weight
    [heads, rel_2d_pos_bins]` -> (lut [heads, (2 r1 + 1) + 2 (2 r2 + 1)] fp32 on the CPU, r1, r2): T1, TX, TY of a head side by side,
    entry `delta + r` of a table being the weight of delta's bucket.  The bucket is constant from max_distance on, so r = max_distance
    and a lookup by the clamped difference is exact."""
    parts = []
    for w, r in ((rel_pos_bias, max_rel_pos), (rel_pos_x_bias, max_rel_2d_pos), (rel_pos_y_bias, max_rel_2d_pos)):
        w = torch.as_tensor(w, dtype=torch.float32)
        parts.append(w[:, relative_position_bucket(torch.arange(-r, r + 1), w.shape[1], r)])
    return torch.cat(parts, 1).contiguous(), max_rel_pos, max_rel_2d_pos


def relpos_triples(position_ids, bbox):
    """position_ids [B, L] and bbox [B, L, 4] -> int32 [B, L, 3]: (position, x = bbox[..., 0], y = bbox[..., 3]), the coordinates
    `_cal_2d_pos_emb` takes differences of."""
    return torch.stack([position_ids, bbox[..., 0], bbox[..., 3]], -1).to(torch.int32).contiguous()


def attention_relpos_form(Lq, Lk, d, dtype, ldq, ldk, ldv, aligned16=True):
    """(form name, queries per workgroup) of a launch; raises what the launch would."""
    f = L.load().vk_attention_relpos_form(Lq, Lk, d, _DT[dtype], ldq, ldk, ldv, int(aligned16))
    if f < 0:
        L.check(-f)
    return FORMS[f], L.load().vk_attention_relpos_queries(f, Lq)


def attention_relpos(q, k, v, rel_q, rel_k, lut, r1, r2, heads, mask=None):
    """softmax((q k^T + bias) / sqrt(d) + mask) v per (batch, head) with bias[b, h, i, j] = T1[h][c(pk - pq)] + (TX[h][c(xk - xq)] +
    TY[h][c(yk - yq)]) looked up inside the kernel.  q [B * Lq, heads * d] and k, v [B * Lk, heads * d] are 2-D device tensors of
    one floating type (column slices of a fused projection are fine: the row stride is the leading dimension); rel_q [B, Lq, 3]
    and rel_k [B, Lk, 3] int32 (`relpos_triples`; self-attention passes one tensor twice); lut, r1, r2 from `relpos_lut`, lut on
    the device; mask [B, Lk] additive fp32 or None.  Returns [B * Lq, heads * d]."""
    B, Lq, Lk = rel_q.shape[0], rel_q.shape[1], rel_k.shape[1]
    for name, t, rows in (("q", q, B * Lq), ("k", k, B * Lk), ("v", v, B * Lk)):
        if t.dim() != 2 or t.shape != (rows, q.shape[1]) or t.stride(1) != 1 or t.dtype != q.dtype or t.device != q.device:
            raise ValueError(f"{name} must be [{rows}, {q.shape[1]}] of {q.dtype} on {q.device} with unit column stride, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}")
    if q.dtype not in _DT or q.shape[1] % heads:
        raise ValueError(f"q of {q.dtype} with {q.shape[1]} columns for {heads} heads")
    for name, t, shape in (("rel_q", rel_q, (B, Lq, 3)), ("rel_k", rel_k, (B, Lk, 3))):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous() or t.device != q.device:
            raise ValueError(f"{name} must be contiguous int32 {shape} on {q.device}")
    nlut = (2 * r1 + 1) + 2 * (2 * r2 + 1)
    if tuple(lut.shape) != (heads, nlut) or lut.dtype != torch.float32 or not lut.is_contiguous() or lut.device != q.device:
        raise ValueError(f"lut must be contiguous fp32 [{heads}, {nlut}] on {q.device}")
    if mask is not None and (tuple(mask.shape) != (B, Lk) or mask.dtype != torch.float32 or not mask.is_contiguous() or mask.device != q.device):
        raise ValueError(f"mask must be contiguous fp32 [{B}, {Lk}] on {q.device}")
    H = q.shape[1]
    out = torch.empty((B * Lq, H), dtype=q.dtype, device=q.device)
    L.call("vk_attention_relpos", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
           mask.data_ptr() if mask is not None else None, rel_q.data_ptr(), rel_k.data_ptr(), lut.data_ptr(), r1, r2, out.data_ptr(), H, B,
           heads, Lq, Lk, H // heads, _DT[q.dtype], stream(q.device))
    return out
