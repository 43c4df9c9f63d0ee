"""LayoutLMv3 on the HIP path: the document model over OCR words, their boxes and the page image.  Restated
from transformers/models/layoutlmv3/modeling_layoutlmv3.py (v5.15) with the state-dict key layout of its classes, so a real
checkpoint's tensors load by name.

The attention: the per-(head, query, key) relative-position bias of every v3 layer formed inside the attention kernel, never
materialised as [B, heads, L, L] (`LayoutLMv3Encoder.relative_position_bucket`, `_cal_1d_pos_emb`, `_cal_2d_pos_emb`,
`LayoutLMv3SelfAttention.forward`).

  relpos_lut             the three bias matrices of a model -> the kernel's table, once per model, on the CPU
  relpos_triples         position ids and boxes -> the kernel's per-token (pos, x, y)
  attention_relpos       one launch of vk_attention_relpos on device tensors
  attention_relpos_form  which kernel that launch runs on, and the queries a workgroup of it serves
  attention_relpos_grad  its backward: dq, dk, dv and the gradient of the table, one call of vk_attention_relpos_grad
  relpos_bucket_map      the fold's map from table entry to bucket; relpos_lut_grad sums a table gradient back into a bias matrix's

The model: `LayoutLMv3Model` (`LayoutLMv3Model.forward` :623-796) and its three inference heads (:799-823, :834-1121).  Its layers
are the shared post-LN BERT layers of `bert_ops.BertOps` with that attention in place of the plain one; what is new on the device is
the embedding stage, `vk_layoutlmv3_embed` (csrc/layoutlmv3.hip): text and patch rows, their two LayerNorms each, the attention's
(pos, x, y) triples and the joint mask in one launch.

  layoutlmv3_config, layoutlmv3_param_spec, layoutlmv3_head_param_spec, make_layoutlmv3_state_dict, make_layoutlmv3_head_state_dict
  visual_bbox            transformers' `create_visual_bbox`: the boxes of the class token and the patches
  LayoutLMv3Model, LayoutLMv3ForTokenClassification, LayoutLMv3ForQuestionAnswering, LayoutLMv3ForSequenceClassification

Out of scope (each raises): an image without text, `inputs_embeds`, a caller's `position_ids`, an image of another size than
`input_size` (the interpolated `pos_embed`), training and losses, `output_attentions` / `output_hidden_states`.

All arithmetic runs in `libvltk_hip.so`; torch owns the buffers.  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib as L
from .bert_ops import BertOps, Model, bert_layer_spec, check_text_inputs, host_array, keep_head, require_gelu, seeded_tensor, to_numpy
from .layers import DTYPES, stream
from .layoutlm import check_bbox, span_select, token_word_labels

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


def relpos_bucket_map(rel_pos_bins, rel_2d_pos_bins, max_rel_pos=128, max_rel_2d_pos=256):
    """int32 [(2 r1 + 1) + 2 (2 r2 + 1)] on the CPU: the bucket of every entry of the folded table, T1 | TX | TY side by side (entry
    `delta + r` of a table holds the weight of delta's bucket)."""
    return torch.cat([relative_position_bucket(torch.arange(-r, r + 1), bins, r)
                      for bins, r in ((rel_pos_bins, max_rel_pos), (rel_2d_pos_bins, max_rel_2d_pos), (rel_2d_pos_bins, max_rel_2d_pos))]).to(torch.int32)


def relpos_lut(rel_pos_bias, rel_pos_x_bias, rel_pos_y_bias, max_rel_pos=128, max_rel_2d_pos=256):
    """`encoder.rel_pos_bias.weight [heads, rel_pos_bins]`, `encoder.rel_pos_x_bias.weight` and `encoder.rel_pos_y_bias.weight
    [heads, rel_2d_pos_bins]` -> (lut [heads, (2 r1 + 1) + 2 (2 r2 + 1)] fp32 on the CPU, r1, r2): T1, TX, TY of a head side by side,
    entry `delta + r` of a table being the weight of delta's bucket.  The bucket is constant from max_distance on, so r = max_distance
    and a lookup by the clamped difference is exact."""
    ws = [torch.as_tensor(w, dtype=torch.float32) for w in (rel_pos_bias, rel_pos_x_bias, rel_pos_y_bias)]
    bucket = relpos_bucket_map(ws[0].shape[1], ws[1].shape[1], max_rel_pos, max_rel_2d_pos).long()
    n1, n2 = 2 * max_rel_pos + 1, 2 * max_rel_2d_pos + 1
    parts = [w[:, bucket[o:o + n]] for w, o, n in zip(ws, (0, n1, n1 + n2), (n1, n2, n2))]
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


def attention_relpos_grad(q, k, v, o, dout, rel_q, rel_k, lut, r1, r2, heads, mask=None, out=None):
    """The backward of `attention_relpos` on its matrix-core form (bf16 / fp16, head dim 32 / 64): q, k, v, rel_q, rel_k, lut, r1,
    r2, heads and mask as the forward took them, o its output and dout [B * Lq, heads * d] the gradient of that output, in the
    type of q.  -> (dq [B * Lq, H], dk, dv [B * Lk, H], dlut [heads, (2 r1 + 1) + 2 (2 r2 + 1)]), all fp32; dlut is the gradient of
    `lut`, summed in fixed point: the same bits on every run.  `out`: (dq, dk, dv) to write into, fp32 2-D tensors with unit column
    stride (the column blocks of one [B * L, 3H] buffer are fine).  Everything the kernel refuses raises ValueError."""
    B, Lq, Lk, H = rel_q.shape[0], rel_q.shape[1], rel_k.shape[1], q.shape[1]
    dev = q.device
    if out is None:
        out = tuple(torch.empty((B * n, H), dtype=torch.float32, device=dev) for n in (Lq, Lk, Lk))
    for name, t, rows, dt in (("q", q, B * Lq, q.dtype), ("k", k, B * Lk, q.dtype), ("v", v, B * Lk, q.dtype), ("o", o, B * Lq, q.dtype),
                              ("dout", dout, B * Lq, q.dtype), ("dq", out[0], B * Lq, torch.float32), ("dk", out[1], B * Lk, torch.float32),
                              ("dv", out[2], B * Lk, torch.float32)):
        if t.dim() != 2 or tuple(t.shape) != (rows, H) or t.stride(1) != 1 or t.dtype != dt or t.device != dev:
            raise ValueError(f"{name} must be [{rows}, {H}] of {dt} on {dev} with unit column stride, got {tuple(t.shape)} {t.dtype} {t.device}")
    if q.dtype not in (torch.bfloat16, torch.float16) or H % heads:
        raise ValueError(f"attention_relpos_grad takes bf16 or fp16 with heads dividing the width, got {q.dtype}, {H} columns, {heads} heads")
    for name, t, shape in (("rel_q", rel_q, (B, Lq, 3)), ("rel_k", rel_k, (B, Lk, 3))):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be contiguous int32 {shape} on {dev}")
    nlut = (2 * r1 + 1) + 2 * (2 * r2 + 1)
    if tuple(lut.shape) != (heads, nlut) or lut.dtype != torch.float32 or not lut.is_contiguous() or lut.device != dev:
        raise ValueError(f"lut must be contiguous fp32 [{heads}, {nlut}] on {dev}")
    if mask is not None and (tuple(mask.shape) != (B, Lk) or mask.dtype != torch.float32 or not mask.is_contiguous() or mask.device != dev):
        raise ValueError(f"mask must be contiguous fp32 [{B}, {Lk}] on {dev}")
    dlut = torch.empty((heads, nlut), dtype=torch.float32, device=dev)
    need = L.load().vk_attention_relpos_grad_workspace_bytes(B, heads, Lq, r1, r2)
    ws = torch.empty((max(need, 8) // 8,), dtype=torch.int64, device=dev)
    args = []
    for t in (q, k, v):
        args += [t.data_ptr(), t.stride(0)]
    args += [mask.data_ptr() if mask is not None else None, rel_q.data_ptr(), rel_k.data_ptr(), lut.data_ptr(), r1, r2]
    for t in (o, dout) + tuple(out):
        args += [t.data_ptr(), t.stride(0)]
    L.call("vk_attention_relpos_grad", *args, dlut.data_ptr(), B, heads, Lq, Lk, H // heads, _DT[q.dtype], ws.data_ptr(), need, stream(dev))
    return out[0], out[1], out[2], dlut


def relpos_lut_grad(dlut, bucket, r1, r2, term, out, accumulate=False):
    """`out [heads, bins]` fp32 (a bias matrix's gradient) = or, with `accumulate`, += the entries of term `term` (0: the 1-D table,
    1: x, 2: y) of `dlut` that share a bucket, by `bucket` (`relpos_bucket_map` on the device): fp64 sums in ascending entry order."""
    heads, nlut = dlut.shape
    if nlut != (2 * r1 + 1) + 2 * (2 * r2 + 1) or dlut.dtype != torch.float32 or not dlut.is_contiguous():
        raise ValueError(f"dlut must be contiguous fp32 [heads, {(2 * r1 + 1) + 2 * (2 * r2 + 1)}], got {tuple(dlut.shape)} {dlut.dtype}")
    if tuple(bucket.shape) != (nlut,) or bucket.dtype != torch.int32 or not bucket.is_contiguous() or bucket.device != dlut.device:
        raise ValueError(f"bucket must be contiguous int32 [{nlut}] on {dlut.device}")
    if out.dim() != 2 or out.shape[0] != heads or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dlut.device:
        raise ValueError(f"out must be contiguous fp32 [{heads}, bins] on {dlut.device}")
    L.call("vk_relpos_lut_grad", dlut.data_ptr(), heads, r1, r2, term, bucket.data_ptr(), out.shape[1], out.data_ptr(), int(accumulate),
           stream(dlut.device))
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
DEFAULT_CONFIG = dict(vocab_size=50265, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                      max_position_embeddings=512, max_2d_position_embeddings=1024, type_vocab_size=2, layer_norm_eps=1e-5,
                      hidden_act="gelu", pad_token_id=1, coordinate_size=128, shape_size=128, input_size=224, patch_size=16,
                      num_channels=3, rel_pos_bins=32, max_rel_pos=128, rel_2d_pos_bins=64, max_rel_2d_pos=256,
                      has_relative_attention_bias=True, has_spatial_attention_bias=True, visual_embed=True)
NORM_EPS = 1e-6                          # LayoutLMv3Model.norm, fixed in transformers (:563)
EMBED_FORMS = ("vector", "scalar")       # VK_L3E_FORM_* by value
TEXT_TABLES = ("word_embeddings", "token_type_embeddings", "position_embeddings", "x_position_embeddings", "y_position_embeddings",
               "h_position_embeddings", "w_position_embeddings")
HEADS = {"token": "classifier", "qa": "qa_outputs", "seq": "classifier"}


def layoutlmv3_config(**kw):
    """transformers' `LayoutLMv3Config` defaults (v5.15: 512 positions; the published base checkpoint's config.json says 514)."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(kw)
    require_gelu(cfg)
    H, cs, ss = cfg["hidden_size"], cfg["coordinate_size"], cfg["shape_size"]
    if H % cfg["num_attention_heads"]:
        raise ValueError(f"hidden_size {H} is no multiple of num_attention_heads {cfg['num_attention_heads']}")
    if 4 * cs + 2 * ss != H:             # the concatenated spatial row is added to the word row (:195)
        raise ValueError(f"4 * coordinate_size ({cs}) + 2 * shape_size ({ss}) must be hidden_size ({H})")
    P, S = cfg["patch_size"], cfg["input_size"]
    if cfg["visual_embed"] and (P < 1 or S < P or S % P or not 1 <= cfg["num_channels"] <= 4):
        raise ValueError(f"input_size {S} must be a positive multiple of patch_size {P}, with 1..4 channels")
    return cfg


def visual_bbox(gh, gw, max_len=1000):
    """transformers' `create_visual_bbox` (:575-596) -> int32 [1 + gh * gw, 4]: the class token's box (1, 1, 999, 999), then the
    patches row by row with the edges floor(1000 i / gw) and floor(1000 j / gh)."""
    xs, ys = np.arange(gw + 1) * max_len // gw, np.arange(gh + 1) * max_len // gh
    grid = np.stack((np.tile(xs[:-1], (gh, 1)), np.tile(ys[:-1, None], (1, gw)), np.tile(xs[1:], (gh, 1)), np.tile(ys[1:, None], (1, gw))), -1)
    return np.concatenate(([[1, 1, max_len - 1, max_len - 1]], grid.reshape(-1, 4))).astype(np.int32)


def layoutlmv3_param_spec(cfg):
    """(name, shape) of every tensor of `transformers.LayoutLMv3Model(config).state_dict()`, in its order."""
    H, I, cs, ss, M2 = cfg["hidden_size"], cfg["intermediate_size"], cfg["coordinate_size"], cfg["shape_size"], cfg["max_2d_position_embeddings"]
    g = cfg["input_size"] // cfg["patch_size"]
    heads = cfg["num_attention_heads"]
    e = "embeddings."
    spec = [("cls_token", (1, 1, H)), ("pos_embed", (1, g * g + 1, H))] if cfg["visual_embed"] else []
    spec += [(e + "word_embeddings.weight", (cfg["vocab_size"], H)), (e + "token_type_embeddings.weight", (cfg["type_vocab_size"], H)),
             (e + "LayerNorm.weight", (H,)), (e + "LayerNorm.bias", (H,)),
             (e + "position_embeddings.weight", (cfg["max_position_embeddings"], H)), (e + "x_position_embeddings.weight", (M2, cs)),
             (e + "y_position_embeddings.weight", (M2, cs)), (e + "h_position_embeddings.weight", (M2, ss)),
             (e + "w_position_embeddings.weight", (M2, ss))]
    if cfg["visual_embed"]:
        spec += [("patch_embed.proj.weight", (H, cfg["num_channels"], cfg["patch_size"], cfg["patch_size"])), ("patch_embed.proj.bias", (H,)),
                 ("LayerNorm.weight", (H,)), ("LayerNorm.bias", (H,)), ("norm.weight", (H,)), ("norm.bias", (H,))]
    for i in range(cfg["num_hidden_layers"]):
        spec += bert_layer_spec(f"encoder.layer.{i}", H, I)
    if cfg["has_relative_attention_bias"]:
        spec += [("encoder.rel_pos_bias.weight", (heads, cfg["rel_pos_bins"]))]
    if cfg["has_spatial_attention_bias"]:
        spec += [("encoder.rel_pos_x_bias.weight", (heads, cfg["rel_2d_pos_bins"])), ("encoder.rel_pos_y_bias.weight", (heads, cfg["rel_2d_pos_bins"]))]
    return spec


def _plain_head(head, num_labels):
    """Whether a head is one nn.Linear: the token head below 10 labels (:841-844); every other head is dense -> tanh -> out_proj."""
    return head == "token" and num_labels < 10


def layoutlmv3_head_param_spec(cfg, head, num_labels):
    """`state_dict()` of a head class ("token" | "qa" | "seq"): the model under `layoutlmv3.` + `classifier` / `qa_outputs`."""
    H, p = cfg["hidden_size"], HEADS[head]
    own = [(p + ".weight", (num_labels, H)), (p + ".bias", (num_labels,))] if _plain_head(head, num_labels) else [
        (p + ".dense.weight", (H, H)), (p + ".dense.bias", (H,)), (p + ".out_proj.weight", (num_labels, H)), (p + ".out_proj.bias", (num_labels,))]
    return [("layoutlmv3." + k, s) for k, s in layoutlmv3_param_spec(cfg)] + own


def _seeded(name, shape, seed):
    # seeded_tensor gives the gamma draw to names with "LayerNorm.weight": the patch rows' first LayerNorm is spelled `norm`
    return seeded_tensor("norm.LayerNorm.weight" if name == "norm.weight" else name, shape, seed)


def make_layoutlmv3_state_dict(cfg, seed=0):
    """Seeded synthetic weights, drawn as `make_lxmert_state_dict` draws them: N(0, 0.05) matrices, tables and biases (so
    `cls_token`, `pos_embed` and the three bias matrices, which transformers initialises to zero, are not), LayerNorm gamma ~ U(0.5, 1.5)."""
    return {name: _seeded(name, shape, seed) for name, shape in layoutlmv3_param_spec(cfg)}


def make_layoutlmv3_head_state_dict(cfg, head, num_labels, seed=0):
    sd = {"layoutlmv3." + k: v for k, v in make_layoutlmv3_state_dict(cfg, seed).items()}
    n_own = 2 if _plain_head(head, num_labels) else 4
    for name, shape in layoutlmv3_head_param_spec(cfg, head, num_labels)[-n_own:]:
        sd[name] = seeded_tensor(name, shape, seed)
    return sd


def embed_form(H, coordinate_size, shape_size, dtype, aligned16=True):
    """The form a `vk_layoutlmv3_embed` launch takes ("vector" | "scalar"); raises what the launch would."""
    f = L.load().vk_layoutlmv3_embed_form(H, coordinate_size, shape_size, _DT[dtype], int(aligned16))
    if f < 0:
        raise ValueError(f"vk_layoutlmv3_embed takes no rows of {H} = 4 * {coordinate_size} + 2 * {shape_size} elements of {dtype}")
    return EMBED_FORMS[f]


def check_layoutlmv3_inputs(cfg, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
    """Everything that needs the values of an input, on the host, before a launch or a capture: ValueError for ids, token types or
    box coordinates outside their tables, a box with x1 < x0 or y1 < y0, a RoBERTa position (`pad + number of non-pad ids so far`)
    past `max_position_embeddings`, a mask of another shape, an image the model does not take."""
    if input_ids is None:
        raise ValueError("LayoutLMv3Model needs input_ids: an image without text is out of scope")
    if input_ids.dim() != 2 or 0 in input_ids.shape:
        raise ValueError(f"input_ids [B, L] with B, L >= 1 expected, got {tuple(input_ids.shape)}")
    B, Lt = input_ids.shape
    try:
        check_text_inputs(input_ids, token_type_ids, cfg)
        check_bbox(bbox, B, Lt, cfg["max_2d_position_embeddings"])
    except IndexError as e:
        raise ValueError(str(e)) from e
    last = cfg["pad_token_id"] + int((host_array(input_ids) != cfg["pad_token_id"]).sum(1).max())
    if last >= cfg["max_position_embeddings"]:
        raise ValueError(f"position id {last} (pad_token_id + the non-pad tokens of a row) exceeds max_position_embeddings = "
                         f"{cfg['max_position_embeddings']}")
    if attention_mask is not None and tuple(attention_mask.shape) != (B, Lt):
        raise ValueError(f"attention_mask must be {(B, Lt)}, got {tuple(attention_mask.shape)}")
    if pixel_values is not None:
        want = (B, cfg["num_channels"], cfg["input_size"], cfg["input_size"])
        if not cfg["visual_embed"] or tuple(pixel_values.shape) != want:
            raise ValueError(f"pixel_values must be {want} (visual_embed={cfg['visual_embed']}; another image size needs the "
                             f"interpolated pos_embed, which is out of scope), got {tuple(pixel_values.shape)}")


class LayoutLMv3Model(BertOps):
    """`transformers.LayoutLMv3Model` on the HIP path: `model(input_ids, bbox=None, attention_mask=None, token_type_ids=None,
    pixel_values=None)` -> last_hidden_state [B, Lt + V, H], the text rows first (V = 1 + patches with an image, 0 without; v3 has
    no pooler).  Defaults are transformers': bbox all zeros, the mask all ones, token types 0."""

    _INPUTS = ("input_ids", "bbox", "attention_mask", "token_type_ids", "pixel_values")
    _PROJ = "patch_embed.proj"

    def __init__(self, config, precision="bf16", device="cuda:0"):
        super().__init__(layoutlmv3_config(**config), precision, device)
        self._lut = self._rel = None

    def load_state_dict(self, sd, strict=True):
        sd = to_numpy(sd)
        cfg = self.cfg
        self._check_state_dict(sd, dict(layoutlmv3_param_spec(cfg)), strict)
        for t in TEXT_TABLES:
            self._load_tab(sd, t)
        self._load_ln(sd, "embeddings.LayerNorm")
        if cfg["visual_embed"]:
            H, g = cfg["hidden_size"], cfg["input_size"] // cfg["patch_size"]
            self._lin[self._PROJ] = self._pack(sd[self._PROJ + ".weight"].reshape(H, -1), sd[self._PROJ + ".bias"])
            self._cls = torch.from_numpy(sd["cls_token"].reshape(H)).to(self.device).to(self.tdt).contiguous()
            self._pos_embed = torch.from_numpy(np.ascontiguousarray(sd["pos_embed"][0])).to(self.device).to(self.tdt).contiguous()
            self._vbox = torch.from_numpy(visual_bbox(g, g)).to(self.device)
            self._load_ln(sd, "LayerNorm")
            self._load_ln(sd, "norm")
        for i in range(cfg["num_hidden_layers"]):
            self._load_bert_layer(sd, f"encoder.layer.{i}")
        # SelfAttention.forward :265-268 adds (rel_pos + rel_2d_pos) with both flags, rel_pos with the first alone and nothing
        # otherwise: a term that is not added is a table of zeros (adding 0.0 is exact); no term at all is the plain attention
        self._lut = None
        if cfg["has_relative_attention_bias"]:
            zeros = np.zeros((cfg["num_attention_heads"], cfg["rel_2d_pos_bins"]), np.float32)
            xy = [sd[f"encoder.rel_pos_{a}_bias.weight"] for a in "xy"] if cfg["has_spatial_attention_bias"] else [zeros, zeros]
            lut, self._r1, self._r2 = relpos_lut(sd["encoder.rel_pos_bias.weight"], *xy, cfg["max_rel_pos"], cfg["max_rel_2d_pos"])
            self._lut = lut.to(self.device)
        self._loaded = True
        return self

    def _check(self, *inputs):
        check_layoutlmv3_inputs(self.cfg, *inputs)

    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None, position_ids=None,
                 inputs_embeds=None):
        if position_ids is not None or inputs_embeds is not None:
            raise TypeError("LayoutLMv3Model: position_ids and inputs_embeds are out of scope")
        return self._run(self._forward, (input_ids, bbox, attention_mask, token_type_ids, pixel_values))

    def capture(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
        """Capture one forward for these input SHAPES into a HIP graph.  Returns `replay(...)` with the model's signature; an input
        given as None at capture stays at its default.  The position ids are counted in the kernel, so a replay follows new pad
        tokens with no host pass."""
        run = self._capture_inputs((input_ids, bbox, attention_mask, token_type_ids, pixel_values))

        def replay(input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
            return run((input_ids, bbox, attention_mask, token_type_ids, pixel_values))
        return replay

    def embeddings(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
        """The embedding stage alone, [B, Lt + V, H]: what transformers feeds its encoder (text `embeddings` and `forward_image`
        joined, then `LayerNorm` with an image)."""
        x, _ = self._run(self._embed, (input_ids, bbox, attention_mask, token_type_ids, pixel_values))
        return x.view(input_ids.shape[0], -1, self.cfg["hidden_size"])

    def embed_form(self):
        return embed_form(self.cfg["hidden_size"], self.cfg["coordinate_size"], self.cfg["shape_size"], self.tdt)

    def relpos_form(self, Lx):
        """(form, queries per workgroup) of every layer's attention at a joint length, or None where the plain attention runs."""
        H = self.cfg["hidden_size"]
        return None if self._lut is None else attention_relpos_form(Lx, Lx, H // self.cfg["num_attention_heads"], self.tdt, 3 * H, 3 * H, 3 * H)

    @torch.no_grad()
    def _embed(self, input_ids, bbox, attention_mask, token_type_ids, pixel_values):
        """-> (embeddings [B * (Lt + V), H], additive mask [B, Lt + V] or None); the attention's triples are kept for the layers."""
        self._require_loaded()
        cfg, dev, tab = self.cfg, self.device, self._tab
        B, Lt = input_ids.shape
        H = cfg["hidden_size"]
        ids = input_ids.to(dev, torch.int64).contiguous()
        tts = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.to(dev, torch.int64).contiguous()
        box = torch.zeros((B, Lt, 4), dtype=torch.int32, device=dev) if bbox is None else bbox.to(dev, torch.int32).contiguous()   # :717
        am = None if attention_mask is None else attention_mask.to(dev, torch.float32).contiguous()
        V, proj, ldp, visual = 0, None, 0, (None,) * 3 + (0,) + (None,) * 2 + (NORM_EPS,) + (None,) * 2
        if pixel_values is not None:
            P = cfg["patch_size"]
            V = (cfg["input_size"] // P) ** 2 + 1
            pix = pixel_values.to(dev, torch.float32).contiguous()
            Kp = self._lin[self._PROJ][3]
            rows = torch.empty((B * (V - 1), Kp), dtype=self.tdt, device=dev)
            L.call("vk_vit_patchify", pix.data_ptr(), B, cfg["num_channels"], cfg["input_size"], cfg["input_size"], P, rows.data_ptr(), Kp,
                   self.dt, stream(dev))
            proj = self._linear(rows, self._PROJ)          # PatchEmbeddings.proj: the conv as a GEMM over the patch rows
            ldp = proj.stride(0)
            (gn, bn), (go, bo) = self._ln["norm"], self._ln["LayerNorm"]
            visual = (self._cls.data_ptr(), self._pos_embed.data_ptr(), self._vbox.data_ptr(), V, gn.data_ptr(), bn.data_ptr(), NORM_EPS,
                      go.data_ptr(), bo.data_ptr())
        Lx = Lt + V
        x = torch.empty((B * Lx, H), dtype=self.tdt, device=dev)
        self._rel = torch.empty((B, Lx, 3), dtype=torch.int32, device=dev)
        mask = torch.empty((B, Lx), dtype=torch.float32, device=dev) if (am is not None or V) else None
        g, b = self._ln["embeddings.LayerNorm"]
        L.call("vk_layoutlmv3_embed", ids.data_ptr(), tts.data_ptr(), box.data_ptr(), am.data_ptr() if am is not None else None, B, Lt,
               cfg["pad_token_id"], tab["word_embeddings"].data_ptr(), cfg["vocab_size"], tab["token_type_embeddings"].data_ptr(),
               cfg["type_vocab_size"], tab["position_embeddings"].data_ptr(), cfg["max_position_embeddings"],
               tab["x_position_embeddings"].data_ptr(), tab["y_position_embeddings"].data_ptr(), tab["h_position_embeddings"].data_ptr(),
               tab["w_position_embeddings"].data_ptr(), cfg["max_2d_position_embeddings"], cfg["coordinate_size"], cfg["shape_size"],
               g.data_ptr(), b.data_ptr(), cfg["layer_norm_eps"], proj.data_ptr() if proj is not None else None, ldp, *visual, x.data_ptr(),
               self._rel.data_ptr(), mask.data_ptr() if mask is not None else None, H, self.dt, stream(dev))
        return x, mask

    def _self_attention(self, q, k, v, mask, B, Lx):
        """LayoutLMv3SelfAttention.forward :235-288 with the bias formed in the kernel.  transformers' `cogview_attention` (:223-233)
        is soft-max restated for fp16's range; the kernel's fp32 online soft-max needs nothing for it."""
        if self._lut is None:
            return self._attention(q, k, v, mask, B, Lx, Lx)
        return attention_relpos(q, k, v, self._rel, self._rel, self._lut, self._r1, self._r2, self.cfg["num_attention_heads"], mask)

    def _encode(self, *inputs):
        """-> (the last layer's rows [B * L, H], B, L)."""
        x, mask = self._embed(*inputs)
        B = inputs[0].shape[0]
        Lx = x.shape[0] // B
        for i in range(self.cfg["num_hidden_layers"]):
            x = self._bert_layer(f"encoder.layer.{i}", x, mask, B, Lx)
        return x, B, Lx

    def _forward(self, *inputs):
        x, B, Lx = self._encode(*inputs)
        return x.view(B, Lx, self.cfg["hidden_size"])

    def _rows(self, x, B, Lx, n):
        """The first `n` rows of each of the B sequences of `x [B * Lx, H]` -> [B * n, H]: `x` itself where that is all of them,
        one gather launch otherwise (vk_linear takes no row stride)."""
        if n == Lx:
            return x
        idx = (torch.arange(B, dtype=torch.int32, device=self.device)[:, None] * Lx + torch.arange(n, dtype=torch.int32, device=self.device)[None])
        return self._gather_rows(x, idx.reshape(-1).contiguous())


class _Head(Model):
    """What the three heads share: the whole model under the `layoutlmv3.` prefix and `classifier` / `qa_outputs` on top of it,
    either one nn.Linear or `LayoutLMv3ClassificationHead` (:799-823: dense -> tanh -> out_proj, the tanh in the GEMM's epilogue)."""

    _KIND = "seq"

    def __init__(self, config, num_labels, precision="bf16", device="cuda:0"):
        self.layoutlmv3 = LayoutLMv3Model(config, precision, device)
        self.num_labels = int(num_labels)
        self._plain = _plain_head(self._KIND, self.num_labels)

    def load_state_dict(self, sd, strict=True):
        enc, p = self.layoutlmv3, HEADS[self._KIND]
        sd = self._load_with_encoder(enc, "layoutlmv3.", layoutlmv3_head_param_spec(enc.cfg, self._KIND, self.num_labels), sd, strict)
        for name in ((p,) if self._plain else (p + ".dense", p + ".out_proj")):
            enc._load_lin(sd, name, name)
            keep_head(enc, sd, name)
        return self

    def _head(self, rows):
        enc, p = self.layoutlmv3, HEADS[self._KIND]
        if self._plain:
            return enc._linear(rows, p)
        return enc._linear(enc._linear(rows, p + ".dense", act=L.VK_ACT_TANH), p + ".out_proj")

    def _logits(self, n_rows, inputs):
        """The head over the first `n_rows(Lt, L)` rows of every sequence, in one checked call -> [B * n, num_labels]."""
        enc = self.layoutlmv3

        def forward(*inputs):
            x, B, Lx = enc._encode(*inputs)
            return self._head(enc._rows(x, B, Lx, n_rows(inputs[0].shape[1], Lx)))
        return enc._run(forward, inputs)


class LayoutLMv3ForTokenClassification(_Head):
    """`transformers.LayoutLMv3ForTokenClassification` (:834-930): the head on the text rows only -> logits [B, Lt, num_labels]."""

    _KIND = "token"

    def word_labels(self, logits, word_ids, num_words):
        """`layoutlm.token_word_labels` (vk_token_word_labels) on this model's logits."""
        return token_word_labels(self.layoutlmv3, logits, word_ids, num_words)

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
        logits = self._logits(lambda Lt, Lx: Lt, (input_ids, bbox, attention_mask, token_type_ids, pixel_values))
        return logits.view(input_ids.shape[0], input_ids.shape[1], self.num_labels)


class LayoutLMv3ForQuestionAnswering(_Head):
    """`transformers.LayoutLMv3ForQuestionAnswering` (:933-1039): the head over the whole sequence -> (start_logits, end_logits),
    each [B, Lt + V]: the two columns of the GEMM's output, not copied."""

    _KIND = "qa"

    def best_span(self, start_logits, end_logits, context_mask, max_answer_tokens=30):
        """`layoutlm.span_select` (vk_span_select) on this model's logits."""
        return span_select(self.layoutlmv3, start_logits, end_logits, context_mask, max_answer_tokens)

    def __init__(self, config, precision="bf16", device="cuda:0"):
        super().__init__(config, 2, precision, device)

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
        logits = self._logits(lambda Lt, Lx: Lx, (input_ids, bbox, attention_mask, token_type_ids, pixel_values))
        B = input_ids.shape[0]
        return logits[:, 0].view(B, -1), logits[:, 1].view(B, -1)


class LayoutLMv3ForSequenceClassification(_Head):
    """`transformers.LayoutLMv3ForSequenceClassification` (:1049-1121): the head on row 0 of each sequence -> logits [B, num_labels]."""

    @torch.no_grad()
    def __call__(self, input_ids, bbox=None, attention_mask=None, token_type_ids=None, pixel_values=None):
        return self._logits(lambda Lt, Lx: 1, (input_ids, bbox, attention_mask, token_type_ids, pixel_values))
