"""A Vision Transformer as the patch-token image encoder: an image becomes `1 + gh * gw` tokens, the sequence lengths the tiled
attention kernel was built for (197 tokens for 224 x 224 / 16, 577 for 384 x 384 / 16), where the Faster R-CNN front end gives 36 to
100 regions.  The reference names the model (`vltk/legacy/vit_ckp_convert.py:192-277` carries the B/16, B/32, L/16, L/32 and H/14
geometries, `vltk/utils/base.py:195-215` a checkpoint-key alias table for `vltk.models.vit.VisionTransformer`) but never shipped it.

Host-side mirror of `transformers.ViTModel` / `ViTForImageClassification` (modeling_vit.py v5.15: `ViTEmbeddings.forward` :129-161,
`ViTLayer.forward` :266-286, `ViTModel.forward` :356-388, `ViTForImageClassification.forward` :537-572) with the state-dict key
layout of those classes; the key names of published checkpoints (`encoder.layer.{i}.attention.attention.query` ...) load as well.
A pre-LN layer is the set of library calls of `BertOps._bert_layer` in another order, so the layers run on the ops `LxmertEncoder`
and `VisualBertModel` run on; what is new is the embedding stage (`vk_vit_patchify`, `vk_vit_assemble`, csrc/vit.hip).  All
arithmetic runs in `libvltk_hip.so`; torch only owns the device buffers.  No CPU fallback.

Out of scope: `bool_masked_pos` (and the masked-image-modeling head), `attention_mask`, `output_attentions` /
`output_hidden_states`, training, uint8 input (pixel values are fp32, already normalised), and a converter from the JAX `.npz`
checkpoints.
"""
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .bert_ops import LN_EPS, BertOps, Model, keep_head, require_gelu, seeded_tensor, to_numpy
from .layers import stream

DEFAULT_CONFIG = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                      layer_norm_eps=LN_EPS, image_size=224, patch_size=16, num_channels=3, qkv_bias=True)
# the public ViT geometries (Dosovitskiy et al. 2021, table 1): hidden, layers, heads, MLP, patch
GEOMETRIES = {"B/16": (768, 12, 12, 3072, 16), "B/32": (768, 12, 12, 3072, 32), "L/16": (1024, 24, 16, 4096, 16),
              "L/32": (1024, 24, 16, 4096, 32), "H/14": (1280, 32, 16, 5120, 14)}


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def vit_config(geometry=None, **kw):
    """transformers' `ViTConfig` defaults (ViT-B/16 at 224 x 224); `geometry` names one of GEOMETRIES instead.  `image_size` may
    be an (height, width) pair; the patch is square."""
    cfg = dict(DEFAULT_CONFIG)
    if geometry is not None:
        cfg.update(zip(("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "patch_size"), GEOMETRIES[geometry]))
    cfg.update(kw)
    require_gelu(cfg)
    if not cfg["qkv_bias"]:
        raise NotImplementedError("qkv_bias=False: the packed q/k/v GEMM always adds its bias")
    ph, pw = _pair(cfg["patch_size"])
    if ph != pw:
        raise NotImplementedError(f"patch_size {ph} x {pw}: vk_vit_patchify takes square patches")
    ih, iw = _pair(cfg["image_size"])
    if ph < 1 or ih < ph or iw < pw or ih % ph or iw % pw:
        raise ValueError(f"image_size {ih} x {iw} is no positive multiple of patch_size {ph}")
    if not 1 <= cfg["num_channels"] <= 4:
        raise ValueError(f"num_channels {cfg['num_channels']}: vk_vit_patchify takes 1..4")
    assert cfg["hidden_size"] % cfg["num_attention_heads"] == 0
    return cfg


def vit_grid(cfg):
    """(gh, gw) of the trained position table and the patch side P."""
    (ih, iw), P = _pair(cfg["image_size"]), _pair(cfg["patch_size"])[0]
    return ih // P, iw // P, P


def vit_param_spec(cfg, add_pooling_layer=True):
    """(name, shape) of every tensor of `transformers.ViTModel(config, add_pooling_layer).state_dict()`, in its order."""
    H, I, C = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_channels"]
    gh, gw, P = vit_grid(cfg)
    spec = [("embeddings.cls_token", (1, 1, H)), ("embeddings.position_embeddings", (1, gh * gw + 1, H)),
            ("embeddings.patch_embeddings.projection.weight", (H, C, P, P)), ("embeddings.patch_embeddings.projection.bias", (H,))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            spec += [(f"{p}.attention.{n}.weight", (H, H)), (f"{p}.attention.{n}.bias", (H,))]
        for n in ("layernorm_before", "layernorm_after"):
            spec += [(f"{p}.{n}.weight", (H,)), (f"{p}.{n}.bias", (H,))]
        spec += [(f"{p}.mlp.fc1.weight", (I, H)), (f"{p}.mlp.fc1.bias", (I,)), (f"{p}.mlp.fc2.weight", (H, I)), (f"{p}.mlp.fc2.bias", (H,))]
    spec += [("layernorm.weight", (H,)), ("layernorm.bias", (H,))]
    if add_pooling_layer:
        spec += [("pooler.dense.weight", (H, H)), ("pooler.dense.bias", (H,))]
    return spec


def vit_classifier_param_spec(cfg, num_labels):
    """`transformers.ViTForImageClassification(config).state_dict()`: the model (no pooler) under `vit.` + `classifier`."""
    return [("vit." + k, s) for k, s in vit_param_spec(cfg, add_pooling_layer=False)] + [
        ("classifier.weight", (num_labels, cfg["hidden_size"])), ("classifier.bias", (num_labels,))]


def _seeded(name, shape, seed):
    # seeded_tensor gives the gamma draw to names with "LayerNorm.weight" / "layer_norm.weight": ViT spells them layernorm*
    return seeded_tensor(re.sub(r"(layernorm(_before|_after)?)\.weight$", r"\1.LayerNorm.weight", name), shape, seed)


def make_vit_state_dict(cfg, seed=0, add_pooling_layer=True):
    """Seeded synthetic weights, drawn as `make_lxmert_state_dict` draws them: N(0, 0.05) matrices, tables and biases,
    LayerNorm gamma ~ U(0.5, 1.5)."""
    return {name: _seeded(name, shape, seed) for name, shape in vit_param_spec(cfg, add_pooling_layer)}


def make_vit_classifier_state_dict(cfg, num_labels, seed=0):
    return {name: _seeded(name[4:] if name.startswith("vit.") else name, shape, seed)
            for name, shape in vit_classifier_param_spec(cfg, num_labels)}


# key names of the published checkpoints (transformers before the q_proj / layers layout) -> the installed class's
_HUB_RENAMES = ((r"^encoder\.layer\.(\d+)\.attention\.attention\.query\.", r"layers.\1.attention.q_proj."),
                (r"^encoder\.layer\.(\d+)\.attention\.attention\.key\.", r"layers.\1.attention.k_proj."),
                (r"^encoder\.layer\.(\d+)\.attention\.attention\.value\.", r"layers.\1.attention.v_proj."),
                (r"^encoder\.layer\.(\d+)\.attention\.output\.dense\.", r"layers.\1.attention.o_proj."),
                (r"^encoder\.layer\.(\d+)\.intermediate\.dense\.", r"layers.\1.mlp.fc1."),
                (r"^encoder\.layer\.(\d+)\.output\.dense\.", r"layers.\1.mlp.fc2."),
                (r"^encoder\.layer\.(\d+)\.layernorm_(before|after)\.", r"layers.\1.layernorm_\2."))


def rename_hub_keys(sd, prefix=""):
    """A state dict with every hub-era key (behind `prefix`) renamed to the installed transformers' name; other keys pass.  Two keys
    that land on one name raise."""
    out = {}
    for k, v in sd.items():
        new = k
        if k.startswith(prefix):
            tail = k[len(prefix):]
            for pat, rep in _HUB_RENAMES:
                tail, n = re.subn(pat, rep, tail)
                if n:
                    break
            new = prefix + tail
        if new in out:
            raise RuntimeError(f"load_state_dict: '{k}' and another key both name '{new}'")
        out[new] = v
    return out


def check_pixel_values(pixel_values, cfg, interpolate_pos_encoding=False):
    """`pixel_values [B, C, Hi, Wi]` against the config -> (B, gh, gw).  Host-side, shapes only: it runs without a GPU and before any
    launch or capture.  ValueError for another rank or channel count, a side that is no positive multiple of the patch, and (as
    transformers) a size other than the model's without `interpolate_pos_encoding`."""
    shape = tuple(pixel_values.shape)
    if len(shape) != 4 or shape[0] < 1:
        raise ValueError(f"pixel_values must be [B, C, H, W] with B >= 1, got {shape}")
    B, C, Hi, Wi = shape
    if C != cfg["num_channels"]:
        raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the configuration."
                         f" Expected {cfg['num_channels']} but got {C}.")
    (ih, iw), P = _pair(cfg["image_size"]), _pair(cfg["patch_size"])[0]
    if Hi < P or Wi < P or Hi % P or Wi % P:
        raise ValueError(f"Input image size ({Hi}*{Wi}) is no positive multiple of the patch size {P}")
    if not interpolate_pos_encoding and (Hi, Wi) != (ih, iw):
        raise ValueError(f"Input image size ({Hi}*{Wi}) doesn't match model ({ih}*{iw}).")
    return B, Hi // P, Wi // P


def interpolate_position_table(pos, trained, grid):
    """transformers' `ViTEmbeddings.interpolate_pos_encoding` :89-127 on the host: `pos [N + 1, H]` fp32 trained for the
    `trained = (gh0, gw0)` grid -> the table `[gh * gw + 1, H]` of `grid = (gh, gw)`: the class row kept, the patch part resized by a
    bicubic `F.interpolate` with `align_corners=False`.  The trained grid itself returns the table as it is.  transformers reshapes
    the patch part to a square, so a non-square trained grid cannot be interpolated (ValueError)."""
    pos = torch.as_tensor(pos, dtype=torch.float32)
    if tuple(grid) == tuple(trained):
        return pos
    gh0, gw0 = trained
    if gh0 != gw0:
        raise ValueError(f"interpolate_pos_encoding: the trained {gh0} x {gw0} position grid is not square")
    H = pos.shape[1]
    patch = pos[1:].reshape(1, gh0, gw0, H).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(int(grid[0]), int(grid[1])), mode="bicubic", align_corners=False)
    return torch.cat((pos[:1], patch.permute(0, 2, 3, 1).reshape(-1, H)), 0)


def patch_tokens(sequence_output):
    """`last_hidden_state [B, N + 1, H]` without its class row -> `[B, N, H]` (a view): the `visual_embeds` of a
    `VisualBertModel(visual_embedding_dim=H)`, the `visual_feats` of an `LxmertEncoder(visual_feat_dim=H)`."""
    if sequence_output.dim() != 3 or sequence_output.shape[1] < 2:
        raise ValueError(f"patch_tokens: [B, N + 1, H] expected, got {tuple(sequence_output.shape)}")
    return sequence_output[:, 1:, :]


def vit_patch_boxes(Hi, Wi, P, normalized=False):
    """`[gh * gw, 4]` fp32: (x1, y1, x2, y2) of every patch in pixels, in the row order of the tokens; `normalized` divides by
    (Wi, Hi, Wi, Hi), which is LXMERT's `visual_pos`."""
    if P < 1 or Hi < P or Wi < P or Hi % P or Wi % P:
        raise ValueError(f"a {Hi} x {Wi} image is no positive multiple of the patch size {P}")
    ys, xs = np.meshgrid(np.arange(Hi // P, dtype=np.float32) * P, np.arange(Wi // P, dtype=np.float32) * P, indexing="ij")
    boxes = np.stack((xs, ys, xs + P, ys + P), -1).reshape(-1, 4).astype(np.float32)
    if normalized:
        boxes /= np.asarray((Wi, Hi, Wi, Hi), np.float32)
    return boxes


class ViTModel(BertOps):
    """`transformers.ViTModel` on the HIP path: `model(pixel_values [B, C, Hi, Wi], interpolate_pos_encoding=False)` ->
    (last_hidden_state [B, N + 1, H] with the class token first, pooler_output [B, H] or None without a pooling layer)."""

    _INPUTS = ("pixel_values",)
    _PROJ = "embeddings.patch_embeddings.projection"

    def __init__(self, config, precision="bf16", device="cuda:0", add_pooling_layer=True):
        super().__init__(vit_config(**config), precision, device)
        self.add_pooling_layer = bool(add_pooling_layer)
        self._pos = {}                                    # (gh, gw) -> position table [gh * gw + 1, H] on the device, storage type

    def load_state_dict(self, sd, strict=True):
        sd = rename_hub_keys(to_numpy(sd))
        self._check_state_dict(sd, dict(vit_param_spec(self.cfg, self.add_pooling_layer)), strict)
        H = self.cfg["hidden_size"]
        self._lin[self._PROJ] = self._pack(sd[self._PROJ + ".weight"].reshape(H, -1), sd[self._PROJ + ".bias"])
        self._cls = torch.from_numpy(sd["embeddings.cls_token"].reshape(H)).to(self.device).to(self.tdt).contiguous()
        self._pos_f32 = torch.from_numpy(np.ascontiguousarray(sd["embeddings.position_embeddings"][0]))
        self._pos = {}
        for i in range(self.cfg["num_hidden_layers"]):
            p = f"layers.{i}"
            self._load_lin(sd, p + ".attention.qkv", *(f"{p}.attention.{n}_proj" for n in "qkv"))
            for n in ("attention.o_proj", "mlp.fc1", "mlp.fc2"):
                self._load_lin(sd, f"{p}.{n}", f"{p}.{n}")
            self._load_ln(sd, p + ".layernorm_before")
            self._load_ln(sd, p + ".layernorm_after")
        self._load_ln(sd, "layernorm")
        if self.add_pooling_layer:
            self._load_lin(sd, "pooler.dense", "pooler.dense")
        self._loaded = True
        return self

    def position_table(self, gh, gw):
        """The position table of a `gh x gw` grid on the device: a transformation of a weight, made once per grid on the host from
        the fp32 table, rounded to the storage type and kept."""
        if (gh, gw) not in self._pos:
            t = interpolate_position_table(self._pos_f32, vit_grid(self.cfg)[:2], (gh, gw))
            self._pos[(gh, gw)] = t.to(self.device).to(self.tdt).contiguous()
        return self._pos[(gh, gw)]

    def _check(self, pixel_values, interpolate_pos_encoding=False):
        check_pixel_values(pixel_values, self.cfg, interpolate_pos_encoding)

    def __call__(self, pixel_values, interpolate_pos_encoding=False):
        return self._run(self._forward, (pixel_values,), interpolate_pos_encoding=interpolate_pos_encoding)

    def embeddings(self, pixel_values, interpolate_pos_encoding=False):
        """The embedding stage alone: what transformers returns as `hidden_states[0]`, [B, N + 1, H]."""
        x = self._run(self._embed, (pixel_values,), interpolate_pos_encoding=interpolate_pos_encoding)
        return x.view(pixel_values.shape[0], -1, self.cfg["hidden_size"])

    def _before_capture(self, pixel_values):              # the table's host work and its copy happen before the capture
        P = vit_grid(self.cfg)[2]
        self.position_table(pixel_values.shape[2] // P, pixel_values.shape[3] // P)

    def capture(self, pixel_values, interpolate_pos_encoding=False):
        """Capture one forward for this input SHAPE into a HIP graph (one stream, no branches).  Returns `replay(pixel_values)`,
        which copies the new pixels into the captured buffer, launches the graph and returns the (static) output tensors; another
        shape raises ValueError."""
        run = self._capture_inputs((pixel_values,), interpolate_pos_encoding=interpolate_pos_encoding)

        def replay(pixel_values):
            return run((pixel_values,))
        return replay

    @torch.no_grad()
    def _embed(self, pixel_values):
        """-> embeddings [B * (N + 1), H]: patch rows, the projection GEMM, then class row and positions in one launch."""
        self._require_loaded()
        cfg, dev = self.cfg, self.device
        B, C, Hi, Wi = pixel_values.shape
        P, H = vit_grid(cfg)[2], cfg["hidden_size"]
        gh, gw = Hi // P, Wi // P
        N = gh * gw
        pix = pixel_values.to(dev, torch.float32).contiguous()
        Kp = self._lin[self._PROJ][3]
        rows = torch.empty((B * N, Kp), dtype=self.tdt, device=dev)
        L.call("vk_vit_patchify", pix.data_ptr(), B, C, Hi, Wi, P, rows.data_ptr(), Kp, self.dt, stream(dev))
        proj = self._linear(rows, self._PROJ)
        pos = self.position_table(gh, gw)
        x = torch.empty((B * (N + 1), H), dtype=self.tdt, device=dev)
        L.call("vk_vit_assemble", proj.data_ptr(), proj.stride(0), self._cls.data_ptr(), pos.data_ptr(), B, N, x.data_ptr(), H, self.dt,
               stream(dev))
        return x

    def _layer(self, p, x, B, Lx):                        # ViTLayer.forward :266-286: pre-LN, both residuals in the GEMM epilogues
        H = self.cfg["hidden_size"]
        h = self._layernorm(x, p + ".layernorm_before")
        qkv = self._linear(h, p + ".attention.qkv")
        ctx = self._attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], None, B, Lx, Lx)
        x = self._linear(ctx, p + ".attention.o_proj", residual=x)
        h = self._layernorm(x, p + ".layernorm_after")
        h = self._linear(h, p + ".mlp.fc1", act=L.VK_ACT_GELU)
        return self._linear(h, p + ".mlp.fc2", residual=x)

    def _sequence(self, pixel_values):
        """-> the final LayerNorm's output [B * (N + 1), H]."""
        x = self._embed(pixel_values)
        B = pixel_values.shape[0]
        Lx = x.shape[0] // B
        for i in range(self.cfg["num_hidden_layers"]):
            x = self._layer(f"layers.{i}", x, B, Lx)
        return self._layernorm(x, "layernorm"), B, Lx

    @torch.no_grad()
    def _forward(self, pixel_values):
        x, B, Lx = self._sequence(pixel_values)
        return x.view(B, Lx, self.cfg["hidden_size"]), (self._pooler(x, B, Lx) if self.add_pooling_layer else None)


class ViTForImageClassification(Model):
    """`transformers.ViTForImageClassification` on the HIP path: the encoder without its pooler, then `classifier` on the class
    row of the normalised sequence output.  `model(pixel_values, interpolate_pos_encoding=False)` returns logits
    `[B, num_labels]` in the storage type."""

    def __init__(self, config, num_labels, precision="bf16", device="cuda:0"):
        self.vit = ViTModel(config, precision, device, add_pooling_layer=False)
        self.num_labels = int(num_labels)
        if self.num_labels < 1:
            raise ValueError("num_labels must be >= 1")

    def load_state_dict(self, sd, strict=True):
        enc = self.vit
        sd = self._load_with_encoder(enc, "vit.", vit_classifier_param_spec(enc.cfg, self.num_labels), sd, strict,
                                     rekey=lambda sd: rename_hub_keys(sd, prefix="vit."))
        enc._load_lin(sd, "classifier", "classifier")
        keep_head(enc, sd, "classifier")
        return self

    def _head_features(self, pixel_values):
        enc = self.vit
        x, B, Lx = enc._sequence(pixel_values)
        idx = (torch.arange(B, dtype=torch.int32, device=enc.device) * Lx).contiguous()
        return enc._gather_rows(x, idx)                                         # the class row of each sequence

    @torch.no_grad()
    def head_features(self, pixel_values, interpolate_pos_encoding=False):
        """What `classifier` consumes: the class row of the normalised sequence output [B, H], storage type
        (`HeadTrainer.step_features` takes it)."""
        return self.vit._run(self._head_features, (pixel_values,), interpolate_pos_encoding=interpolate_pos_encoding)

    @torch.no_grad()
    def __call__(self, pixel_values, interpolate_pos_encoding=False):
        enc = self.vit
        return enc._run(lambda pixel_values: enc._linear(self._head_features(pixel_values), "classifier"), (pixel_values,),
                        interpolate_pos_encoding=interpolate_pos_encoding)
