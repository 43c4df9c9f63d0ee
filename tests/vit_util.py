"""TEST INFRASTRUCTURE ONLY -- tests/golden/vit_small.npz (tools/gen_golden_vit.py): its models rebuilt from the seed, the stored
cases, and a CPU restatement of transformers' ViT forward.

`ViTOracle` follows transformers/models/vit/modeling_vit.py (v5.15): ViTPatchEmbeddings.forward :62-69, ViTEmbeddings.forward
:129-161 with interpolate_pos_encoding :89-127, ViTAttention.forward :207-238, ViTLayer.forward :266-286, ViTModel.forward
:356-388, ViTForImageClassification.forward :537-572.  It takes `q`, `linear` and `ln` (and with them the rounding points of a GEMM
and a LayerNorm) from `oracle.lxmert_oracle.LxmertOracle`.  It is pinned by the stored vectors of transformers itself
(tests/test_vit_host.py).  `emulate="bf16"|"fp16"` rounds where the HIP path stores: the patch rows, the projection output, the
class token and the position table, every GEMM and LayerNorm output, the attention probabilities before the second product and
the attention output; the embedding sum and the residual sums are fp32 with one rounding, as in csrc/vit.hip and the GEMM epilogue.
"""
import math
import re

import numpy as np
import torch
import torch.nn.functional as F

from oracle.lxmert_oracle import LxmertOracle
from vltk_amd.vit import (interpolate_position_table, make_vit_classifier_state_dict, make_vit_state_dict, vit_config, vit_grid)

CASES = ["square", "tall", "long", "p14"]


def _value(a):
    a = np.asarray(a)
    return tuple(int(v) for v in a) if a.ndim else int(a)


def golden_model(g, name):
    """-> (cfg, state dict) of the fixture's model `name` ("main" | "p14")."""
    pre = f"cfg/{name}/"
    cfg = vit_config(**{k[len(pre):]: _value(g[k]) for k in g.files if k.startswith(pre)})
    return cfg, make_vit_state_dict(cfg, int(g["seed"]))


def golden_classifier(g):
    """-> (cfg, classifier state dict, num_labels) of the fixture's main model."""
    cfg, _ = golden_model(g, "main")
    n = int(g["num_labels"])
    return cfg, make_vit_classifier_state_dict(cfg, n, int(g["seed"])), n


def golden_case(g, case):
    """-> (model name, pixel_values [B, 3, Hi, Wi], interpolate_pos_encoding) of one stored case."""
    return str(g[f"{case}/model"]), g[f"{case}/pixel_values"], bool(g[f"{case}/interpolate_pos_encoding"])


def hub_era_names(sd, prefix=""):
    """The state dict under the key names published ViT checkpoints carry (`encoder.layer.{i}.attention.attention.query` ...)."""
    table = (("attention.q_proj", "attention.attention.query"), ("attention.k_proj", "attention.attention.key"),
             ("attention.v_proj", "attention.attention.value"), ("attention.o_proj", "attention.output.dense"),
             ("mlp.fc1", "intermediate.dense"), ("mlp.fc2", "output.dense"))
    out = {}
    for k, v in sd.items():
        m = re.match(rf"^{re.escape(prefix)}layers\.(\d+)\.(.*)\.(weight|bias)$", k)
        if m:
            mod = dict(table).get(m.group(2), m.group(2))
            k = f"{prefix}encoder.layer.{m.group(1)}.{mod}.{m.group(3)}"
        out[k] = v
    return out


class ViTOracle(LxmertOracle):
    def embeddings(self, pixel_values, interpolate_pos_encoding=False):
        sd, q, cfg = self.sd, self.q, self.cfg
        pix = torch.as_tensor(pixel_values).float()
        B, C, Hi, Wi = pix.shape
        gh0, gw0, P = vit_grid(cfg)
        if not interpolate_pos_encoding:
            assert (Hi // P, Wi // P) == (gh0, gw0)
        rows = q(F.unfold(pix, P, stride=P).transpose(1, 2))                        # [B, N, C * P * P] in (c, py, px) order
        w = sd["embeddings.patch_embeddings.projection.weight"]
        proj = q(F.linear(rows, q(w.reshape(w.shape[0], -1))) + sd["embeddings.patch_embeddings.projection.bias"])
        pos = q(interpolate_position_table(sd["embeddings.position_embeddings"][0], (gh0, gw0), (Hi // P, Wi // P)))
        cls = q(sd["embeddings.cls_token"]).reshape(1, 1, -1).expand(B, 1, -1)
        return q(torch.cat((cls, proj), 1) + pos[None])

    def vit_attention(self, x, p):
        B, Lx, H = x.shape
        heads = self.cfg["num_attention_heads"]
        d = H // heads
        qh, kh, vh = (self.linear(x, f"{p}.{n}_proj").view(B, Lx, heads, d).transpose(1, 2) for n in "qkv")
        s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(d)
        o = torch.matmul(self.q(F.softmax(s, dim=-1)), vh)
        return self.q(o.permute(0, 2, 1, 3).reshape(B, Lx, H))

    def layer(self, x, p):
        h = self.q(self.ln(x, p + ".layernorm_before"))
        x = self.linear(self.vit_attention(h, p + ".attention"), p + ".attention.o_proj", residual=x)
        h = self.q(self.ln(x, p + ".layernorm_after"))
        return self.linear(self.linear(h, p + ".mlp.fc1", act="gelu"), p + ".mlp.fc2", residual=x)

    def forward(self, pixel_values, interpolate_pos_encoding=False, return_stages=False):
        x = self.embeddings(pixel_values, interpolate_pos_encoding)
        st = {"embeddings": x}
        for i in range(self.cfg["num_hidden_layers"]):
            x = self.layer(x, f"layers.{i}")
        seq = self.q(self.ln(x, "layernorm"))
        pooled = self.linear(seq[:, 0], "pooler.dense", act="tanh") if "pooler.dense.weight" in self.sd else None
        return ((seq, pooled), st) if return_stages else (seq, pooled)

    def classify(self, pixel_values, interpolate_pos_encoding=False):
        """State dict with the `vit.` prefix and `classifier.*`: classifier(sequence_output[:, 0])."""
        full = self.sd
        self.sd = {k[len("vit."):]: v for k, v in full.items() if k.startswith("vit.")}
        try:
            seq, _ = self.forward(pixel_values, interpolate_pos_encoding)
        finally:
            self.sd = full
        return self.linear(seq[:, 0], "classifier")
