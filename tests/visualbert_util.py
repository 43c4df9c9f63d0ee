"""TEST INFRASTRUCTURE ONLY -- tests/golden/visualbert_small.npz (tools/gen_golden_visualbert.py): its inputs rebuilt from the
seed, the keyword arguments of each stored case, and a CPU restatement of transformers' VisualBERT forward.

`VisualBertOracle` follows transformers/models/visual_bert/modeling_visual_bert.py (v5.15): VisualBertEmbeddings.forward :72-168,
VisualBertModel.forward :599-662, VisualBertForQuestionAnswering.forward :1106-1132.  Its layers are BERT layers, the ones
`oracle.lxmert_oracle.LxmertOracle` restates (linear / ln / attention / bert_layer and their rounding points), so it subclasses
that; what it adds is the embedding stage and the gather head.  It is pinned by the stored vectors of transformers itself
(tests/test_visualbert_host.py).  `emulate="bf16"|"fp16"` rounds where the HIP path stores: the tables, the projection output
and the LayerNorm output; the embedding sums stay fp32, as in csrc/visualbert.hip.
"""
import numpy as np
import torch

from oracle.lxmert_oracle import LxmertOracle
from vltk_amd.visualbert import make_visualbert_qa_state_dict, make_visualbert_state_dict, visualbert_config

CASES = [("short", "masked"), ("short", "plain"), ("long", "masked"), ("long", "aligned")]


def golden_inputs(g, geo):
    """-> (cfg, state dict, visual_embeds [B, V, 2048]) of one geometry ("short" | "long"); the generator's order of draws."""
    cfg = visualbert_config(**{k[4:]: int(g[k]) for k in g.files if k.startswith("cfg/")})
    seed = int(g["seed"])
    ids = g[f"{geo}/input_ids"]
    B, Lt = ids.shape
    V = g[f"{geo}/visual_attention_mask"].shape[1]
    r = np.random.Generator(np.random.PCG64([seed, Lt]))
    assert (r.integers(1, cfg["vocab_size"], (B, Lt)) == ids).all()
    r.integers(0, 2, (B, Lt))
    feats = np.maximum(r.standard_normal((B, V, cfg["visual_embedding_dim"])), 0).astype(np.float32) * 2.0
    return cfg, make_visualbert_state_dict(cfg, seed), feats


def golden_qa_state_dict(g):
    cfg = visualbert_config(**{k[4:]: int(g[k]) for k in g.files if k.startswith("cfg/")})
    return make_visualbert_qa_state_dict(cfg, int(g["qa/num_labels"]), int(g["seed"]))


def case_kwargs(g, geo, case):
    """Keyword arguments of the stored case `<geo>/<case>` besides input_ids and visual_embeds (numpy arrays)."""
    kw = {}
    if case in ("masked", "aligned"):
        kw.update({k: g[f"{geo}/{k}"] for k in ("attention_mask", "visual_attention_mask", "token_type_ids")})
    if case == "aligned":
        kw.update({k: g[f"{geo}/{k}"] for k in ("image_text_alignment", "visual_token_type_ids")})
    return kw


class VisualBertOracle(LxmertOracle):
    def embeddings(self, input_ids, visual_embeds, token_type_ids=None, visual_token_type_ids=None, image_text_alignment=None):
        sd, q = self.sd, self.q
        ids = torch.as_tensor(input_ids).long()
        B, Lt = ids.shape
        vf = q(torch.as_tensor(visual_embeds).float())
        V = vf.shape[1]
        tts = torch.zeros_like(ids) if token_type_ids is None else torch.as_tensor(token_type_ids).long()
        vtts = torch.ones((B, V), dtype=torch.long) if visual_token_type_ids is None else torch.as_tensor(visual_token_type_ids).long()
        pos = q(sd["embeddings.position_embeddings.weight"])
        text = q(sd["embeddings.word_embeddings.weight"])[ids] + q(sd["embeddings.token_type_embeddings.weight"])[tts] + pos[:Lt][None]
        visn = (self.linear(vf, "embeddings.visual_projection") + q(sd["embeddings.visual_token_type_embeddings.weight"])[vtts] +
                q(sd["embeddings.visual_position_embeddings.weight"])[0])
        if image_text_alignment is not None:             # :115-155: mean of the aligned words' positions, -1 pads
            al = torch.as_tensor(image_text_alignment).long()
            valid = (al != -1)
            summed = (pos[al * valid] * valid[..., None].float()).sum(2)
            visn = visn + summed / valid.sum(2).clamp_min(1)[..., None].float()
        return q(self.ln(torch.cat((text, visn), 1), "embeddings.LayerNorm"))

    def forward(self, input_ids, visual_embeds, attention_mask=None, visual_attention_mask=None, token_type_ids=None,
                visual_token_type_ids=None, image_text_alignment=None, return_stages=False):
        x = self.embeddings(input_ids, visual_embeds, token_type_ids, visual_token_type_ids, image_text_alignment)
        B, Lx = x.shape[:2]
        V = np.asarray(visual_embeds).shape[1]
        am = torch.ones((B, Lx - V)) if attention_mask is None else torch.as_tensor(attention_mask).float()
        vm = torch.ones((B, V)) if visual_attention_mask is None else torch.as_tensor(visual_attention_mask).float()
        mask = ((1.0 - torch.cat((am, vm), 1)) * torch.finfo(torch.float32).min)[:, None, None, :]
        st = {"embeddings": x}
        for i in range(self.cfg["num_hidden_layers"]):
            x = self.bert_layer(x, mask, f"encoder.layer.{i}")
        out = (x, self.linear(x[:, 0], "pooler.dense", act="tanh"))
        return (out, st) if return_stages else out

    def qa_forward(self, input_ids, visual_embeds, attention_mask=None, **kw):
        """State dict with the `visual_bert.` prefix and `cls.*`: cls(sequence_output[b, attention_mask.sum(1) - 2])."""
        full = self.sd
        self.sd = {k[len("visual_bert."):]: v for k, v in full.items() if k.startswith("visual_bert.")}
        try:
            seq, _ = self.forward(input_ids, visual_embeds, attention_mask=attention_mask, **kw)
        finally:
            self.sd = full
        B, Lx, H = seq.shape
        Lt = np.asarray(input_ids).shape[1]
        idx = torch.full((B,), Lt - 2) if attention_mask is None else torch.as_tensor(attention_mask).long().sum(1) - 2
        return self.linear(seq[torch.arange(B), idx], "cls")
