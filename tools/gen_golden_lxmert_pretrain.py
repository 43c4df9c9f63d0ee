#!/usr/bin/env python3
"""Golden vectors for LXMERT's pre-training heads and losses from `transformers.LxmertForPreTraining` itself (runs in the build
container only; the tests never import transformers for them).

No checkpoint can be fetched offline, so the model is built from a tiny config with awkward sizes and build-owned seeded weights
(vltk_amd.lxmert_pretrain.make_lxmert_pretraining_state_dict, regenerated from the seed by the tests, never stored) and run on
the CPU in fp32, eval mode, on seeded inputs.  tests/golden/lxmert_pretrain_small.npz holds the config, the `state_dict()` names
and shapes under each task switch, the inputs and labels of every case, every logit tensor, every loss term and the total.

transformers returns the total only; the terms are recomputed here from its own logits with its own loss modules, in its order,
and their sum is asserted to equal its total bit for bit.
"""
import os
import sys

import numpy as np
import torch
from torch.nn import CrossEntropyLoss, SmoothL1Loss

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd.lxmert_pretrain import (lxmert_pretraining_config, lxmert_pretraining_param_spec,  # noqa: E402
                                      make_lxmert_pretraining_state_dict, visual_losses)

SMALL = dict(vocab_size=97, hidden_size=128, num_attention_heads=4, intermediate_size=256, l_layers=1, x_layers=1, r_layers=1,
             max_position_embeddings=16, type_vocab_size=2, visual_feat_dim=32, visual_pos_dim=4, num_qa_labels=11,
             num_object_labels=13, num_attr_labels=7)
CONFIGS = {"A": {}, "B": dict(task_qa=False, visual_attr_loss=False)}
# the state_dict() names and shapes are recorded under these switches too
SPEC_SWITCHES = {"A": {}, "B": CONFIGS["B"], "noobj": dict(task_obj_predict=False), "featonly": dict(visual_obj_loss=False, visual_attr_loss=False),
                 "untied": dict(tie_word_embeddings=False)}
SEED = 2027
B, LT, V = 3, 9, 5
# case -> (config, padded masks?, the labels it passes)
CASES = {"all": ("A", False, ("labels", "matched_label", "obj_labels", "ans")),
         "mlm": ("A", False, ("labels",)),
         "obj": ("A", False, ("obj_labels_zero_conf",)),
         "ans": ("A", False, ("ans_ignored",)),
         "nan": ("A", False, ("labels_none_counted", "matched_label")),
         "switched_off": ("B", False, ("labels", "matched_label", "obj_labels", "ans")),
         "padded": ("A", True, ("labels", "matched_label", "obj_labels", "ans"))}


def hf_config(cfg):
    from transformers import LxmertConfig
    return LxmertConfig(**cfg)


def draw(cfg):
    g = np.random.Generator(np.random.PCG64(SEED))
    ids = g.integers(1, cfg["vocab_size"], (B, LT))
    tts = g.integers(0, 2, (B, LT))
    feats = (np.maximum(g.standard_normal((B, V, cfg["visual_feat_dim"])), 0) * 2.0).astype(np.float32)
    x1y1 = g.uniform(0, 0.6, (B, V, 2))
    pos = np.concatenate([x1y1, x1y1 + g.uniform(0.05, 0.4, (B, V, 2))], -1).astype(np.float32)
    amask = np.ones((B, LT), np.float32)
    amask[1, 6:] = 0
    amask[2, 3:] = 0
    vmask = np.ones((B, V), np.float32)
    vmask[0, 3:] = 0
    labels = np.where(g.uniform(size=(B, LT)) < 0.4, g.integers(0, cfg["vocab_size"], (B, LT)), -100)
    labels[0, 0], labels[0, 1], labels[2, LT - 1] = 0, cfg["vocab_size"] - 1, -100          # both ends of the table
    obj = {"obj": (g.integers(0, cfg["num_object_labels"], (B, V)), g.uniform(0, 1, (B, V)).astype(np.float32)),
           "attr": (g.integers(0, cfg["num_attr_labels"], (B, V)), g.uniform(0, 1, (B, V)).astype(np.float32)),
           # targets up to about +-3 around predictions of about +-1: both branches of SmoothL1
           "feat": ((g.standard_normal((B, V, cfg["visual_feat_dim"])) * 1.5).astype(np.float32), (g.uniform(size=(B, V)) < 0.5).astype(np.float32))}
    obj["obj"][0][0, 0], obj["obj"][0][0, 1], obj["attr"][0][1, 2] = 0, cfg["num_object_labels"] - 1, -100
    zero = {k: (lab, np.zeros_like(conf) if k == "attr" else conf) for k, (lab, conf) in obj.items()}
    return dict(input_ids=ids, token_type_ids=tts, visual_feats=feats, visual_pos=pos, attention_mask=amask, visual_attention_mask=vmask,
                labels=labels, labels_none_counted=np.full((B, LT), -100), matched_label=np.asarray([1, 0, 1]),
                ans=np.asarray([3, cfg["num_qa_labels"] - 1, 0]), ans_ignored=np.asarray([5, -100, 10]), obj_labels=obj,
                obj_labels_zero_conf=zero)


ALIAS = {"ans_ignored": "ans", "labels_none_counted": "labels", "obj_labels_zero_conf": "obj_labels"}


def label_kwargs(inp, names):
    """The label keyword arguments of one case: the input `ans_ignored` is passed as `ans`, and so on."""
    return {ALIAS.get(n, n): inp[n] for n in names}


def terms_of(cfg, out, visual, kw):
    """The loss terms from transformers' own logits, with its loss modules and its expressions (:1064-1095)."""
    ce, ce_rows, l2 = CrossEntropyLoss(), CrossEntropyLoss(reduction="none"), SmoothL1Loss(reduction="none")
    t = {}
    if "labels" in kw and cfg["task_mask_lm"]:
        t["mlm"] = ce(out.prediction_logits.view(-1, cfg["vocab_size"]), kw["labels"].view(-1))
    if "matched_label" in kw and cfg["task_matched"]:
        t["matched"] = ce(out.cross_relationship_score.view(-1, 2), kw["matched_label"].view(-1))
    if "obj_labels" in kw and cfg["task_obj_predict"]:
        for key, n in visual_losses(cfg):
            label, conf = kw["obj_labels"][key]
            rows = l2(visual[key].view(-1, n), label.view(-1, n)).mean(1) if key == "feat" else ce_rows(visual[key].view(-1, n), label.view(-1))
            t[key] = (rows * conf.view(-1)).mean() * cfg["visual_loss_normalizer"]
    if "ans" in kw and cfg["task_qa"]:
        t["ans"] = ce(out.question_answering_score.view(-1, cfg["num_qa_labels"]), kw["ans"].view(-1))
    total = torch.full((), 0.0)
    for k in ("mlm", "matched"):
        if k in t:
            total += t[k]
    if any(k in t for k in ("obj", "attr", "feat")):
        v = torch.full((), 0.0)
        for k in ("obj", "attr", "feat"):
            if k in t:
                v += t[k]
        total += v
    if "ans" in t:
        total += t["ans"]
    return t, total


def to_torch(v):
    if isinstance(v, dict):
        return {k: (torch.from_numpy(a), torch.from_numpy(b)) for k, (a, b) in v.items()}
    return torch.from_numpy(v)


def main():
    from transformers import LxmertForPreTraining
    out = {"seed": np.asarray(SEED)}
    out.update({f"cfg/{k}": np.asarray(v) for k, v in SMALL.items()})
    for tag, sw in SPEC_SWITCHES.items():
        c = lxmert_pretraining_config(**SMALL, **sw)
        with torch.device("meta"):
            spec = [(k, tuple(v.shape)) for k, v in LxmertForPreTraining(hf_config(c)).state_dict().items()]
        assert spec == [(k, tuple(s)) for k, s in lxmert_pretraining_param_spec(c)], f"param spec differs from transformers' under {sw}"
        out[f"spec/{tag}/names"] = np.asarray([n for n, _ in spec])
        out[f"spec/{tag}/shapes"] = np.asarray([tuple(s) + (0,) * (2 - len(s)) for _, s in spec], np.int64)
        out.update({f"spec/{tag}/switch/{k}": np.asarray(v) for k, v in sw.items()})

    models = {}
    for name, sw in CONFIGS.items():
        c = lxmert_pretraining_config(**SMALL, **sw)
        hf = LxmertForPreTraining(hf_config(c)).eval()
        hf.load_state_dict({k: torch.from_numpy(v) for k, v in make_lxmert_pretraining_state_dict(c, SEED).items()}, strict=True)
        assert hf.cls.predictions.decoder.weight.data_ptr() == hf.lxmert.embeddings.word_embeddings.weight.data_ptr(), "not tied"
        models[name] = (c, hf)
        out.update({f"config/{name}/{k}": np.asarray(v) for k, v in sw.items()})

    inp = draw(models["A"][0])
    for k, v in inp.items():
        if isinstance(v, dict):
            for key, (lab, conf) in v.items():
                out[f"in/{k}/{key}/label"], out[f"in/{k}/{key}/conf"] = lab, conf
        else:
            out[f"in/{k}"] = v
    with torch.no_grad():
        for case, (cname, padded, names) in CASES.items():
            c, hf = models[cname]
            kw = dict(input_ids=torch.from_numpy(inp["input_ids"]), visual_feats=torch.from_numpy(inp["visual_feats"]),
                      visual_pos=torch.from_numpy(inp["visual_pos"]))
            if padded:
                kw.update({k: torch.from_numpy(inp[k]) for k in ("attention_mask", "visual_attention_mask", "token_type_ids")})
            lab = {k: to_torch(v) for k, v in label_kwargs(inp, names).items()}
            grabbed = []
            hook = hf.obj_predict_head.register_forward_hook(lambda mod, args, output: grabbed.append(output))
            o = hf(**kw, **lab, return_dict=True)
            if not grabbed:                                    # upstream runs the visual head only when obj_labels is given
                hf.obj_predict_head(hf.lxmert(**kw)[1])
            hook.remove()
            visual = grabbed[0]
            terms, total = terms_of(c, o, visual, lab)
            assert (o.loss is None) == (not lab)
            assert torch.equal(o.loss, total) or (torch.isnan(o.loss) and torch.isnan(total)), (case, o.loss, total)
            out[f"case/{case}/config"], out[f"case/{case}/padded"] = np.asarray(cname), np.asarray(padded)
            out[f"case/{case}/labels"] = np.asarray(list(names))
            out[f"case/{case}/loss"] = o.loss.numpy()
            out.update({f"case/{case}/loss/{k}": v.numpy() for k, v in terms.items()})
            logits = {"prediction_logits": o.prediction_logits, "cross_relationship_score": o.cross_relationship_score}
            if c["task_qa"]:
                logits["question_answering_score"] = o.question_answering_score
            logits.update({f"visual/{k}": v for k, v in visual.items()})
            tag = f"logits/{cname}/{'padded' if padded else 'plain'}"       # the logits do not depend on the labels: stored once
            for k, v in logits.items():
                assert np.array_equal(out.setdefault(f"{tag}/{k}", v.numpy()), v.numpy())
            print(case, "loss", float(o.loss), {k: round(float(v), 5) for k, v in terms.items()})
    assert np.isnan(out["case/nan/loss"]) and np.isnan(out["case/nan/loss/mlm"]) and out["case/obj/loss/attr"] == 0
    path = os.path.join(ROOT, "tests", "golden", "lxmert_pretrain_small.npz")
    np.savez_compressed(path, **out)
    print("lxmert_pretrain_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
