"""TEST INFRASTRUCTURE ONLY -- tests/golden/layoutlmv3_small.npz (tools/gen_golden_layoutlmv3_model.py): its models rebuilt from
the seed, the keyword arguments of each stored case and the `state_dict()` specs transformers recorded."""
from vltk_amd import layoutlmv3 as V3

CASES = [(geo, case) for geo in ("short", "long") for case in ("plain", "masked", "textonly")]
HEADS = {"token5": "token", "token12": "token", "qa": "qa", "seq": "seq"}


def golden_cfg(g):
    return V3.layoutlmv3_config(**{k[4:]: int(g[k]) for k in g.files if k.startswith("cfg/")})


def golden_state_dict(g, head=None):
    """-> (cfg, num_labels or None, state dict) of the bare model, or of one stored head ("token5" | "token12" | "qa" | "seq")."""
    cfg = golden_cfg(g)
    if head is None:
        return cfg, None, V3.make_layoutlmv3_state_dict(cfg, int(g["seed"]))
    n = int(g[f"{head}/num_labels"])
    return cfg, n, V3.make_layoutlmv3_head_state_dict(cfg, HEADS[head], n, int(g["seed"]))


def case_kwargs(g, geo, case):
    """Every keyword argument of the stored case `<geo>/<case>` (numpy arrays), input_ids included."""
    kw = dict(input_ids=g[f"{geo}/input_ids"], bbox=g[f"{geo}/bbox"])
    if case == "masked":
        kw.update(input_ids=g[f"{geo}/input_ids_masked"], attention_mask=g[f"{geo}/attention_mask"], token_type_ids=g[f"{geo}/token_type_ids"])
    if case != "textonly":
        kw["pixel_values"] = g[f"{geo}/pixel_values"]
    return kw


def stored_spec(g, tag, which):
    """The `state_dict()` names and shapes recorded from transformers: tag "small" | "default", which "model" | a head."""
    names, shapes = g[f"spec/{tag}/{which}/names"], g[f"spec/{tag}/{which}/shapes"]
    return [(str(n), tuple(int(v) for v in s if v)) for n, s in zip(names, shapes)]
