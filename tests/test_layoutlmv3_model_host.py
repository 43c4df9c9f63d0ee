"""CPU (-m "not gpu"): the host side of LayoutLMv3Model against what transformers recorded in tests/golden/layoutlmv3_small.npz
(state-dict names and shapes, `create_visual_bbox`), and the refusals that come before any launch."""
import os

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import layoutlmv3 as V3

from layoutlmv3_util import HEADS, golden_cfg, stored_spec


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "layoutlmv3_small.npz"))


@pytest.mark.parametrize("tag", ["small", "default"])
def test_param_specs_are_transformers_state_dicts(g, tag):
    cfg = golden_cfg(g) if tag == "small" else V3.layoutlmv3_config()
    assert [(k, tuple(s)) for k, s in V3.layoutlmv3_param_spec(cfg)] == stored_spec(g, tag, "model")
    for head, kind in HEADS.items():
        n = int(g[f"{head}/num_labels"])
        assert [(k, tuple(s)) for k, s in V3.layoutlmv3_head_param_spec(cfg, kind, n)] == stored_spec(g, tag, head)
        assert set(V3.make_layoutlmv3_head_state_dict(golden_cfg(g), kind, n)) == {k for k, _ in stored_spec(g, "small", head)}


@pytest.mark.parametrize("grid", [2, 14])
def test_visual_bbox_is_create_visual_bbox(g, grid):
    assert np.array_equal(V3.visual_bbox(grid, grid), g[f"vbox/{grid}"])


def _inputs(cfg, Lt=6):
    ids = torch.arange(2, 2 + 2 * Lt).view(2, Lt)
    box = torch.tensor([10, 20, 30, 40]).expand(2, Lt, 4).clone()
    return dict(input_ids=ids, bbox=box, attention_mask=torch.ones(2, Lt), token_type_ids=torch.zeros(2, Lt, dtype=torch.long),
                pixel_values=torch.zeros(2, 3, cfg["input_size"], cfg["input_size"]))


def _set(t, index, value):
    t = t.clone()
    t[index] = value
    return t


REFUSALS = {
    "id past the vocabulary": lambda kw, cfg: dict(kw, input_ids=_set(kw["input_ids"], (0, 1), cfg["vocab_size"])),
    "token type past its table": lambda kw, cfg: dict(kw, token_type_ids=_set(kw["token_type_ids"], (0, 0), cfg["type_vocab_size"])),
    "coordinate past the 2-D tables": lambda kw, cfg: dict(kw, bbox=_set(kw["bbox"], (0, 0, 2), cfg["max_2d_position_embeddings"])),
    "x1 < x0": lambda kw, cfg: dict(kw, bbox=_set(kw["bbox"], (1, 2, 2), 9)),
    "y1 < y0": lambda kw, cfg: dict(kw, bbox=_set(kw["bbox"], (1, 2, 3), 19)),
    "mask of another shape": lambda kw, cfg: dict(kw, attention_mask=torch.ones(2, 5)),
    "image of another size": lambda kw, cfg: dict(kw, pixel_values=torch.zeros(2, 3, 2 * cfg["input_size"], 2 * cfg["input_size"])),
    "image without text": lambda kw, cfg: dict(kw, input_ids=None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_host_check_refuses(g, what):
    cfg = golden_cfg(g)
    kw = _inputs(cfg)
    V3.check_layoutlmv3_inputs(cfg, **kw)                  # the inputs themselves pass
    with pytest.raises(ValueError):
        V3.check_layoutlmv3_inputs(cfg, **REFUSALS[what](kw, cfg))


def test_position_past_the_table_is_refused_by_count_not_by_length(g):
    """80 positions, pad 1: 78 non-pad tokens end at position 79 and pass, 79 do not; 79 tokens of which one is a pad pass."""
    cfg = golden_cfg(g)
    full = torch.full((1, 79), 5)
    V3.check_layoutlmv3_inputs(cfg, full[:, :78])
    V3.check_layoutlmv3_inputs(cfg, _set(full, (0, 40), cfg["pad_token_id"]))
    with pytest.raises(ValueError, match="position id 80"):
        V3.check_layoutlmv3_inputs(cfg, full)


def test_config_and_form_refuse_a_split_that_is_not_the_row():
    with pytest.raises(ValueError):
        V3.layoutlmv3_config(hidden_size=64, num_attention_heads=2, coordinate_size=8, shape_size=8)
    assert L.load().vk_layoutlmv3_embed_form(64, 8, 8, L.VK_F32, 1) == -L.VK_EINVAL
    with pytest.raises(ValueError):
        V3.embed_form(64, 8, 8, torch.float32)
    assert V3.embed_form(128, 16, 32, torch.bfloat16) == "vector" and V3.embed_form(128, 16, 32, torch.bfloat16, aligned16=False) == "scalar"
    assert V3.embed_form(136, 18, 32, torch.float32) == "scalar"      # an aligned row with an unaligned segment
