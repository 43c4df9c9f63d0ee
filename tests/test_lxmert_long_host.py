"""CPU: the LXMERT oracle against transformers.LxmertModel's vectors at 40 text and 140 visual tokens (tests/golden/lxmert_long.npz,
tools/gen_golden_lxmert_long.py), the reference of the GPU tests of the long-sequence attention kernels."""
import os

import numpy as np
import pytest

from oracle.lxmert_oracle import LxmertOracle

from lxmert_util import case_kwargs, golden_inputs


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lxmert_long.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-9)


def test_fixture_geometry(g):
    cfg, _, feats = golden_inputs(g)
    assert cfg["hidden_size"] // cfg["num_attention_heads"] == 64
    assert g["input_ids"].shape == (2, 40) and feats.shape == (2, 140, 256)
    # both masks ragged
    assert sorted(g["attention_mask"].sum(1).tolist()) == [17, 33] and sorted(g["visual_attention_mask"].sum(1).tolist()) == [70, 131]


@pytest.mark.parametrize("tag", ["masked", "plain"])
def test_oracle_vs_transformers_golden_long(g, tag):
    cfg, sd, feats = golden_inputs(g)
    lang, visn, pooled = LxmertOracle(cfg, sd).forward(g["input_ids"], feats, g["visual_pos"], **case_kwargs(g, tag))
    assert rel(lang, g[f"{tag}/language_output"]) <= 1e-5
    assert rel(visn, g[f"{tag}/vision_output"]) <= 1e-5
    assert rel(pooled, g[f"{tag}/pooled_output"]) <= 1e-5
