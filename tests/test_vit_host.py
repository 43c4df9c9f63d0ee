"""CPU: the ViT oracle (tests/vit_util.py) against vectors produced by transformers.ViTModel / ViTForImageClassification
themselves, the build's parameter specs against those classes' state_dict, the hub-era key names, and the host-side pieces of
vltk_amd/vit.py that run before any library call."""
import os
import re

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd import vit as V

from vit_util import CASES, ViTOracle, golden_case, golden_classifier, golden_model, hub_era_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(hidden_size=32, num_attention_heads=2, intermediate_size=64, num_hidden_layers=2, image_size=16, patch_size=8)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "vit_small.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-9)


# ---- the oracle against transformers' vectors --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_oracle_vs_transformers_golden(g, case):
    """Every stored output to 1e-5, the interpolated position tables of `tall` and `long` included."""
    name, pix, interp = golden_case(g, case)
    cfg, sd = golden_model(g, name)
    (seq, pooled), st = ViTOracle(cfg, sd).forward(pix, interp, return_stages=True)
    assert rel(st["embeddings"], g[f"{case}/embedding_output"]) <= 1e-5
    assert rel(seq, g[f"{case}/last_hidden_state"]) <= 1e-5
    if name == "main":
        assert rel(pooled, g[f"{case}/pooler_output"]) <= 1e-5
        ccfg, csd, _ = golden_classifier(g)
        assert rel(ViTOracle(ccfg, csd).classify(pix, interp), g[f"{case}/logits"]) <= 1e-5


def test_golden_cases_exercise_what_they_claim(g):
    """17, 19 (gh != gw) and 65 tokens from the 4 x 4-grid model, two of them through interpolated tables that differ from the
    trained one; 7 tokens from 14-pixel patches whose 588 columns are no K-tile multiple."""
    shapes = {c: g[f"{c}/last_hidden_state"].shape for c in CASES}
    assert shapes == {"square": (2, 17, 128), "tall": (2, 19, 128), "long": (2, 65, 128), "p14": (2, 7, 128)}
    assert g["tall/pixel_values"].shape == (2, 3, 48, 24) and g["p14/pixel_values"].shape == (2, 3, 28, 42)
    assert [bool(g[f"{c}/interpolate_pos_encoding"]) for c in CASES] == [False, True, True, False]
    cfg, sd = golden_model(g, "main")
    assert V.vit_grid(cfg) == (4, 4, 8)
    pos = sd["embeddings.position_embeddings"][0]
    tall = V.interpolate_position_table(pos, (4, 4), (6, 3))
    assert tall.shape == (19, 128) and torch.equal(tall[0], torch.from_numpy(pos[0]))
    assert torch.equal(V.interpolate_position_table(pos, (4, 4), (4, 4)), torch.from_numpy(pos))      # the table as loaded
    pcfg, _ = golden_model(g, "p14")
    assert V.vit_grid(pcfg) == (2, 3, 14) and 3 * 14 * 14 == 588 and 588 % 32 and 588 % 64


@pytest.mark.parametrize("emulate,tol", [("bf16", 6e-2), ("fp16", 1e-2)])
def test_emulation_stays_near_fp32(g, emulate, tol):
    """Storage roundings through the embeddings and two layers stay within the bound the LXMERT and VisualBERT oracles'
    emulation is held to."""
    name, pix, interp = golden_case(g, "long")
    cfg, sd = golden_model(g, name)
    seq, pooled = ViTOracle(cfg, sd, emulate=emulate).forward(pix, interp)
    assert rel(seq, g["long/last_hidden_state"]) <= tol and rel(pooled, g["long/pooler_output"]) <= tol


# ---- parameter specs, seeded weights, key names --------------------------------------------------------------------------------
def test_param_spec_matches_transformers():
    tr = pytest.importorskip("transformers")
    for kw in (SMALL, {}, dict(SMALL, image_size=(28, 42), patch_size=14), dict(SMALL, num_channels=1)):
        cfg = V.vit_config(**kw)
        with torch.device("meta"):
            m = tr.ViTModel(tr.ViTConfig(**cfg))
            bare = tr.ViTModel(tr.ViTConfig(**cfg), add_pooling_layer=False)
            c = tr.ViTForImageClassification(tr.ViTConfig(num_labels=10, **cfg))
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in V.vit_param_spec(cfg)]
        assert [(k, tuple(v.shape)) for k, v in bare.state_dict().items()] == [(k, tuple(s)) for k, s in V.vit_param_spec(cfg, False)]
        assert [(k, tuple(v.shape)) for k, v in c.state_dict().items()] == [(k, tuple(s)) for k, s in V.vit_classifier_param_spec(cfg, 10)]


def test_config_defaults_and_refusals():
    cfg = V.vit_config()
    assert (cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"]) == (768, 12, 12, 3072)
    assert (cfg["image_size"], cfg["patch_size"], cfg["num_channels"], cfg["layer_norm_eps"], cfg["hidden_act"], cfg["qkv_bias"]) == \
        (224, 16, 3, 1e-12, "gelu", True)
    assert V.vit_grid(cfg) == (14, 14, 16)
    h14 = V.vit_config("H/14")
    assert (h14["hidden_size"], h14["num_hidden_layers"], h14["num_attention_heads"], h14["intermediate_size"], h14["patch_size"]) == \
        (1280, 32, 16, 5120, 14)
    assert V.vit_grid(V.vit_config(image_size=(48, 32), patch_size=(16, 16))) == (3, 2, 16)
    for kw in (dict(hidden_act="relu"), dict(qkv_bias=False), dict(patch_size=(16, 8))):
        with pytest.raises(NotImplementedError):
            V.vit_config(**kw)
    for kw in (dict(image_size=30), dict(image_size=(32, 8), patch_size=16), dict(num_channels=5)):
        with pytest.raises(ValueError):
            V.vit_config(**kw)


def test_synthetic_weights_are_seeded_per_tensor():
    cfg = V.vit_config(**SMALL)
    a, b, c = V.make_vit_state_dict(cfg, 3), V.make_vit_state_dict(cfg, 3), V.make_vit_state_dict(cfg, 4)
    assert list(a) == [k for k, _ in V.vit_param_spec(cfg)]
    assert all(np.array_equal(a[k], b[k]) and a[k].shape == tuple(s) for k, s in V.vit_param_spec(cfg))
    assert not np.array_equal(a["pooler.dense.weight"], c["pooler.dense.weight"])
    gammas = [k for k in a if re.search(r"layernorm(_before|_after)?\.weight$", k)]
    assert len(gammas) == 2 * cfg["num_hidden_layers"] + 1
    for k in gammas:                                       # the gamma draw, U(0.5, 1.5), and a draw of its own per tensor
        assert 0.5 <= a[k].min() and a[k].max() <= 1.5
    assert not np.array_equal(a["layers.0.layernorm_before.weight"], a["layers.0.layernorm_after.weight"])
    assert np.abs(a["layers.0.layernorm_before.bias"]).max() < 0.5
    cl = V.make_vit_classifier_state_dict(cfg, 7, 3)
    assert list(cl) == [k for k, _ in V.vit_classifier_param_spec(cfg, 7)] and cl["classifier.weight"].shape == (7, 32)
    assert np.array_equal(cl["vit.layers.1.mlp.fc1.weight"], a["layers.1.mlp.fc1.weight"])
    assert np.array_equal(cl["vit.layernorm.weight"], a["layernorm.weight"])


def test_hub_era_names_rename_to_the_same_tensors():
    cfg = V.vit_config(**SMALL)
    sd = V.make_vit_state_dict(cfg, 5)
    hub = hub_era_names(sd)
    assert "encoder.layer.1.attention.attention.query.weight" in hub and "encoder.layer.0.layernorm_after.bias" in hub
    assert "encoder.layer.0.output.dense.weight" in hub and not any(k.startswith("layers.") for k in hub)
    back = V.rename_hub_keys(hub)
    assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
    csd = V.make_vit_classifier_state_dict(cfg, 4, 5)
    cback = V.rename_hub_keys(hub_era_names(csd, "vit."), prefix="vit.")
    assert set(cback) == set(csd) and all(cback[k] is csd[k] for k in csd)
    same = V.rename_hub_keys(sd)                           # current names pass through
    assert list(same) == list(sd) and all(same[k] is sd[k] for k in sd)
    with pytest.raises(RuntimeError):                     # both spellings of one tensor
        V.rename_hub_keys(dict(hub, **{"layers.0.mlp.fc1.weight": sd["layers.0.mlp.fc1.weight"]}))


def test_strict_load_refuses_stray_and_missing_keys_after_renaming():
    """BertOps._check_state_dict is what load_state_dict runs on the renamed keys; it needs no GPU."""
    cfg = V.vit_config(**SMALL)
    sd = V.make_vit_state_dict(cfg, 5)
    want = dict(V.vit_param_spec(cfg))
    check = V.ViTModel._check_state_dict
    model = object.__new__(V.ViTModel)
    check(model, V.rename_hub_keys(hub_era_names(sd)), want, True)
    with pytest.raises(RuntimeError, match="unexpected"):
        check(model, V.rename_hub_keys(dict(hub_era_names(sd), **{"encoder.layer.0.attention.attention.extra.weight": sd["layernorm.weight"]})),
              want, True)
    short = hub_era_names(sd)
    del short["encoder.layer.1.intermediate.dense.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        check(model, V.rename_hub_keys(short), want, True)
    bad = dict(sd, **{"layernorm.weight": np.zeros(33, np.float32)})
    with pytest.raises(RuntimeError, match="shape"):
        check(model, bad, want, True)


# ---- host helpers -----------------------------------------------------------------------------------------------------------------
def test_patch_boxes_by_hand():
    b = V.vit_patch_boxes(28, 42, 14)
    assert b.dtype == np.float32 and b.tolist() == [[0, 0, 14, 14], [14, 0, 28, 14], [28, 0, 42, 14],
                                                    [0, 14, 14, 28], [14, 14, 28, 28], [28, 14, 42, 28]]
    n = V.vit_patch_boxes(28, 42, 14, normalized=True)
    want = np.asarray([[0, 0, 1 / 3, 0.5], [1 / 3, 0, 2 / 3, 0.5], [2 / 3, 0, 1, 0.5],
                       [0, 0.5, 1 / 3, 1], [1 / 3, 0.5, 2 / 3, 1], [2 / 3, 0.5, 1, 1]], np.float32)
    assert n.dtype == np.float32 and np.abs(n - want).max() <= 1e-7
    assert V.vit_patch_boxes(224, 224, 16).shape == (196, 4)
    for bad in ((28, 40, 14), (0, 14, 14), (28, 42, 0)):
        with pytest.raises(ValueError):
            V.vit_patch_boxes(*bad)


def test_patch_tokens_drops_the_class_row():
    seq = torch.arange(2 * 5 * 3, dtype=torch.float32).view(2, 5, 3)
    t = V.patch_tokens(seq)
    assert t.shape == (2, 4, 3) and torch.equal(t, seq[:, 1:]) and t.dtype == seq.dtype
    with pytest.raises(ValueError):
        V.patch_tokens(seq[0])
    with pytest.raises(ValueError):
        V.patch_tokens(seq[:, :1])


def test_pixel_values_are_checked_on_the_host():
    """Rank, channel count, a side that is no multiple of the patch, and transformers' own error for another size without
    interpolate_pos_encoding: all before any library call (these functions never load the library)."""
    cfg = V.vit_config(**dict(SMALL, image_size=32))
    assert V.check_pixel_values(torch.zeros(2, 3, 32, 32), cfg) == (2, 4, 4)
    assert V.check_pixel_values(np.zeros((1, 3, 48, 24), np.float32), cfg, interpolate_pos_encoding=True) == (1, 6, 3)
    for bad in (torch.zeros(3, 32, 32), torch.zeros(2, 1, 32, 32), torch.zeros(2, 3, 32, 36), torch.zeros(2, 3, 4, 32),
                torch.zeros(0, 3, 32, 32)):
        with pytest.raises(ValueError):
            V.check_pixel_values(bad, cfg, interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="doesn't match model"):
        V.check_pixel_values(torch.zeros(2, 3, 64, 64), cfg)
    with pytest.raises(ValueError, match="not square"):
        V.interpolate_position_table(np.zeros((7, 8), np.float32), (2, 3), (4, 4))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW = ("vk_vit_patchify", "vk_vit_assemble")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} not declared"
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 10
        assert hasattr(L.load(), name), f"{name} not exported"
    mk = open(os.path.join(ROOT, "vltk_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/vit.o" in mk
    nofma = re.search(r"\$\(if \$\(filter ([^,]*),\$\*\),\$\(NOFMA\)\)", mk).group(1).split()
    hazsrc = re.search(r"^HAZSRC\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "vit" not in nofma and "vit.hip" not in hazsrc


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """The size checks come before anything touches a device, so they answer on a machine without one (pointers are never
    dereferenced on the host)."""
    lib, p = L.load(), 4096

    def patchify(B=2, C=3, Hi=28, Wi=42, P=14, ldk=608, dt=L.VK_F32, rows=p):
        return lib.vk_vit_patchify(p, B, C, Hi, Wi, P, rows, ldk, dt, None)
    for bad in (dict(B=0), dict(P=0), dict(C=0), dict(C=5), dict(Hi=30), dict(Wi=0), dict(Hi=0), dict(ldk=587), dict(ldk=590),
                dict(ldk=588, dt=L.VK_F16), dict(dt=L.VK_I32), dict(rows=p + 4), dict(rows=None),
                dict(B=1 << 20, Hi=64 * 14, Wi=64 * 14)):                       # 2^32 rows
        assert patchify(**bad) == L.VK_EINVAL, bad
    with pytest.raises(ValueError, match="vit_patchify"):
        L.call("vk_vit_patchify", p, 2, 3, 30, 42, 14, p, 608, L.VK_F32, None)

    def assemble(B=2, N=6, H=128, ldp=136, dt=L.VK_BF16, proj=p):
        return lib.vk_vit_assemble(proj, ldp, p, p, B, N, p, H, dt, None)
    for bad in (dict(B=0), dict(N=0), dict(H=0), dict(ldp=127), dict(dt=L.VK_I64), dict(proj=None), dict(B=1 << 16, N=1 << 15)):
        assert assemble(**bad) == L.VK_EINVAL, bad


def test_lazy_exports():
    import vltk_amd
    assert vltk_amd.ViTModel is V.ViTModel and vltk_amd.ViTForImageClassification is V.ViTForImageClassification
    assert vltk_amd.patch_tokens is V.patch_tokens and vltk_amd.vit_patch_boxes is V.vit_patch_boxes and vltk_amd.vit_config is V.vit_config
