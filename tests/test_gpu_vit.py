"""-m gpu: the Vision Transformer on the HIP path (vltk_amd.ViTModel / ViTForImageClassification -> C ABI) against
(a) torch, for the two new kernels (vk_vit_patchify, vk_vit_assemble) alone,
(b) vectors produced by transformers.ViTModel / ViTForImageClassification themselves (fp32 strict mode, the bounds of test_gpu_visualbert.py),
(c) the oracle restating the bf16 / fp16 storage roundings (tests/vit_util.py), with the launches and the attention kernel asserted,
then graph replay, the hand-over to VisualBertModel and one forward at ViT-B/16 size."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                          # noqa: E402
from vltk_amd import visualbert as VB                                                   # noqa: E402
from vltk_amd import vit as V                                                           # noqa: E402

import gpu_util as G                                                                    # noqa: E402
from vit_util import CASES, ViTOracle, golden_case, golden_classifier, golden_model, hub_era_names    # noqa: E402

TDT = G.TDT
EPS = {L.VK_F32: 2e-5, L.VK_F16: 1e-3, L.VK_BF16: 8e-3}          # one rounding of the storage type (+ margin): test_gpu_visualbert.py's
IDS = ["fp32", "fp16", "bf16"]
DTS = [L.VK_F32, L.VK_F16, L.VK_BF16]
ES = {L.VK_F32: 4, L.VK_F16: 2, L.VK_BF16: 2}


def rel(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b).float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-9))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "vit_small.npz"))


@pytest.fixture(scope="module")
def models(g):
    """One model per (fixture model, precision), shared by the tests of this module."""
    cache = {}

    def get(name, precision):
        if (name, precision) not in cache:
            cfg, sd = golden_model(g, name)
            cache[name, precision] = V.ViTModel(cfg, precision=precision).load_state_dict(sd)
        return cache[name, precision]
    return get


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------
def run_patchify(pix, B, C, Hi, Wi, P, ldk, dt, rows=None):
    n = B * (Hi // max(P, 1)) * (Wi // max(P, 1)) if rows is None else rows
    y = torch.full((n + 1, ldk), 77.0, dtype=TDT[dt], device=G.DEV)                    # one guard row behind the output
    L.call("vk_vit_patchify", G.P(pix), B, C, Hi, Wi, P, G.P(y), ldk, dt, G.stream())
    torch.cuda.synchronize()
    assert (y[n].float() == 77.0).all(), "the launch wrote behind its last row"
    return y[:n]


@pytest.mark.parametrize("Hi,Wi,P,extra", [(28, 42, 14, 0), (32, 48, 16, 1)], ids=["28x42p14", "32x48p16"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_patchify_kernel_is_a_gather_plus_one_rounding(dt, Hi, Wi, P, extra):
    """Exactly F.unfold(...).transpose rounded to the storage type: 14-pixel patches (588 columns, rows of the image that are not
    16-byte aligned: the per-element form) and 16-pixel ones (float4 loads; one K-tile of padding added, 768 columns being a
    whole number of tiles).  The padding columns are written as zero over a buffer filled with 77."""
    B, C = 3, 3
    gen = np.random.Generator(np.random.PCG64(P))
    pix = torch.from_numpy(gen.standard_normal((B, C, Hi, Wi)).astype(np.float32))
    K, ktile = C * P * P, 128 // ES[dt]
    ldk = (K + ktile - 1) // ktile * ktile + extra * ktile
    assert ldk > K
    y = run_patchify(pix.to(G.DEV), B, C, Hi, Wi, P, ldk, dt).cpu()
    ref = F.unfold(pix, P, stride=P).transpose(1, 2).reshape(-1, K).to(TDT[dt])
    assert y.shape == (B * (Hi // P) * (Wi // P), ldk)
    assert torch.equal(y[:, :K], ref)
    assert (y[:, K:].float() == 0).all(), "a padding column the GEMM reads is not zero"


def assemble_case(dt, H, split_ranges=False):
    """Inputs of one vk_vit_assemble launch (B = 3, N = 20; proj rows 8 elements wider than H, 1000.0 in the padding) and its torch
    reference.  split_ranges: the class token in [1, 2], the projected patches in [-2, -1], positions within +-0.25 -- the sign of
    an output row tells which kind of row it is."""
    gen = np.random.Generator(np.random.PCG64(H + int(split_ranges)))
    td = TDT[dt]
    B, N, ldp = 3, 20, H + 8
    if split_ranges:
        cls = torch.from_numpy(gen.uniform(1.0, 2.0, H).astype(np.float32)).to(td)
        proj = torch.from_numpy(gen.uniform(-2.0, -1.0, (B * N, H)).astype(np.float32)).to(td)
        pos = torch.from_numpy(gen.uniform(-0.25, 0.25, (N + 1, H)).astype(np.float32)).to(td)
    else:
        cls, proj, pos = (torch.from_numpy(gen.standard_normal(s).astype(np.float32)).to(td) for s in ((H,), (B * N, H), (N + 1, H)))
    projw = torch.full((B * N, ldp), 1000.0, dtype=td)                                # the padding columns must never be read
    projw[:, :H] = proj
    ref = (torch.cat((cls.float().expand(B, 1, H), proj.float().view(B, N, H)), 1) + pos.float()[None]).to(td).float().view(-1, H)
    dev = {k: v.to(G.DEV) for k, v in dict(proj=projw, cls=cls, pos=pos).items()}
    return dict(B=B, N=N, H=H, ldp=ldp, td=td, dt=dt), dev, ref


def run_assemble(geo, d):
    rows = max(geo["B"], 1) * (max(geo["N"], 0) + 1)
    x = torch.full((rows + 1, max(geo["H"], 1)), 77.0, dtype=geo["td"], device=G.DEV)  # one guard row behind the output
    L.call("vk_vit_assemble", G.P(d["proj"]), geo["ldp"], G.P(d["cls"]), G.P(d["pos"]), geo["B"], geo["N"], G.P(x), geo["H"], geo["dt"],
           G.stream())
    torch.cuda.synchronize()
    assert (x[rows].float() == 77.0).all(), "the launch wrote behind its last row"
    return x[:rows]


@pytest.mark.parametrize("H", [128, 100], ids=["vec128", "scalar100"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_assemble_kernel_vs_torch(dt, H):
    """cls + pos[0] | proj + pos[1 + n], fp32 sum and one rounding: the 16-byte-chunk form (H = 128) and the scalar form
    (H = 100), 63 rows over several workgroups."""
    geo, dev, ref = assemble_case(dt, H)
    err = rel(run_assemble(geo, dev), ref)
    print(f"\n[vk_vit_assemble {IDS[DTS.index(dt)]} H={H}] rel err {err:.2e}")
    assert err <= EPS[dt]


@pytest.mark.parametrize("H", [128, 100], ids=["vec128", "scalar100"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_assemble_rows_land_in_sequence_order(dt, H):
    """The class row at b * (N + 1), patch n at b * (N + 1) + 1 + n: the two kinds of row are drawn from disjoint value ranges."""
    geo, dev, ref = assemble_case(dt, H, split_ranges=True)
    x = run_assemble(geo, dev).float().cpu().view(geo["B"], geo["N"] + 1, H)
    assert (x[:, 0] > 0.5).all(), "a class position holds something else"
    assert (x[:, 1:] < -0.5).all(), "a patch position holds something else"
    assert rel(x.view(-1, H), ref) <= EPS[dt]


def test_entries_refuse_bad_sizes():
    pix = torch.zeros((3, 3, 28, 42), device=G.DEV)
    ok = dict(B=3, C=3, Hi=28, Wi=42, P=14, ldk=608, dt=L.VK_F32)
    run_patchify(pix, **ok)
    for patch in (dict(B=0), dict(P=0), dict(C=0), dict(C=5), dict(Hi=30), dict(Wi=40), dict(Hi=0), dict(ldk=587), dict(ldk=590),
                  dict(ldk=596, dt=L.VK_BF16), dict(ldk=588, dt=L.VK_F16)):
        with pytest.raises(ValueError):
            run_patchify(pix, rows=18, **dict(ok, **patch))
    with pytest.raises(ValueError):                       # 2^20 images of 64 x 64 patches: 2^32 rows (refused before any launch)
        run_patchify(pix, rows=18, **dict(ok, B=1 << 20, Hi=64 * 14, Wi=64 * 14))
    geo, dev, _ = assemble_case(L.VK_F32, 128)
    run_assemble(geo, dev)
    for patch in (dict(B=0), dict(N=0), dict(H=0), dict(ldp=127), dict(B=1 << 16, N=1 << 15)):
        bad = dict(geo, **patch)
        x = torch.empty((64, 128), device=G.DEV)
        with pytest.raises(ValueError):
            L.call("vk_vit_assemble", G.P(dev["proj"]), bad["ldp"], G.P(dev["cls"]), G.P(dev["pos"]), bad["B"], bad["N"], G.P(x), bad["H"],
                   geo["dt"], G.stream())
    x = torch.full((64, 128), 77.0, device=G.DEV)
    with pytest.raises(ValueError):
        L.call("vk_vit_assemble", G.P(dev["proj"]), geo["ldp"], G.P(dev["cls"]), G.P(dev["pos"]), geo["B"], geo["N"], G.P(x), geo["H"],
               L.VK_I32, G.stream())
    torch.cuda.synchronize()
    assert (x == 77.0).all(), "a refused dtype wrote the output"


# ---- 2. fp32 against transformers' vectors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_model_fp32_vs_transformers_golden(g, models, case):
    name, pix, interp = golden_case(g, case)
    m = models(name, "fp32")
    pix = torch.from_numpy(pix)
    seq, pooled = (t.clone() for t in m(pix, interpolate_pos_encoding=interp))
    emb = m.embeddings(pix, interpolate_pos_encoding=interp)
    errs = [rel(emb, g[f"{case}/embedding_output"]), rel(seq, g[f"{case}/last_hidden_state"])]
    if name == "main":
        errs.append(rel(pooled, g[f"{case}/pooler_output"]))
    print(f"\n[ViT fp32 strict vs transformers, {case}] rel err embeddings {errs[0]:.2e} seq {errs[1]:.2e}"
          + (f" pooled {errs[2]:.2e}" if name == "main" else ""))
    assert errs[0] <= 1e-5
    assert max(errs[1:]) <= 1e-3


@pytest.mark.parametrize("case", ["square", "tall", "long"])
def test_classifier_fp32_vs_transformers_golden(g, case):
    cfg, sd, n = golden_classifier(g)
    _, pix, interp = golden_case(g, case)
    logits = V.ViTForImageClassification(cfg, n, precision="fp32").load_state_dict(sd)(torch.from_numpy(pix), interpolate_pos_encoding=interp)
    stored = g[f"{case}/logits"]
    assert logits.shape == stored.shape
    err = rel(logits, stored)
    print(f"\n[ViTForImageClassification fp32, {case}] rel err {err:.2e}")
    assert err <= 1e-3
    assert logits.float().argmax(-1).cpu().tolist() == stored.argmax(-1).tolist()


def test_hub_era_checkpoint_names_load_to_the_same_model(g, models):
    """The fixture's weights under the key names of published checkpoints give the same bits; a stray key fails the strict load."""
    name, pix, _ = golden_case(g, "square")
    cfg, sd = golden_model(g, name)
    hub = hub_era_names(sd)
    assert "encoder.layer.0.attention.attention.query.weight" in hub and "layers.0.attention.q_proj.weight" not in hub
    want = [t.clone() for t in models(name, "fp32")(torch.from_numpy(pix))]
    got = V.ViTModel(cfg, precision="fp32").load_state_dict(hub)(torch.from_numpy(pix))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="unexpected"):
        V.ViTModel(cfg, precision="fp32").load_state_dict(dict(hub, **{"encoder.layer.0.attention.attention.extra.bias": hub["layernorm.bias"]}))


# ---- 3. reduced precision against the emulating oracle, with the launches asserted ------------------------------------------------
@pytest.mark.parametrize("case,route", [("square", L.VK_ATT_ROUTE_MFMA), ("long", L.VK_ATT_ROUTE_TILED)], ids=["square", "long"])
@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("fp16", 6e-3)])
def test_model_reduced_precision_vs_emulating_oracle(g, models, monkeypatch, precision, tol, case, route):
    name, pix, interp = golden_case(g, case)
    cfg, sd = golden_model(g, name)
    m = models(name, precision)
    Lx, H, heads = g[f"{case}/last_hidden_state"].shape[1], cfg["hidden_size"], cfg["num_attention_heads"]
    entries = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), real(name, *a))[1])
    seq, pooled = m(torch.from_numpy(pix), interpolate_pos_encoding=interp)
    monkeypatch.undo()
    # the entry point each layer's attention went through, and the kernel that entry runs this shape on: q, k and v are column
    # slices of the fused projection's [B * Lx, 3H] output (that row stride, 16-byte aligned)
    want = "vk_attention" if route == L.VK_ATT_ROUTE_MFMA else "vk_attention_tiled"
    assert [e for e in entries if e.startswith("vk_attention")] == [want] * cfg["num_hidden_layers"]
    assert L.load().vk_attention_route(Lx, Lx, H // heads, m.dt, 3 * H, 3 * H, 3 * H, 1, int(want == "vk_attention_tiled")) == route
    assert entries.count("vk_vit_patchify") == 1 and entries.count("vk_vit_assemble") == 1
    assert entries[0] == "vk_vit_patchify" and entries[1] == "vk_linear" and entries[2] == "vk_vit_assemble"
    assert set(entries) == {"vk_vit_patchify", "vk_vit_assemble", "vk_linear", "vk_layernorm", "vk_conv2d", want}, \
        "a launch outside the ViT path (the text / region embedding kernels, or the other attention entry)"
    o_seq, o_pooled = ViTOracle(cfg, sd, emulate=precision).forward(pix, interp)
    errs = (rel(seq, o_seq), rel(pooled, o_pooled))
    print(f"\n[ViT {precision} vs emulating oracle, {case}] seq {errs[0]:.2e} pooled {errs[1]:.2e};"
          f" vs transformers fp32: seq {rel(seq, g[f'{case}/last_hidden_state']):.2e}")
    assert max(errs) <= tol


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(g, models):
    """One forward captured into a HIP graph replays bit-identically and follows new pixels of the same shape; another shape raises."""
    name, pix, interp = golden_case(g, "long")
    m = models(name, "bf16")
    pix = torch.from_numpy(pix)
    eager = [t.clone() for t in m(pix, interpolate_pos_encoding=interp)]
    replay = m.capture(pix, interpolate_pos_encoding=interp)
    got = replay(pix)
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    pix2 = torch.flip(pix, dims=(3,))
    eager2 = [t.clone() for t in m(pix2, interpolate_pos_encoding=interp)]
    got2 = replay(pix2)
    torch.cuda.synchronize()
    for a, b in zip(got2, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(eager2[0], eager[0])
    with pytest.raises(ValueError):
        replay(pix[:, :, :32, :32])
    with pytest.raises(ValueError):
        m.capture(pix)                                    # 64 x 64 without interpolate_pos_encoding


# ---- 5. patch tokens into VisualBERT ----------------------------------------------------------------------------------------------
def test_patch_tokens_feed_visualbert(g, models):
    """Plumbing: the [B, N, H] view behind the class row (device, storage type, not contiguous) goes into a VisualBertModel as
    `visual_embeds` and gives what the same values give after a trip through the host."""
    name, pix, interp = golden_case(g, "square")
    cfg, _ = golden_model(g, name)
    seq, _ = models(name, "bf16")(torch.from_numpy(pix))
    tokens = V.patch_tokens(seq)
    assert tokens.shape == (2, 16, cfg["hidden_size"]) and tokens.dtype == torch.bfloat16 and not tokens.is_contiguous()
    vcfg = VB.visualbert_config(vocab_size=100, hidden_size=128, num_attention_heads=4, intermediate_size=256, num_hidden_layers=1,
                                max_position_embeddings=16, visual_embedding_dim=cfg["hidden_size"])
    vb = VB.VisualBertModel(vcfg, precision="bf16").load_state_dict(VB.make_visualbert_state_dict(vcfg, 3))
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).integers(1, 100, (2, 6)))
    direct = [t.clone() for t in vb(ids, tokens)]
    via_host = vb(ids, tokens.cpu().float().contiguous())
    assert direct[0].shape == (2, 6 + 16, 128)
    for a, b in zip(direct, via_host):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_patch_tokens_and_boxes_feed_lxmert(g, models):
    """The same view as `visual_feats` of an LxmertEncoder(visual_feat_dim=H), with `vit_patch_boxes(normalized=True)` as its
    `visual_pos`: one box per token, and the result of the same values through the host."""
    from vltk_amd.lxmert import LxmertEncoder, lxmert_config, make_lxmert_state_dict
    name, pix, _ = golden_case(g, "square")
    cfg, _ = golden_model(g, name)
    tokens = V.patch_tokens(models(name, "bf16")(torch.from_numpy(pix))[0])
    boxes = torch.from_numpy(V.vit_patch_boxes(32, 32, 8, normalized=True))
    assert boxes.shape == (tokens.shape[1], 4) and float(boxes.min()) == 0.0 and float(boxes.max()) == 1.0
    pos = boxes[None].expand(tokens.shape[0], -1, -1)
    lcfg = lxmert_config(vocab_size=100, hidden_size=128, num_attention_heads=4, intermediate_size=256, l_layers=1, x_layers=1, r_layers=1,
                         max_position_embeddings=16, visual_feat_dim=cfg["hidden_size"])
    enc = LxmertEncoder(lcfg, precision="bf16").load_state_dict(make_lxmert_state_dict(lcfg, 3))
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).integers(1, 100, (2, 6)))
    direct = [t.clone() for t in enc(ids, tokens, pos)]
    via_host = enc(ids, tokens.cpu().float().contiguous(), pos.contiguous())
    assert direct[1].shape == (2, 16, 128)
    for a, b in zip(direct, via_host):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


# ---- 6. default geometry ---------------------------------------------------------------------------------------------------------
def test_model_full_size_runs_and_is_reproducible():
    """ViT-B/16 (12 layers, hidden 768) on 224 x 224 at B = 4, bf16: 197 tokens, finite, bit-reproducible."""
    cfg = V.vit_config()
    m = V.ViTModel(cfg, precision="bf16").load_state_dict(V.make_vit_state_dict(cfg, 1))
    pix = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).standard_normal((4, 3, 224, 224)).astype(np.float32))
    a = [t.clone() for t in m(pix)]
    b = m(pix)
    for u, v in zip(a, b):
        assert torch.isfinite(u.float()).all() and torch.equal(u, v)
    assert a[0].shape == (4, 197, 768) and a[1].shape == (4, 768)
