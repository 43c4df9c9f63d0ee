"""-m gpu: VisualBERT on the HIP path (vltk_amd.VisualBertModel / VisualBertForQuestionAnswering -> C ABI) against
(a) torch, for the one new kernel (vk_visualbert_embed) alone,
(b) vectors produced by transformers.VisualBertModel / ForQuestionAnswering themselves (fp32 strict mode, 1e-3 as test_gpu_lxmert.py),
(c) the oracle restating the bf16 / fp16 storage roundings (tests/visualbert_util.py), with the attention kernel asserted."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                          # noqa: E402
from vltk_amd import visualbert as VB                                                   # noqa: E402

import gpu_util as G                                                                    # noqa: E402
from visualbert_util import CASES, VisualBertOracle, case_kwargs, golden_inputs, golden_qa_state_dict   # noqa: E402

TDT = G.TDT
EPS = {L.VK_F32: 2e-5, L.VK_F16: 1e-3, L.VK_BF16: 8e-3}          # one rounding of the storage type (+ margin): test_gpu_lxmert.py's
IDS = ["fp32", "fp16", "bf16"]
DTS = [L.VK_F32, L.VK_F16, L.VK_BF16]


def rel(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b).float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-9))


def T(kw):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in kw.items()}


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "visualbert_small.npz"))


@pytest.fixture(scope="module")
def models(g):
    """One model per precision, shared by the tests of this module (the weights are the fixture's, geometry-independent)."""
    cfg, sd, _ = golden_inputs(g, "short")
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = VB.VisualBertModel(cfg, precision=precision).load_state_dict(sd)
        return cache[precision]
    return get


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
def embed_case(dt, Cc, aligned, split_ranges=False):
    """Inputs of one vk_visualbert_embed launch (B = 3, Lt = 9, V = 5, A = 3; proj rows 8 elements wider than Cc) and its torch
    reference.  split_ranges: text sources positive in the first half of the channels and negative in the second, visual sources
    the other way round, gamma = 1 and beta = 0 -- the sign of an output row's first half then tells which kind of row it is."""
    gen = np.random.Generator(np.random.PCG64(Cc + 7 * int(aligned)))
    td = TDT[dt]
    B, Lt, V, A, vocab, P = 3, 9, 5, 3, 50, 16
    ldp = Cc + 8

    def tab(rows, sign):
        if not split_ranges:
            return torch.from_numpy(gen.standard_normal((rows, Cc)).astype(np.float32)).to(td)
        v = gen.uniform(1.0, 2.0, (rows, Cc)).astype(np.float32)
        v[:, Cc // 2:] *= -1
        return torch.from_numpy(v * sign).to(td)
    word, pos, typ = tab(vocab, 1), tab(P, 1), tab(2, 1)
    vtyp, vpos, proj = tab(2, -1), tab(P, -1), tab(B * V, -1)
    projw = torch.zeros((B * V, ldp), dtype=td)
    projw[:, :Cc] = proj
    projw[:, Cc:] = 1000.0                               # the padding columns must never be read
    ids = torch.from_numpy(gen.integers(0, vocab, (B, Lt)))
    tts = torch.from_numpy(gen.integers(0, 2, (B, Lt)))
    vtts = torch.from_numpy(gen.integers(0, 2, (B, V)))
    align = None
    if aligned:
        a = gen.integers(0, P, (B, V, A))
        a[gen.uniform(size=a.shape) < 0.4] = -1
        a[1, 2] = -1                                      # an all-padding box
        a[2, 0] = (-1, -1, P - 1)
        align = torch.from_numpy(a.astype(np.int32))
    gm = torch.ones(Cc) if split_ranges else torch.from_numpy(gen.uniform(0.5, 1.5, Cc).astype(np.float32))
    bt = torch.zeros(Cc) if split_ranges else torch.from_numpy(gen.standard_normal(Cc).astype(np.float32))
    text = word.float()[ids] + typ.float()[tts] + pos.float()[:Lt][None]
    visn = proj.float().view(B, V, Cc) + vtyp.float()[vtts] + vpos.float()[0]
    if aligned:
        al = align.long()
        ok = al >= 0
        visn = visn + (pos.float()[al * ok] * ok[..., None]).sum(2) / ok.sum(2).clamp_min(1)[..., None]
    ref = F.layer_norm(torch.cat((text, visn), 1), (Cc,), gm, bt, 1e-12).to(td).float().view(B * (Lt + V), Cc)
    dev = dict(ids=ids, tts=tts, vtts=vtts, align=align, word=word, pos=pos, typ=typ, vtyp=vtyp, vpos=vpos, proj=projw, gm=gm, bt=bt)
    dev = {k: (None if v is None else v.to(G.DEV)) for k, v in dev.items()}
    return dict(B=B, Lt=Lt, V=V, A=A if aligned else 0, vocab=vocab, P=P, ldp=ldp, Cc=Cc, td=td, dt=dt), dev, ref


def run_embed(geo, d, y=None):
    rows = geo["B"] * (geo["Lt"] + geo["V"])
    if y is None:
        y = torch.full((rows + 1, geo["Cc"]), 77.0, dtype=geo["td"], device=G.DEV)   # one guard row behind the output
    L.call("vk_visualbert_embed", G.P(d["ids"]), G.P(d["tts"]), G.P(d["vtts"]), G.P(d["align"]), geo["A"], geo["B"], geo["Lt"], geo["V"],
           G.P(d["word"]), geo["vocab"], G.P(d["pos"]), geo["P"], G.P(d["typ"]), G.P(d["vtyp"]), 2, G.P(d["vpos"]), G.P(d["proj"]),
           geo["ldp"], G.P(d["gm"]), G.P(d["bt"]), G.P(y), geo["Cc"], 1e-12, geo["dt"], G.stream())
    torch.cuda.synchronize()
    assert (y[rows].float() == 77.0).all(), "the launch wrote behind its last row"
    return y[:rows]


@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
@pytest.mark.parametrize("Cc", [128, 100], ids=["vec128", "scalar100"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_kernel_vs_torch(dt, Cc, aligned):
    """LayerNorm(word + token_type + position | proj + visual_token_type + visual_position[0] (+ aligned mean)) in one launch:
    the 16-byte-chunk form (C = 128) and the scalar form (C = 100), 14 rows per batch entry over four workgroups."""
    geo, dev, ref = embed_case(dt, Cc, aligned)
    y = run_embed(geo, dev)
    err = rel(y, ref)
    print(f"\n[vk_visualbert_embed {IDS[DTS.index(dt)]} C={Cc} aligned={aligned}] rel err {err:.2e}")
    assert err <= EPS[dt]


@pytest.mark.parametrize("Cc", [128, 100], ids=["vec128", "scalar100"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_rows_land_in_sequence_order(dt, Cc):
    """Text rows at b * (Lt + V) + t, visual rows at b * (Lt + V) + Lt + j: the two kinds of row are built from disjoint value
    ranges whose sign pattern survives the LayerNorm."""
    geo, dev, ref = embed_case(dt, Cc, False, split_ranges=True)
    y = run_embed(geo, dev).float().cpu().view(geo["B"], geo["Lt"] + geo["V"], Cc)
    first = y[:, :, :Cc // 2]
    assert (first[:, :geo["Lt"]] > 0.3).all(), "a text position holds something else"
    assert (first[:, geo["Lt"]:] < -0.3).all(), "a visual position holds something else"
    assert rel(y.view(-1, Cc), ref) <= EPS[dt]


def test_embed_entry_refuses_bad_sizes():
    geo, dev, _ = embed_case(L.VK_F32, 128, True)
    for patch in (dict(A=17), dict(A=0), dict(Lt=17), dict(Cc=2049), dict(ldp=127), dict(B=0)):
        with pytest.raises(ValueError):
            run_embed(dict(geo, **patch), dev)
    with pytest.raises(ValueError):
        run_embed(dict(geo, A=3), dict(dev, align=None))
    y = torch.full((geo["B"] * (geo["Lt"] + geo["V"]) + 1, geo["Cc"]), 77.0, device=G.DEV)
    with pytest.raises(ValueError):
        run_embed(dict(geo, dt=L.VK_I32), dev, y)
    torch.cuda.synchronize()
    assert (y == 77.0).all(), "a refused dtype wrote the output"


# ---- 2. fp32 against transformers' vectors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_model_fp32_vs_transformers_golden(g, models, geo, case):
    cfg, sd, feats = golden_inputs(g, geo)
    m = models("fp32")
    ids, f, kw = torch.from_numpy(g[f"{geo}/input_ids"]), torch.from_numpy(feats), T(case_kwargs(g, geo, case))
    seq, pooled = m(ids, f, **kw)
    emb = m.embeddings(ids, f, **kw)
    tag = f"{geo}/{case}"
    errs = (rel(seq, g[f"{tag}/last_hidden_state"]), rel(pooled, g[f"{tag}/pooler_output"]), rel(emb, g[f"{tag}/embedding_output"]))
    print(f"\n[VisualBERT fp32 strict vs transformers, {tag}] rel err seq {errs[0]:.2e} pooled {errs[1]:.2e} embeddings {errs[2]:.2e}")
    assert errs[2] <= 1e-5
    assert max(errs[:2]) <= 1e-3


# ---- 3. reduced precision against the emulating oracle, with the attention kernel asserted ---------------------------------------
@pytest.mark.parametrize("geo,case,route", [("short", "masked", L.VK_ATT_ROUTE_MFMA), ("long", "aligned", L.VK_ATT_ROUTE_TILED)],
                         ids=["short/masked", "long/aligned"])
@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("fp16", 6e-3)])
def test_model_reduced_precision_vs_emulating_oracle(g, models, monkeypatch, precision, tol, geo, case, route):
    cfg, sd, feats = golden_inputs(g, geo)
    m = models(precision)
    ids = g[f"{geo}/input_ids"]
    B, Lt = ids.shape
    Lx, H, heads = Lt + feats.shape[1], cfg["hidden_size"], cfg["num_attention_heads"]
    entries = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), real(name, *a))[1])
    kw = case_kwargs(g, geo, case)
    seq, pooled = m(torch.from_numpy(ids), torch.from_numpy(feats), **T(kw))
    monkeypatch.undo()
    # the entry point each layer's attention went through, and the kernel that entry runs this shape on: q, k and v are column
    # slices of the fused projection's [B * Lx, 3H] output (that row stride, 16-byte aligned)
    want = "vk_attention" if route == L.VK_ATT_ROUTE_MFMA else "vk_attention_tiled"
    assert [e for e in entries if e.startswith("vk_attention")] == [want] * cfg["num_hidden_layers"]
    assert L.load().vk_attention_route(Lx, Lx, H // heads, m.dt, 3 * H, 3 * H, 3 * H, 1, int(want == "vk_attention_tiled")) == route
    assert entries.count("vk_visualbert_embed") == 1
    o_seq, o_pooled = VisualBertOracle(cfg, sd, emulate=precision).forward(ids, feats, **kw)
    errs = (rel(seq, o_seq), rel(pooled, o_pooled))
    print(f"\n[VisualBERT {precision} vs emulating oracle, {geo}/{case}] seq {errs[0]:.2e} pooled {errs[1]:.2e};"
          f" vs transformers fp32: seq {rel(seq, g[f'{geo}/{case}/last_hidden_state']):.2e}")
    assert max(errs) <= tol


# ---- 4. the QA head ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qa_models(g):
    cfg, _, _ = golden_inputs(g, "short")
    sd, n = golden_qa_state_dict(g), int(g["qa/num_labels"])
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = VB.VisualBertForQuestionAnswering(cfg, n, precision=precision).load_state_dict(sd)
        return cache[precision]
    return get


@pytest.mark.parametrize("geo", ["short", "long"])
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 4e-2)])
def test_question_answering_head(g, qa_models, precision, tol, geo):
    """fp32 against the logits transformers produced (same arg-max answers), bf16 against the emulating oracle."""
    cfg, _, feats = golden_inputs(g, geo)
    kw = case_kwargs(g, geo, "masked")
    kw["attention_mask"] = kw["attention_mask"].astype(np.int64)
    ids = g[f"{geo}/input_ids"]
    logits = qa_models(precision)(torch.from_numpy(ids), torch.from_numpy(feats), **T(kw))
    stored = g[f"qa/{geo}/logits"]
    ref = stored if precision == "fp32" else VisualBertOracle(cfg, golden_qa_state_dict(g), emulate=precision).qa_forward(ids, feats, **kw)
    assert logits.shape == stored.shape
    err = rel(logits, ref)
    print(f"\n[VisualBertForQuestionAnswering {precision}, {geo}] rel err {err:.2e}")
    assert err <= tol
    if precision == "fp32":
        assert logits.float().argmax(-1).cpu().tolist() == stored.argmax(-1).tolist()


def test_question_answering_mask_edges(g, qa_models):
    """A text mask that sums to 1 would gather row -1: IndexError, nothing launched.  attention_mask=None is an all-ones mask."""
    cfg, _, feats = golden_inputs(g, "short")
    m = qa_models("bf16")
    ids, f = torch.from_numpy(g["short/input_ids"]), torch.from_numpy(feats)
    bad = torch.ones(ids.shape, dtype=torch.int64)
    bad[1, 1:] = 0
    with pytest.raises(IndexError):
        m(ids, f, attention_mask=bad)
    a = m(ids, f).clone()
    b = m(ids, f, attention_mask=torch.ones(ids.shape))
    assert torch.equal(a, b)


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(g, models):
    """One forward captured into a HIP graph replays bit-identically and follows new inputs of the same shape; inputs the
    host checks refuse are refused at replay too."""
    cfg, sd, feats = golden_inputs(g, "long")
    m = models("bf16")
    ids, f = torch.from_numpy(g["long/input_ids"]), torch.from_numpy(feats)
    kw = T(case_kwargs(g, "long", "aligned"))
    eager = [t.clone() for t in m(ids, f, **kw)]
    replay = m.capture(ids, f, **kw)
    got = replay(ids, f, **kw)
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    ids2 = torch.roll(ids, 1, dims=1)
    kw2 = dict(kw, image_text_alignment=torch.roll(kw["image_text_alignment"], 1, dims=1))
    eager2 = [t.clone() for t in m(ids2, f, **kw2)]
    got2 = replay(ids2, f, **kw2)
    torch.cuda.synchronize()
    for a, b in zip(got2, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(eager2[0], eager[0])
    with pytest.raises(IndexError):
        replay(ids2, f, **dict(kw2, image_text_alignment=torch.full_like(kw["image_text_alignment"], cfg["max_position_embeddings"])))
    with pytest.raises(ValueError):
        replay(ids2, f)                                   # the capture had masks


# ---- 6. default geometry ---------------------------------------------------------------------------------------------------------
def test_model_full_size_runs_and_is_reproducible():
    """transformers' default VisualBERT geometry (12 layers, hidden 768) with this extractor's 2048-wide features at B = 8,
    20 + 36 tokens, bf16: finite, bit-reproducible."""
    cfg = VB.visualbert_config(visual_embedding_dim=2048)
    m = VB.VisualBertModel(cfg, precision="bf16").load_state_dict(VB.make_visualbert_state_dict(cfg, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (8, 20)))
    feats = torch.from_numpy(np.maximum(gen.standard_normal((8, 36, 2048)), 0).astype(np.float32))
    a = [t.clone() for t in m(ids, feats)]
    b = m(ids, feats)
    for u, v in zip(a, b):
        assert torch.isfinite(u.float()).all() and torch.equal(u, v)
    assert a[0].shape == (8, 56, 768) and a[1].shape == (8, 768)
