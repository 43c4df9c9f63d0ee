"""-m gpu: LayoutLM on the HIP path (vltk_amd.LayoutLMModel and its three heads -> C ABI) against
(a) torch, for vk_layoutlm_embed alone; the numpy restatements (tests/layoutlm_util.py), bit for bit, for the two tail kernels,
(b) vectors produced by transformers.LayoutLMModel / ForTokenClassification / ForQuestionAnswering / ForSequenceClassification
    themselves (fp32 strict mode, 1e-3 as test_gpu_visualbert.py),
(c) the oracle restating the bf16 / fp16 storage roundings, with the attention kernel asserted."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                          # noqa: E402
from vltk_amd import layoutlm as LM                                                     # noqa: E402

import gpu_util as G                                                                    # noqa: E402
from layoutlm_util import (CASES, LayoutLMOracle, case_kwargs, golden_head, golden_model, span_select_ref,   # noqa: E402
                           token_word_labels_ref)

TDT = G.TDT
EPS = {L.VK_F32: 2e-5, L.VK_F16: 1e-3, L.VK_BF16: 8e-3}          # one rounding of the storage type (+ margin): test_gpu_visualbert.py's
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
    return np.load(os.path.join(golden_dir, "layoutlm_small.npz"))


@pytest.fixture(scope="module")
def models(g):
    """One model per (kind, precision), shared by the tests of this module: kind "model" | "token" | "qa" | "seq"."""
    cache = {}

    def get(kind, precision):
        if (kind, precision) not in cache:
            if kind == "model":
                cfg, sd = golden_model(g)
                m = LM.LayoutLMModel(cfg, precision=precision)
            else:
                cfg, n, sd = golden_head(g, kind)
                m = {"token": lambda: LM.LayoutLMForTokenClassification(cfg, n, precision=precision),
                     "qa": lambda: LM.LayoutLMForQuestionAnswering(cfg, precision=precision),
                     "seq": lambda: LM.LayoutLMForSequenceClassification(cfg, n, precision=precision)}[kind]()
            cache[(kind, precision)] = m.load_state_dict(sd)
        return cache[(kind, precision)]
    return get


# ---- 1. vk_layoutlm_embed alone ----------------------------------------------------------------------------------------------------
def embed_case(dt, Cc):
    """Inputs of one vk_layoutlm_embed launch (B = 3, L = 9: seven workgroups of four rows) and its torch reference.  The x table
    lies around +3 and the y table around -3, the h table around +6 and the w table around -6, so a lookup in the wrong table, or
    x0 / x1 / y0 / y1 taken for each other, moves the result by far more than the tolerance."""
    gen = np.random.Generator(np.random.PCG64(Cc))
    td = TDT[dt]
    B, Lt, vocab, P, M2 = 3, 9, 50, 16, 64

    def tab(rows, shift=0.0):
        return torch.from_numpy((gen.standard_normal((rows, Cc)) + shift).astype(np.float32)).to(td)
    word, pos, typ = tab(vocab), tab(P), tab(2)
    xt, yt, ht, wt = tab(M2, 3.0), tab(M2, -3.0), tab(M2, 6.0), tab(M2, -6.0)
    ids = torch.from_numpy(gen.integers(0, vocab, (B, Lt)))
    tts = torch.from_numpy(gen.integers(0, 2, (B, Lt)))
    xs, ys = np.sort(gen.integers(0, M2, (B, Lt, 2)), -1), np.sort(gen.integers(0, M2, (B, Lt, 2)), -1)
    box = np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)
    box[0, 0] = (0, 0, M2 - 1, M2 - 1)
    box[1, 3] = (17, 5, 17, 40)                           # zero width
    box[2, 8] = (2, M2 - 1, 30, M2 - 1)                   # zero height, in the last row of the launch
    box[2, 0] = (0, 0, 0, 0)
    box = torch.from_numpy(box)
    gm = torch.from_numpy(gen.uniform(0.5, 1.5, Cc).astype(np.float32))
    bt = torch.from_numpy(gen.standard_normal(Cc).astype(np.float32))
    e = word.float()[ids] + pos.float()[:Lt][None]
    for t_, i in ((xt, box[..., 0]), (yt, box[..., 1]), (xt, box[..., 2]), (yt, box[..., 3]), (ht, box[..., 3] - box[..., 1]),
                  (wt, box[..., 2] - box[..., 0]), (typ, tts)):
        e = e + t_.float()[i]
    ref = F.layer_norm(e, (Cc,), gm, bt, 1e-12).to(td).float().view(B * Lt, Cc)
    dev = dict(ids=ids, tts=tts, box=box.to(torch.int32), word=word, pos=pos, typ=typ, xt=xt, yt=yt, ht=ht, wt=wt, gm=gm, bt=bt)
    dev = {k: v.to(G.DEV) for k, v in dev.items()}
    return dict(B=B, Lt=Lt, vocab=vocab, P=P, M2=M2, Cc=Cc, td=td, dt=dt), dev, ref


def run_embed(geo, d, y=None):
    rows = geo["B"] * geo["Lt"]
    if y is None:
        y = torch.full((rows + 1, geo["Cc"]), 77.0, dtype=geo["td"], device=G.DEV)   # one guard row behind the output
    L.call("vk_layoutlm_embed", G.P(d["ids"]), G.P(d["tts"]), G.P(d["box"]), geo["B"], geo["Lt"], G.P(d["word"]), geo["vocab"],
           G.P(d["pos"]), geo["P"], G.P(d["xt"]), G.P(d["yt"]), G.P(d["ht"]), G.P(d["wt"]), geo["M2"], G.P(d["typ"]), 2, G.P(d["gm"]),
           G.P(d["bt"]), G.P(y), geo["Cc"], 1e-12, geo["dt"], G.stream())
    torch.cuda.synchronize()
    assert (y[rows].float() == 77.0).all(), "the launch wrote behind its last row"
    return y[:rows]


@pytest.mark.parametrize("Cc", [128, 100], ids=["vec128", "scalar100"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_kernel_vs_torch(dt, Cc):
    """LayerNorm of the nine-row sum in one launch: the 16-byte-chunk form (C = 128) and the scalar form (C = 100)."""
    geo, dev, ref = embed_case(dt, Cc)
    y = run_embed(geo, dev)
    err = rel(y, ref)
    print(f"\n[vk_layoutlm_embed {IDS[DTS.index(dt)]} C={Cc}] rel err {err:.2e}")
    assert err <= EPS[dt]


def test_embed_reference_tells_the_tables_apart():
    """The reference of the test above is sensitive to what it is meant to catch: x0 <-> y0 or x1 <-> x0 swapped in the boxes
    moves it by far more than any tolerance used here."""
    geo, dev, ref = embed_case(L.VK_F32, 128)
    for perm in ((1, 0, 2, 3), (2, 1, 0, 3)):
        swapped = dict(dev, box=dev["box"][..., list(perm)].contiguous())
        assert rel(run_embed(geo, swapped), ref) > 0.1


def test_embed_entry_refuses_a_bad_dtype():
    geo, dev, _ = embed_case(L.VK_F32, 128)
    y = torch.full((geo["B"] * geo["Lt"] + 1, geo["Cc"]), 77.0, device=G.DEV)
    with pytest.raises(ValueError):
        run_embed(dict(geo, dt=L.VK_I32), dev, y)
    torch.cuda.synchronize()
    assert (y == 77.0).all(), "a refused dtype wrote the output"


# ---- 2. vk_token_word_labels, bit-equal to the restatement ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def labels_case(Cn, Lt):
    """Small-integer logits (exact in every storage type; arg-max ties and vote ties are real), word ids with -1 holes, words whose
    tokens are scattered, ids >= W, a word without tokens; rows with a NaN, with nothing but NaN and with nothing but -inf.
    -> (logits [B, L, C] f32, word_ids, W, reference token labels, reference word labels)."""
    gen = np.random.Generator(np.random.PCG64([Cn, Lt]))
    B, W = 3, max(1, Lt // 3)
    logits = gen.integers(-3, 4, (B, Lt, Cn)).astype(np.float32)
    logits[0, 0, 0] = np.nan
    logits[1, Lt - 1, :] = np.nan
    logits[2, Lt // 2, :] = -np.inf
    wid = gen.integers(-1, W + 2, (B, Lt)).astype(np.int32)                          # W and W + 1 are no words
    if W > 1:
        wid[wid == W - 1] = -1                                                       # the last word has no token
    tok, words = token_word_labels_ref(logits, wid, W)
    return logits, wid, W, tok, words


@pytest.mark.parametrize("Lt", [1, 64, 65, 512])
@pytest.mark.parametrize("Cn", [1, 2, 7, 64])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_token_word_labels_bit_equal(dt, Cn, Lt):
    logits, wid, W, tok_ref, words_ref = labels_case(Cn, Lt)
    B, ld = logits.shape[0], Cn + 3
    buf = torch.full((B, Lt, ld), 100.0, dtype=TDT[dt])                              # the padding columns would win if read
    buf[..., :Cn] = torch.from_numpy(logits).to(TDT[dt])
    buf, wid_d = buf.to(G.DEV), torch.from_numpy(wid).to(G.DEV)
    tok = torch.full((B * Lt + 1,), -7, dtype=torch.int32, device=G.DEV)            # one guard element behind each output
    words = torch.full((B * W + 1,), -7, dtype=torch.int32, device=G.DEV)
    L.call("vk_token_word_labels", G.P(buf), ld, G.P(wid_d), B, Lt, Cn, W, G.P(tok), G.P(words), dt, G.stream())
    torch.cuda.synchronize()
    assert int(tok[-1]) == -7 and int(words[-1]) == -7
    assert np.array_equal(tok[:-1].cpu().numpy().reshape(B, Lt), tok_ref)
    assert np.array_equal(words[:-1].cpu().numpy().reshape(B, W), words_ref)
    if W > 1:
        assert (words_ref[:, W - 1] == -1).all()
    for b in range(B):                                                               # the vote is torch.mode on the CPU
        for w in range(W):
            mine = torch.from_numpy(tok_ref[b][wid[b] == w])
            if len(mine):
                assert int(torch.mode(mine).values) == words_ref[b, w]


# ---- 3. vk_span_select, bit-equal to the restatement ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def span_case(Lt, mx):
    """Five examples: a context that does not start at 0 (from L // 3 on, where L allows), a one-token context, an empty one,
    all-equal logits, and scattered context tokens among NaN and infinite logits.  Logits are quarters (exact in every storage
    type, so ties are real).  -> (start, end [B, L] f32, context, reference start, end, score)."""
    gen = np.random.Generator(np.random.PCG64([Lt, mx]))
    B = 5
    st = (gen.integers(-20, 21, (B, Lt)) / 4).astype(np.float32)
    en = (gen.integers(-20, 21, (B, Lt)) / 4).astype(np.float32)
    ctx = np.zeros((B, Lt), np.int32)
    ctx[0, Lt // 3:] = 1
    ctx[1, Lt // 2] = 1
    first = min(2, Lt - 1)
    st[3], en[3], ctx[3, first:] = 1.25, -0.5, 1
    ctx[4] = gen.integers(0, 2, Lt)
    st[4, ::5], en[4, 1::7], en[4, 2::11] = np.nan, np.inf, -np.inf
    ref = span_select_ref(st, en, ctx, mx)
    assert (ref[0][2], ref[1][2], ref[2][2]) == (-1, -1, -np.inf)                    # the empty context
    assert (ref[0][1], ref[1][1]) == (Lt // 2, Lt // 2) and (ref[0][3], ref[1][3]) == (first, first)
    return st, en, ctx, ref


@pytest.mark.parametrize("mx", ["1", "30", "L"])
@pytest.mark.parametrize("Lt", [1, 63, 64, 65, 512])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_span_select_bit_equal(dt, Lt, mx):
    mx = Lt if mx == "L" else int(mx)
    st, en, ctx, (s_ref, e_ref, sc_ref) = span_case(Lt, mx)
    B = st.shape[0]
    buf = torch.full((B, Lt, 8), 50.0, dtype=TDT[dt])                                # the logits are columns 2 and 5 of a wider buffer
    buf[..., 2], buf[..., 5] = torch.from_numpy(st).to(TDT[dt]), torch.from_numpy(en).to(TDT[dt])
    buf, ctx_d = buf.to(G.DEV), torch.from_numpy(ctx).to(G.DEV)
    s = torch.full((B + 1,), -7, dtype=torch.int32, device=G.DEV)
    e = torch.full((B + 1,), -7, dtype=torch.int32, device=G.DEV)
    sc = torch.full((B + 1,), -7.0, dtype=torch.float32, device=G.DEV)
    es = buf.element_size()
    L.call("vk_span_select", buf.data_ptr() + 2 * es, 8, buf.data_ptr() + 5 * es, 8, G.P(ctx_d), B, Lt, mx, G.P(s), G.P(e), G.P(sc),
           dt, G.stream())
    torch.cuda.synchronize()
    assert int(s[-1]) == -7 and int(e[-1]) == -7 and float(sc[-1]) == -7.0
    assert s[:-1].cpu().tolist() == s_ref.tolist() and e[:-1].cpu().tolist() == e_ref.tolist()
    assert np.array_equal(sc[:-1].cpu().numpy().view(np.uint32), sc_ref.view(np.uint32))


# ---- 4. fp32 against transformers' vectors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_model_fp32_vs_transformers_golden(g, models, geo, case):
    ids, kw, tag = torch.from_numpy(g[f"{geo}/input_ids"]), T(case_kwargs(g, geo, case)), f"{geo}/{case}"
    m = models("model", "fp32")
    seq, pooled = m(ids, **kw)
    emb = m.embeddings(ids, **kw)
    errs = (rel(seq, g[f"{tag}/last_hidden_state"]), rel(pooled, g[f"{tag}/pooler_output"]), rel(emb, g[f"{tag}/embedding_output"]))
    print(f"\n[LayoutLM fp32 strict vs transformers, {tag}] rel err seq {errs[0]:.2e} pooled {errs[1]:.2e} embeddings {errs[2]:.2e}")
    assert errs[2] <= 1e-5
    assert max(errs[:2]) <= 1e-3


@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_heads_fp32_vs_transformers_golden(g, models, geo, case):
    """The three heads to 1e-3, with the arg-max labels and the best span the stored logits give."""
    ids, kw, tag = torch.from_numpy(g[f"{geo}/input_ids"]), T(case_kwargs(g, geo, case)), f"{geo}/{case}"
    B, Lt = ids.shape
    tokm = models("token", "fp32")
    logits = tokm(ids, **kw)
    stored = g[f"{tag}/token_logits"]
    wid = torch.from_numpy(np.tile(np.arange(Lt, dtype=np.int32) // 4, (B, 1)))
    tok, words = tokm.word_labels(logits, wid, Lt // 4)
    tok_ref, words_ref = token_word_labels_ref(stored, wid.numpy(), Lt // 4)
    qam = models("qa", "fp32")
    start, end = qam(ids, **kw)
    ctx = torch.from_numpy(g[f"{geo}/attention_mask"] if case == "masked" else np.ones((B, Lt), np.float32))
    s, e, sc = qam.best_span(start, end, ctx, max_answer_tokens=30)
    s_ref, e_ref, sc_ref = span_select_ref(g[f"{tag}/start_logits"], g[f"{tag}/end_logits"], ctx.numpy(), 30)
    seq_logits = models("seq", "fp32")(ids, **kw)
    errs = (rel(logits, stored), rel(start, g[f"{tag}/start_logits"]), rel(end, g[f"{tag}/end_logits"]), rel(seq_logits, g[f"{tag}/seq_logits"]))
    print(f"\n[LayoutLM heads fp32 vs transformers, {tag}] rel err token {errs[0]:.2e} start {errs[1]:.2e} end {errs[2]:.2e} seq {errs[3]:.2e}")
    assert max(errs) <= 1e-3
    assert logits.shape == stored.shape and start.shape == (B, Lt) and seq_logits.shape == g[f"{tag}/seq_logits"].shape
    assert tok.cpu().tolist() == stored.argmax(-1).tolist() == tok_ref.tolist()
    assert words.cpu().tolist() == words_ref.tolist()
    assert s.cpu().tolist() == s_ref.tolist() and e.cpu().tolist() == e_ref.tolist()
    assert np.abs(sc.cpu().numpy() - sc_ref).max() <= 1e-3 * np.abs(sc_ref).max()
    assert seq_logits.float().argmax(-1).cpu().tolist() == g[f"{tag}/seq_logits"].argmax(-1).tolist()


# ---- 5. reduced precision against the emulating oracle, with the attention kernel asserted ---------------------------------------
@pytest.mark.parametrize("geo,route", [("short", L.VK_ATT_ROUTE_MFMA), ("long", L.VK_ATT_ROUTE_TILED)], ids=["short/masked", "long/masked"])
@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("fp16", 6e-3)])
def test_model_reduced_precision_vs_emulating_oracle(g, models, monkeypatch, precision, tol, geo, route):
    cfg, sd = golden_model(g)
    m = models("model", precision)
    ids, kw = g[f"{geo}/input_ids"], case_kwargs(g, geo, "masked")
    B, Lt = ids.shape
    H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    entries = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), real(name, *a))[1])
    seq, pooled = m(torch.from_numpy(ids), **T(kw))
    monkeypatch.undo()
    # the entry point each layer's attention went through, and the kernel that entry runs this shape on: q, k and v are column
    # slices of the fused projection's [B * L, 3H] output (that row stride, 16-byte aligned)
    want = "vk_attention" if route == L.VK_ATT_ROUTE_MFMA else "vk_attention_tiled"
    assert [e for e in entries if e.startswith("vk_attention")] == [want] * cfg["num_hidden_layers"]
    assert L.load().vk_attention_route(Lt, Lt, H // heads, m.dt, 3 * H, 3 * H, 3 * H, 1, int(want == "vk_attention_tiled")) == route
    assert entries.count("vk_layoutlm_embed") == 1
    o_seq, o_pooled = LayoutLMOracle(cfg, sd, emulate=precision).forward(ids, **kw)
    errs = (rel(seq, o_seq), rel(pooled, o_pooled))
    print(f"\n[LayoutLM {precision} vs emulating oracle, {geo}/masked] seq {errs[0]:.2e} pooled {errs[1]:.2e};"
          f" vs transformers fp32: seq {rel(seq, g[f'{geo}/masked/last_hidden_state']):.2e}")
    assert max(errs) <= tol


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(g, models):
    """One forward captured into a HIP graph replays bit-identically and follows new ids and boxes of the same shape; inputs the
    host checks refuse are refused at replay too, and so is an input that was None at capture (or the other way round)."""
    cfg, _ = golden_model(g)
    m = models("model", "bf16")
    ids = torch.from_numpy(g["long/input_ids"])
    kw = T(case_kwargs(g, "long", "masked"))
    eager = [t.clone() for t in m(ids, **kw)]
    replay = m.capture(ids, **kw)
    got = replay(ids, **kw)
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    ids2 = torch.roll(ids, 1, dims=1)
    kw2 = dict(kw, bbox=torch.roll(kw["bbox"], 3, dims=1))
    eager2 = [t.clone() for t in m(ids2, **kw2)]
    got2 = replay(ids2, **kw2)
    torch.cuda.synchronize()
    for a, b in zip(got2, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(eager2[0], eager[0])
    with pytest.raises(IndexError):
        replay(ids2, **dict(kw2, bbox=torch.full_like(kw["bbox"], cfg["max_2d_position_embeddings"])))
    with pytest.raises(ValueError):
        replay(ids2, **{k: v for k, v in kw2.items() if k != "bbox"})          # the capture had boxes
    with pytest.raises(ValueError):
        replay(ids2, bbox=kw2["bbox"])                                         # ... and masks


# ---- 7. pages to word labels -----------------------------------------------------------------------------------------------------
def test_pages_to_word_labels_end_to_end(g, models):
    """`ocr_token_boxes` -> LayoutLMForTokenClassification -> `word_labels` on two pages equals the oracle's word labels (fp32)."""
    cfg, n, sd = golden_head(g, "token")
    gen = np.random.Generator(np.random.PCG64(11))
    Lt, pages = 48, []
    for raw, nwords in (((850, 1100), 14), ((612, 792), 9)):
        xy = gen.uniform(0, 0.9, (nwords, 2)) * raw
        wh = gen.uniform(0.01, 0.2, (nwords, 2)) * raw                          # some boxes end past the page
        pages.append(LM.ocr_token_boxes(np.concatenate((xy, wh), 1), gen.integers(0, 5, nwords), raw, Lt, add_cls=True))
    bbox = np.stack([p[0] for p in pages])
    wid = np.stack([p[1] for p in pages])
    W = 14
    assert wid.max() < W and (wid == -1).any() and bbox.max() <= 1000
    ids = gen.integers(1, cfg["vocab_size"], (2, Lt))
    mask = (wid >= 0).astype(np.float32)
    mask[:, 0] = 1                                                             # the page token
    m = models("token", "fp32")
    logits = m(torch.from_numpy(ids), bbox=torch.from_numpy(bbox), attention_mask=torch.from_numpy(mask))
    tok, words = m.word_labels(logits, torch.from_numpy(wid), W)
    o_logits = LayoutLMOracle(cfg, sd).token_forward(ids, bbox=bbox, attention_mask=mask)
    tok_ref, words_ref = token_word_labels_ref(o_logits.numpy(), wid, W)
    assert rel(logits, o_logits) <= 1e-3
    assert tok.cpu().tolist() == tok_ref.tolist() and words.cpu().tolist() == words_ref.tolist()
    assert (words_ref[1, 9:] == -1).all() and (words_ref >= 0).any()            # the second page has nine words


# ---- 8. default geometry -----------------------------------------------------------------------------------------------------------
def test_model_full_size_runs_and_is_reproducible(monkeypatch):
    """transformers' default LayoutLM geometry (12 layers, hidden 768) on two 512-token pages, bf16: finite, bit-reproducible, and
    every layer's attention on the tiled kernel."""
    cfg = LM.layoutlm_config()
    m = LM.LayoutLMModel(cfg, precision="bf16").load_state_dict(LM.make_layoutlm_state_dict(cfg, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (2, 512)))
    xs, ys = np.sort(gen.integers(0, 1001, (2, 512, 2)), -1), np.sort(gen.integers(0, 1001, (2, 512, 2)), -1)
    bbox = torch.from_numpy(np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1))
    entries = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), real(name, *a))[1])
    a = [t.clone() for t in m(ids, bbox)]
    monkeypatch.undo()
    b = m(ids, bbox)
    for u, v in zip(a, b):
        assert torch.isfinite(u.float()).all() and torch.equal(u, v)
    assert a[0].shape == (2, 512, 768) and a[1].shape == (2, 768)
    assert [e for e in entries if e.startswith("vk_attention")] == ["vk_attention_tiled"] * 12
    assert L.load().vk_attention_route(512, 512, 64, m.dt, 2304, 2304, 2304, 1, 1) == L.VK_ATT_ROUTE_TILED
