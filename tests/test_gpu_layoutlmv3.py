"""-m gpu: vk_layoutlmv3_embed against torch in fp64 from the same tables; vltk_amd.LayoutLMv3Model and its heads against vectors
of transformers' own classes (fp32: 1e-3; bf16 / fp16: 8 x transformers' own 16-bit CPU deviation); a captured forward replayed."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                          # noqa: E402
from vltk_amd import layoutlmv3 as V3                                                   # noqa: E402

import gpu_util as G                                                                    # noqa: E402
from layoutlmv3_util import CASES, HEADS, case_kwargs, golden_state_dict               # noqa: E402
from test_gpu_layoutlm import DTS, EPS, IDS, T, rel                                     # noqa: E402

ROUND = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}            # one rounding of the storage type
SHAPES = [(128, 16, 32, "vector"), (100, 15, 20, "scalar"), (136, 18, 32, "scalar")]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "layoutlmv3_small.npz"))


@pytest.fixture(scope="module")
def models(g):
    """One model per (kind, precision), shared by the tests of this module: kind None (the bare model) or a stored head."""
    cache = {}

    def get(kind, precision):
        if (kind, precision) not in cache:
            cfg, n, sd = golden_state_dict(g, kind)
            cls = {None: V3.LayoutLMv3Model, "token": V3.LayoutLMv3ForTokenClassification, "qa": V3.LayoutLMv3ForQuestionAnswering,
                   "seq": V3.LayoutLMv3ForSequenceClassification}[HEADS.get(kind)]
            cache[(kind, precision)] = cls(*((cfg, n) if HEADS.get(kind) in ("token", "seq") else (cfg,)), precision=precision).load_state_dict(sd)
        return cache[(kind, precision)]
    return get


# ---- 1. vk_layoutlmv3_embed alone ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def embed_case(dt, H, cs, ss):
    """Inputs of one launch (B = 2, Lt = 70, V = 5: 38 workgroups, two ballot chunks a row) and its fp64 torch reference with and
    without the image.  The spatial tables lie around +3, -3, +6, -6, so a swapped segment or table is far outside tolerance; pad
    ids at t = 0, 63, 64, 69; a zero-width box, a zero-height one, and the whole page at max_2d = 1024, so h and w index 1000."""
    gen = np.random.Generator(np.random.PCG64([H, cs]))
    td = G.TDT[dt]
    B, Lt, V, vocab, P, M2, pad = 2, 70, 5, 50, 80, 1024, 1

    def tab(rows, cols=H, shift=0.0):
        return torch.from_numpy((gen.standard_normal((rows, cols)) + shift).astype(np.float32)).to(td)

    def ln():
        return torch.from_numpy(gen.uniform(0.5, 1.5, H).astype(np.float32)), torch.from_numpy(gen.standard_normal(H).astype(np.float32))
    word, typ, pos = tab(vocab), tab(2), tab(P)
    xt, yt, ht, wt = tab(M2 + 1, cs, 3.0), tab(M2, cs, -3.0), tab(M2, ss, 6.0), tab(M2, ss, -6.0)         # a guard row behind x
    cls, vpos = tab(1)[0], tab(V)
    proj = tab(B * (V - 1), H + 8)                         # the projection's rows are wider than the row, as the GEMM pads them
    ids = gen.integers(pad + 1, vocab, (B, Lt))
    ids[:, [0, 63, 64, 69]] = pad
    ids, tts = torch.from_numpy(ids), torch.from_numpy(gen.integers(0, 2, (B, Lt)))
    xs, ys = np.sort(gen.integers(0, 1001, (B, Lt, 2)), -1), np.sort(gen.integers(0, 1001, (B, Lt, 2)), -1)
    box = np.stack((xs[..., 0], ys[..., 0], xs[..., 1], ys[..., 1]), -1)
    box[0, 3], box[1, 66], box[1, 69] = (17, 5, 17, 40), (2, 900, 30, 900), (0, 0, 1000, 1000)
    box = torch.from_numpy(box)
    am = torch.ones(B, Lt)
    am[1, 64:] = 0
    vbox = torch.from_numpy(V3.visual_bbox(2, 2))
    (g1, b1), (g2, b2), (g3, b3) = ln(), ln(), ln()

    notpad = (ids != pad).long()
    p = torch.cumsum(notpad, 1) * notpad + pad             # create_position_ids_from_input_ids :138-146
    d = torch.double
    spatial = torch.cat((xt.to(d)[box[..., 0]], yt.to(d)[box[..., 1]], xt.to(d)[box[..., 2]], yt.to(d)[box[..., 3]],
                         ht.to(d)[(box[..., 3] - box[..., 1]).clip(0, 1023)], wt.to(d)[(box[..., 2] - box[..., 0]).clip(0, 1023)]), -1)
    text = F.layer_norm(word.to(d)[ids] + typ.to(d)[tts] + pos.to(d)[p] + spatial, (H,), g1.to(d), b1.to(d), 1e-5)
    vis = torch.cat((cls.to(d).expand(B, 1, H), proj.to(d)[:, :H].view(B, V - 1, H)), 1) + vpos.to(d)[None]
    vis = F.layer_norm(vis, (H,), g2.to(d), b2.to(d), 1e-6)
    joint = F.layer_norm(torch.cat((text, vis), 1), (H,), g3.to(d), b3.to(d), 1e-5)
    ref = dict(image=joint.to(td).float().view(-1, H), textonly=text.to(td).float().view(-1, H),
               rel=torch.cat((torch.stack((torch.arange(Lt).expand(B, Lt), box[..., 0], box[..., 3]), -1),
                              torch.stack((torch.arange(V), vbox[:, 0], vbox[:, 3]), -1).expand(B, V, 3)), 1).to(torch.int32),
               mask=torch.cat(((1.0 - am) * torch.finfo(torch.float32).min, torch.zeros(B, V)), 1))
    dev = dict(ids=ids, tts=tts, box=box.to(torch.int32), am=am, word=word, typ=typ, pos=pos, xt=xt, yt=yt, ht=ht, wt=wt, cls=cls, vpos=vpos,
               proj=proj, vbox=vbox, g1=g1, b1=b1, g2=g2, b2=b2, g3=g3, b3=b3)
    return dict(B=B, Lt=Lt, V=V, vocab=vocab, P=P, M2=M2, pad=pad, H=H, cs=cs, ss=ss, td=td, dt=dt), {k: v.to(G.DEV) for k, v in dev.items()}, ref


def run_embed(geo, d, image=True, masked=True):
    """One launch -> (out, rel, mask or None), each checked for a write behind its last row."""
    B, Lt, H, V = geo["B"], geo["Lt"], geo["H"], geo["V"] if image else 0
    rows = B * (Lt + V)
    y = torch.full((rows + 1, H), 77.0, dtype=geo["td"], device=G.DEV)
    r = torch.full((rows + 1, 3), -7, dtype=torch.int32, device=G.DEV)
    m = torch.full((rows + 1,), 77.0, device=G.DEV) if (image or masked) else None
    vis = [G.P(d[k]) for k in ("cls", "vpos", "vbox")] + [V, G.P(d["g2"]), G.P(d["b2"]), 1e-6, G.P(d["g3"]), G.P(d["b3"])] if image else \
        [None, None, None, 0, None, None, 1e-6, None, None]
    L.call("vk_layoutlmv3_embed", G.P(d["ids"]), G.P(d["tts"]), G.P(d["box"]), G.P(d["am"]) if masked else None, B, Lt, geo["pad"],
           G.P(d["word"]), geo["vocab"], G.P(d["typ"]), 2, G.P(d["pos"]), geo["P"], G.P(d["xt"]), G.P(d["yt"]), G.P(d["ht"]), G.P(d["wt"]),
           geo["M2"], geo["cs"], geo["ss"], G.P(d["g1"]), G.P(d["b1"]), 1e-5, G.P(d["proj"]) if image else None, d["proj"].stride(0) if image else 0,
           *vis, G.P(y), G.P(r), G.P(m) if m is not None else None, H, geo["dt"], G.stream())
    torch.cuda.synchronize()
    assert (y[rows].float() == 77.0).all() and (r[rows] == -7).all() and (m is None or float(m[rows]) == 77.0), "a write behind the last row"
    return y[:rows], r[:rows].view(B, Lt + V, 3), (None if m is None else m[:rows].view(B, Lt + V))


@pytest.mark.parametrize("H,cs,ss,form", SHAPES, ids=[f"{s[3]}{s[0]}" for s in SHAPES])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_kernel_vs_torch(dt, H, cs, ss, form):
    geo, dev, ref = embed_case(dt, H, cs, ss)
    assert V3.embed_form(H, cs, ss, geo["td"]) == form
    y, r, m = run_embed(geo, dev)
    err = rel(y, ref["image"])
    y_text, r_text, m_text = run_embed(geo, dev, image=False)
    err_text = rel(y_text, ref["textonly"])                # the text-only launch leaves out the second LayerNorm
    print(f"\n[vk_layoutlmv3_embed {IDS[DTS.index(dt)]} H={H} {form}] rel err {err:.2e}, text only {err_text:.2e}")
    assert err <= EPS[dt] and err_text <= EPS[dt]
    assert torch.equal(r.cpu(), ref["rel"]) and torch.equal(m.cpu(), ref["mask"])
    assert torch.equal(r_text.cpu(), ref["rel"][:, :geo["Lt"]]) and torch.equal(m_text.cpu(), ref["mask"][:, :geo["Lt"]])
    assert torch.equal(run_embed(geo, dev)[0], y)          # two launches, the same bits
    assert run_embed(geo, dev, image=False, masked=False)[2] is None


# ---- 2. fp32 against transformers' vectors --------------------------------------------------------------------------------------------
def assert_attention(m, cfg, Lx, entries):
    """Every layer's attention went through vk_attention_relpos, on the form and the workgroup size the joint length calls for."""
    assert [e for e in entries if e.startswith("vk_attention")] == ["vk_attention_relpos"] * cfg["num_hidden_layers"]
    assert entries.count("vk_layoutlmv3_embed") == 1
    form, queries = m.relpos_form(Lx)
    assert form == ("strict" if m.dt == L.VK_F32 else "mfma")
    # 16 queries per workgroup at L = 16, 96 at L = 65 (text only: 16 at 11, 64 at 60): the mfma form's sizes, a 16-query wave up to
    # L = 16, then 32-query waves.  The strict form (fp32) serves 16 at every length, so fp32 at L = 65 expects 16, not 96.
    assert queries == (16 if m.dt == L.VK_F32 else {11: 16, 16: 16, 60: 64, 65: 96}[Lx])


def traced(monkeypatch, fn):
    entries = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), real(name, *a))[1])
    out = fn()
    monkeypatch.undo()
    return out, entries


@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
def test_model_and_heads_fp32_vs_transformers_golden(g, models, monkeypatch, geo, case):
    kw, tag = T(case_kwargs(g, geo, case)), f"{geo}/{case}"
    m = models(None, "fp32")
    seq, entries = traced(monkeypatch, lambda: m(**kw))
    assert_attention(m, m.cfg, seq.shape[1], entries)
    errs = dict(emb=rel(m.embeddings(**kw), g[f"{tag}/embedding_output"]), seq=rel(seq, g[f"{tag}/last_hidden_state"]))
    for head in ("token5", "token12", "seq"):
        errs[head] = rel(models(head, "fp32")(**kw), g[f"{tag}/{head}_logits"])
    qam = models("qa", "fp32")
    start, end = qam(**kw)
    errs["start"], errs["end"] = rel(start, g[f"{tag}/start_logits"]), rel(end, g[f"{tag}/end_logits"])
    print(f"\n[LayoutLMv3 fp32 strict vs transformers, {tag}] rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["emb"] <= 1e-5
    assert max(errs.values()) <= 1e-3
    # the two tails on the model's own logits: the labels and the span the stored logits give
    B, Lt = kw["input_ids"].shape
    tokm = models("token12", "fp32")
    wid = torch.from_numpy(np.tile(np.arange(Lt, dtype=np.int32) // 4, (B, 1)))
    tok, _ = tokm.word_labels(tokm(**kw), wid, max(1, Lt // 4))
    assert tok.cpu().tolist() == g[f"{tag}/token12_logits"].argmax(-1).tolist()
    s, e, _ = qam.best_span(start, end, torch.ones(start.shape), max_answer_tokens=start.shape[1])
    stored = torch.from_numpy(g[f"{tag}/start_logits"])[:, :, None] + torch.from_numpy(g[f"{tag}/end_logits"])[:, None, :]
    best = stored.masked_fill(~torch.ones_like(stored[0], dtype=torch.bool).triu(), -np.inf).flatten(1).argmax(1)     # s <= e
    assert (s.cpu() * start.shape[1] + e.cpu()).tolist() == best.tolist()


# ---- 3. reduced precision against the same fp32 vectors, held to transformers' own 16-bit run -----------------------------------------
@pytest.mark.parametrize("geo,case", CASES, ids=["/".join(c) for c in CASES])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_model_16bit_within_8x_of_transformers_16bit(g, models, monkeypatch, precision, geo, case):
    kw, tag = T(case_kwargs(g, geo, case)), f"{geo}/{case}"
    m = models(None, precision)
    seq, entries = traced(monkeypatch, lambda: m(**kw))
    assert_attention(m, m.cfg, seq.shape[1], entries)
    err, theirs = rel(seq, g[f"{tag}/last_hidden_state"]), float(g[f"dev16/{tag}/{precision}"])
    print(f"\n[LayoutLMv3 {precision} vs transformers fp32, {tag}] rel err {err:.2e}; transformers' own {precision} CPU run {theirs:.2e}; "
          f"ratio {err / theirs:.2f}")
    assert err <= 8 * max(theirs, ROUND[precision])


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------------------
def test_captured_masked_forward_replays_plain_inputs(g, models):
    """long/masked captured, long/plain replayed (other ids, so other positions counted in the kernel): the eager call's bits, twice."""
    m = models(None, "bf16")
    masked, plain = T(case_kwargs(g, "long", "masked")), T(case_kwargs(g, "long", "plain"))
    plain.update(attention_mask=torch.ones_like(masked["attention_mask"]), token_type_ids=torch.zeros_like(masked["token_type_ids"]))
    eager = {k: m(**kw).clone() for k, kw in (("masked", masked), ("plain", plain))}
    replay = m.capture(**masked)
    assert torch.equal(replay(**masked), eager["masked"])
    for _ in range(2):
        assert torch.equal(replay(**plain), eager["plain"])
    assert not torch.equal(eager["plain"], eager["masked"])
    with pytest.raises(ValueError):
        replay(**{k: v for k, v in plain.items() if k != "pixel_values"})      # the capture had an image
