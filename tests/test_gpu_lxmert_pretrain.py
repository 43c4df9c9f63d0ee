"""-m gpu: LXMERT's pre-training heads and losses on the HIP path (vltk_amd.LxmertForPreTraining -> C ABI) against
(a) float64 references computed from the STORED operands, under the per-row bounds tests/lxmert_pretrain_util.py derives from the
    kernels' rounding points, for vk_cross_entropy (both forms, asserted), vk_smooth_l1_rows and vk_loss_reduce alone,
(b) vectors produced by transformers.LxmertForPreTraining itself (fp32 strict mode, 1e-3 as test_gpu_visualbert.py),
(c) the oracle restating the bf16 / fp16 storage roundings, with the attention kernel asserted."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                                                          # noqa: E402
from vltk_amd import lxmert_pretrain as LP                                              # noqa: E402

import gpu_util as G                                                                    # noqa: E402
import lxmert_pretrain_util as U                                                        # noqa: E402

TDT = G.TDT
IDS = ["fp32", "fp16", "bf16"]
DTS = [L.VK_F32, L.VK_F16, L.VK_BF16]
FORMS = {"vec": L.VK_CE_FORM_VEC, "scalar": L.VK_CE_FORM_SCALAR}
TERM_KEYS = ("mlm", "matched", "obj", "attr", "feat", "ans")
EPS = {"fp16": 1e-3, "bf16": 8e-3}      # one rounding of the storage type (+ margin): test_gpu_visualbert.py's and test_gpu_layoutlm.py's


def rel(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b).float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-9))


def worst(out, ref, bound):
    """max over the rows of |out - ref| / bound; a row off a zero bound, or not finite, counts as inf."""
    out, err = np.asarray(out, np.float64), np.abs(np.asarray(out, np.float64) - ref)
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(np.where(np.isfinite(out), ratio, np.inf).max())


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lxmert_pretrain_small.npz"))


@pytest.fixture(scope="module")
def models(g):
    """One model per (stored config, precision), shared by the tests of this module."""
    cache = {}

    def get(name, precision):
        if (name, precision) not in cache:
            cfg, sd = U.golden_model(g, name)
            cache[(name, precision)] = LP.LxmertForPreTraining(cfg, precision=precision).load_state_dict(sd)
        return cache[(name, precision)]
    return get


class Recorder:
    """L.call with every call's name and arguments kept."""

    def __init__(self, monkeypatch):
        self.calls, real = [], L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (self.calls.append((name, a)), real(name, *a))[1])

    def names(self, prefix="vk_"):
        return [n for n, _ in self.calls if n.startswith(prefix)]


# ---- 1. vk_cross_entropy alone ---------------------------------------------------------------------------------------------------
CE_CASES = {"vec128": (128, 128, "vec"), "scalar100": (100, 104, "scalar"), "oddstride128": (128, 131, "scalar"), "two": (2, 8, "scalar"),
            "vocab30522": (30522, 30528, "vec")}


@functools.lru_cache(maxsize=None)
def ce_case(name, dt):
    """Seven rows (five at the vocabulary's width, where a thread makes many passes): random, logits near +-90 (a single
    fp32 exp overflows without the max subtraction), all equal, peaked; labels 0, C - 1 and -100.  -> (stored logits [M, ld], labels, reference)."""
    C, ld, _ = CE_CASES[name]
    M = 5 if C > 1000 else 7
    gen = np.random.Generator(np.random.PCG64([C, ld]))
    x = gen.standard_normal((M, ld)) * 2
    x[1] = np.where(gen.uniform(size=ld) < 0.5, 90.0, -90.0) + gen.standard_normal(ld)
    x[1, 0] = 90.5
    x[2] = 1.25
    x[3, C // 2] += 12
    x[:, C:] = 200.0                                        # the padding columns would swamp the sum if read
    labels = np.asarray([0, C - 1, C // 2, -100, C - 1, 0, -100][:M])
    x = torch.from_numpy(x).to(TDT[dt])
    return x, labels, U.ce_reference(x[:, :C], labels)


@pytest.mark.parametrize("name", list(CE_CASES))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_cross_entropy_rows_within_bound(dt, name):
    C, ld, form = CE_CASES[name]
    x, labels, r = ce_case(name, dt)
    M = len(labels)
    xd, ld_ = x.to(G.DEV), torch.from_numpy(labels).to(G.DEV)
    assert L.load().vk_cross_entropy_form(C, ld, dt, int(xd.data_ptr() % 16 == 0)) == FORMS[form] == FORMS[U.ce_form(C, ld, TDT[dt])]
    rows = torch.full((M + 1,), 77.0, dtype=torch.float32, device=G.DEV)               # one guard element behind the output
    L.call("vk_cross_entropy", G.P(xd), ld, M, C, G.P(ld_), -100, G.P(rows), dt, G.stream())
    torch.cuda.synchronize()
    assert float(rows[M]) == 77.0, "the launch wrote behind its last row"
    got = rows[:M].cpu().numpy()
    w = worst(got, r["ref"], U.ce_bound(r, form, TDT[dt]))
    print(f"\n[vk_cross_entropy {IDS[DTS.index(dt)]} {name} ({form})] worst |out - ref| / bound {w:.3f}", end="")
    assert w <= 1.0, (got, r["ref"])
    assert (got[labels == -100] == 0).all()


def test_cross_entropy_both_forms_ran_and_agree():
    """The same rows through both kernels (an aligned and a one-byte-element-shifted copy of the buffer): each within its bound."""
    C, ld = 256, 256
    gen = np.random.Generator(np.random.PCG64(4))
    x = torch.from_numpy(gen.standard_normal((6, ld)) * 3).to(torch.bfloat16)
    labels = np.asarray([0, 255, -100, 17, 128, 3])
    r = U.ce_reference(x, labels)
    buf = torch.zeros((6 * ld + 8,), dtype=torch.bfloat16, device=G.DEV)
    lab = torch.from_numpy(labels).to(G.DEV)
    seen = set()
    for shift in (0, 1):                                    # shift 1: rows start 2 bytes off a 16-byte boundary
        view = buf[shift:shift + 6 * ld].view(6, ld)
        view.copy_(x)
        form = L.load().vk_cross_entropy_form(C, ld, L.VK_BF16, int(view.data_ptr() % 16 == 0))
        seen.add(form)
        rows = torch.empty((6,), dtype=torch.float32, device=G.DEV)
        L.call("vk_cross_entropy", G.P(view), ld, 6, C, G.P(lab), -100, G.P(rows), L.VK_BF16, G.stream())
        torch.cuda.synchronize()
        name = "vec" if form == L.VK_CE_FORM_VEC else "scalar"
        assert worst(rows.cpu().numpy(), r["ref"], U.ce_bound(r, name, torch.bfloat16)) <= 1.0
    assert seen == {L.VK_CE_FORM_VEC, L.VK_CE_FORM_SCALAR}


def test_cross_entropy_refuses_bad_arguments():
    x = torch.zeros((2, 8), device=G.DEV)
    lab = torch.zeros((2,), dtype=torch.int64, device=G.DEV)
    rows = torch.zeros((2,), device=G.DEV)
    with pytest.raises(ValueError):
        L.call("vk_cross_entropy", G.P(x), 4, 2, 8, G.P(lab), -100, G.P(rows), L.VK_F32, G.stream())      # ld < C
    with pytest.raises(ValueError):
        L.call("vk_cross_entropy", G.P(x), 8, 2, 8, G.P(lab), 3, G.P(rows), L.VK_F32, G.stream())         # ignore_index names a class
    assert L.load().vk_cross_entropy_form(8, 4, L.VK_F32, 1) == -L.VK_EINVAL


# ---- 2. vk_smooth_l1_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 2048])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_smooth_l1_rows_within_bound(dt, C):
    """Differences on both sides of +-1, entries at exactly +-1 and 0, a row that is all zeros (the loss is 0 exactly)."""
    gen = np.random.Generator(np.random.PCG64(C))
    M, ld, ldt = 6, C + 8, C + 3
    pred = torch.zeros((M, ld), dtype=TDT[dt])
    pred[:, :C] = torch.from_numpy(gen.standard_normal((M, C))).to(TDT[dt])
    pred[0, :3] = torch.tensor([0.5, -0.25, 2.0])            # exact in every type, and so are these minus +-1
    pred[:, C:] = 500.0
    diff = gen.uniform(-3, 3, (M, C)).astype(np.float32)
    diff[0, :3], diff[5] = (1, -1, 0), 0
    target = np.full((M, ldt), -500.0, np.float32)
    target[:, :C] = pred[:, :C].float().numpy() - diff
    r = U.smooth_l1_reference(pred[:, :C], target[:, :C])
    d = pred[0, :3].double().numpy() - target[0, :3].astype(np.float64)
    assert d.tolist() == [1.0, -1.0, 0.0]
    rows = torch.full((M + 1,), 77.0, dtype=torch.float32, device=G.DEV)
    pd, td = pred.to(G.DEV), torch.from_numpy(target).to(G.DEV)
    L.call("vk_smooth_l1_rows", G.P(pd), ld, G.P(td), ldt, M, C, G.P(rows), dt, G.stream())
    torch.cuda.synchronize()
    assert float(rows[M]) == 77.0
    got = rows[:M].cpu().numpy()
    w = worst(got, r["ref"], U.smooth_l1_bound(r))
    print(f"\n[vk_smooth_l1_rows {IDS[DTS.index(dt)]} C={C}] worst |out - ref| / bound {w:.3f}", end="")
    assert w <= 1.0 and got[5] == 0


def test_smooth_l1_rows_refuses_a_bad_dtype():
    pred, target = torch.zeros((2, 8), device=G.DEV), torch.zeros((2, 8), device=G.DEV)
    rows = torch.full((2,), 77.0, device=G.DEV)
    assert L.load().vk_smooth_l1_rows(G.P(pred), 8, G.P(target), 8, 2, 8, G.P(rows), L.VK_I32, G.stream()) == L.VK_EINVAL
    torch.cuda.synchronize()
    assert (rows == 77.0).all(), "a refused dtype wrote the output"


# ---- 3. vk_loss_reduce and vk_loss_total -------------------------------------------------------------------------------------------
def reduce_call(rows, weight=None, labels=None, scale=1.0):
    out = torch.full((2,), 77.0, dtype=torch.float32, device=G.DEV)
    L.call("vk_loss_reduce", G.P(rows), G.P(weight), G.P(labels), -100, rows.numel(), scale, G.P(out), G.stream())
    torch.cuda.synchronize()
    assert float(out[1]) == 77.0
    return out[0].cpu().numpy()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 4097])
def test_loss_reduce_is_the_rounded_fp64_mean(M):
    gen = np.random.Generator(np.random.PCG64(M))
    rows = gen.uniform(0.1, 9, M).astype(np.float32)
    labels = np.where(gen.uniform(size=M) < 0.3, -100, 5)
    labels[0] = 5
    conf = gen.uniform(0, 1, M).astype(np.float32)
    rd, ld_, cd = (torch.from_numpy(a).to(G.DEV) for a in (rows, labels, conf))
    a = reduce_call(rd, labels=ld_)
    assert U.reduce_matches(a, U.reduce_reference(rows, labels=labels)), (a, U.reduce_reference(rows, labels=labels))
    assert reduce_call(rd, labels=ld_).tobytes() == a.tobytes()                        # two runs, the same bits
    b = reduce_call(rd, weight=cd, scale=6.67)
    assert U.reduce_matches(b, U.reduce_reference(rows, weight=conf, scale=6.67))
    assert reduce_call(rd, weight=cd, scale=6.67).tobytes() == b.tobytes()
    assert U.reduce_matches(reduce_call(rd), U.reduce_reference(rows))                 # no weight: all ones
    assert np.isnan(reduce_call(rd, labels=torch.full((M,), -100, device=G.DEV)))      # no row counts: NaN, as torch
    with pytest.raises(ValueError):
        reduce_call(rd, weight=cd, labels=ld_)


def test_loss_total_adds_in_transformers_order():
    vals = np.asarray([4.6762013, 0.66830236, 6.0986114, 7.838683, 2.8063495, 2.4481301], np.float32)
    terms = torch.from_numpy(vals).to(G.DEV)
    for present in (0, 1, 0x3f, 0x1c, 0x2b, 0x14, 0x20):
        out = torch.full((2,), 77.0, dtype=torch.float32, device=G.DEV)
        L.call("vk_loss_total", G.P(terms), present, G.P(out), G.stream())
        torch.cuda.synchronize()
        want = U.total_reference({k: vals[i] for i, k in enumerate(TERM_KEYS) if present & (1 << i)})
        assert out.cpu().numpy().tobytes() == np.asarray([want, 77.0], np.float32).tobytes(), present


# ---- 4. the model, fp32 against transformers' vectors -----------------------------------------------------------------------------
def logits_of(out):
    """Every logit tensor of a call under the names the golden file and the oracle use; the visual scores as [B, V, columns]."""
    d = {"prediction_logits": out.prediction_logits, "cross_relationship_score": out.cross_relationship_score}
    if out.question_answering_score is not None:
        d["question_answering_score"] = out.question_answering_score
    for key, part in (out.visual_prediction_scores or {}).items():
        d[f"visual/{key}"] = part.view(out.cross_relationship_score.shape[0], -1, part.shape[1])
    return d


def close(a, b, tol):
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * abs(b)


@pytest.mark.parametrize("case", ["all", "mlm", "obj", "ans", "nan", "switched_off", "padded"])
def test_model_fp32_vs_transformers_golden(g, models, case):
    cname, kw, lab = U.case_args(g, case)
    out = models(cname, "fp32")(**kw, **lab)
    want, (total, terms) = U.case_logits(g, case), U.case_losses(g, case)
    got = logits_of(out)
    assert set(got) == {k for k in want if "obj_labels" in lab or not k.startswith("visual/")}       # upstream runs the visual head for obj_labels only
    errs = {k: rel(v, want[k]) for k, v in got.items()}
    lerr = {k: abs(float(out.losses[k]) - float(v)) / abs(float(v)) for k, v in terms.items() if np.isfinite(v) and v != 0}
    print(f"\n[LxmertForPreTraining fp32 vs transformers, {case}] logits rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          "; loss rel err " + " ".join(f"{k} {v:.2e}" for k, v in lerr.items()) + f"; total {float(out.loss):.6f} vs {float(total):.6f}", end="")
    assert max(errs.values()) <= 1e-3
    assert set(out.losses) == set(terms)
    for k, v in terms.items():
        assert out.losses[k].dtype == torch.float32 and close(out.losses[k], v, 1e-3), (k, float(out.losses[k]), float(v))
    assert close(out.loss, total, 1e-3)
    assert (out.question_answering_score is None) == (cname == "B")
    assert out.prediction_logits.shape == want["prediction_logits"].shape
    if case == "nan":
        assert np.isnan(float(out.loss)) and np.isnan(float(out.losses["mlm"])) and np.isfinite(float(out.losses["matched"]))
    if case == "obj":
        assert float(out.losses["attr"]) == 0.0                                        # a conf of zeros


def test_model_without_labels_has_no_loss(g, models, monkeypatch):
    _, kw, _ = U.case_args(g, "all")
    rec = Recorder(monkeypatch)
    out = models("A", "fp32")(**kw)
    assert out.loss is None and out.losses == {}
    assert not [n for n in rec.names() if n in ("vk_cross_entropy", "vk_smooth_l1_rows", "vk_loss_reduce", "vk_loss_total")]
    assert rel(out.prediction_logits, U.case_logits(g, "all")["prediction_logits"]) <= 1e-3


def test_loss_only_mode(g, models, monkeypatch):
    """logits=False: the labelled rows alone go through the transform, the decoder and the cross-entropy; the terms are the full
    call's; with no labelled row no GEMM over the word table is launched and mlm is NaN."""
    cfg, _ = U.golden_model(g)
    _, kw, lab = U.case_args(g, "all")
    m = models("A", "fp32")
    n = int((lab["labels"] != -100).sum())
    rec = Recorder(monkeypatch)
    out = m(**kw, **lab, logits=False)
    total, terms = U.case_losses(g, "all")
    assert out.prediction_logits is None and set(out.losses) == set(terms)
    print(f"\n[loss-only mode fp32] mlm {float(out.losses['mlm']):.6f} vs transformers {float(terms['mlm']):.6f}", end="")
    for k, v in terms.items():
        assert close(out.losses[k], v, 1e-3), k
    assert close(out.loss, total, 1e-3)
    gathers = [a for name, a in rec.calls if name == "vk_gather_rows"]
    assert len(gathers) == 1 and gathers[0][2] == n
    decoder = [a for name, a in rec.calls if name == "vk_linear" and a[7] == cfg["vocab_size"]]
    assert len(decoder) == 1 and decoder[0][1] == n and 0 < n < lab["labels"].numel()
    rec.calls.clear()
    _, _, none = U.case_args(g, "nan")
    out = m(**kw, **none, logits=False)
    assert np.isnan(float(out.losses["mlm"])) and np.isnan(float(out.loss)) and np.isfinite(float(out.losses["matched"]))
    assert not [a for name, a in rec.calls if name in ("vk_linear", "vk_gather_rows") and (name == "vk_gather_rows" or a[7] == cfg["vocab_size"])]


# ---- 5. reduced precision against the emulating oracle, with the attention kernel asserted -----------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_model_reduced_precision_vs_emulating_oracle(g, models, monkeypatch, precision):
    """Every logit tensor (the three column slices of the visual GEMM among them) and every loss term against the emulating
    oracle at the siblings' EPS."""
    tol = EPS[precision]
    cfg, sd = U.golden_model(g)
    _, kw, lab = U.case_args(g, "padded")
    m = models("A", precision)
    rec = Recorder(monkeypatch)
    out = m(**kw, **lab)
    monkeypatch.undo()
    # every attention of the forward on the small matrix-core kernel: 1 + 1 self-attention layers, 4 attentions in the cross layer
    H, heads, Lt, V = cfg["hidden_size"], cfg["num_attention_heads"], kw["input_ids"].shape[1], kw["visual_feats"].shape[1]
    assert rec.names("vk_attention") == ["vk_attention"] * 6
    for Lq, Lk in ((Lt, Lt), (V, V), (Lt, V), (V, Lt)):
        for ld in (H, 2 * H, 3 * H):
            assert L.load().vk_attention_route(Lq, Lk, H // heads, m.lxmert.dt, ld, ld, ld, 1, 0) == L.VK_ATT_ROUTE_MFMA
    oracle = U.PretrainOracle(cfg, sd, emulate=precision).heads(**{k: v.numpy() for k, v in kw.items()})
    got = logits_of(out)
    assert set(got) == set(oracle)
    errs = {k: rel(v, oracle[k]) for k, v in got.items()}
    o_total, o_terms = U.losses_reference(cfg, oracle, lab)
    lerr = {k: abs(float(out.losses[k]) - v) / abs(v) for k, v in o_terms.items()}
    print(f"\n[LxmertForPreTraining {precision} vs emulating oracle] logits " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          "; losses " + " ".join(f"{k} {v:.2e}" for k, v in lerr.items()), end="")
    assert max(errs.values()) <= tol and max(lerr.values()) <= tol and close(out.loss, o_total, tol)
    # the losses the kernels made of the model's OWN logits: float64 from the stored values, to fp32 rounding
    _, own_terms = U.losses_reference(cfg, got, lab)
    assert set(own_terms) == set(TERM_KEYS)
    for k, v in own_terms.items():
        assert close(out.losses[k], v, 1e-5), (k, float(out.losses[k]), v)


# ---- 6. graph replay -------------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(g, models):
    """One logits=True call captured into a HIP graph replays bit-identically, follows new labels of the same shape, and repeats
    the host checks."""
    _, kw, lab = U.case_args(g, "padded")
    m = models("A", "bf16")

    def snapshot(o):
        return [o.loss.clone(), o.prediction_logits.clone(), o.cross_relationship_score.clone(), o.question_answering_score.clone()] + \
            [o.losses[k].clone() for k in TERM_KEYS]
    eager = snapshot(m(**kw, **lab))
    replay = m.capture(**kw, **lab)
    got = replay(**kw, **lab)
    torch.cuda.synchronize()
    for a, b in zip(snapshot(got), eager):
        assert torch.equal(a, b)
    obj = lab["obj_labels"]
    lab2 = dict(labels=torch.roll(lab["labels"], 2, dims=1), matched_label=1 - lab["matched_label"], ans=torch.roll(lab["ans"], 1),
                obj_labels={"obj": (torch.roll(obj["obj"][0], 1, dims=1), obj["obj"][1]), "attr": (obj["attr"][0], torch.roll(obj["attr"][1], 1, dims=0)),
                            "feat": (obj["feat"][0] * 0.5, 1 - obj["feat"][1])})
    eager2 = snapshot(m(**kw, **lab2))
    got2 = replay(**kw, **lab2)
    torch.cuda.synchronize()
    for a, b in zip(snapshot(got2), eager2):
        assert torch.equal(a, b)
    assert not torch.equal(eager2[0], eager[0]) and all(not torch.equal(a, b) for a, b in zip(eager2[4:], eager[4:]))
    with pytest.raises(IndexError):
        replay(**kw, **dict(lab2, ans=torch.tensor([0, 11, 0])))
    with pytest.raises(ValueError):
        replay(**kw, **{k: v for k, v in lab2.items() if k != "ans"})                 # the capture had answers


# ---- 7. LxmertForQuestionAnswering with labels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_question_answering_loss(g, monkeypatch, precision):
    """(loss, score) with labels: the loss is CrossEntropyLoss() of the returned scores (float64 from the stored values, within
    the mean of the rows' bounds and one rounding); without labels the scores have the same bits and no loss kernel runs."""
    from vltk_amd.lxmert import LxmertForQuestionAnswering, make_lxmert_qa_state_dict
    cfg, _ = U.golden_model(g)
    enc_cfg = {k: v for k, v in cfg.items() if k not in LP.PRETRAIN_DEFAULTS}
    nqa = 11
    m = LxmertForQuestionAnswering(enc_cfg, nqa, precision=precision).load_state_dict(make_lxmert_qa_state_dict(enc_cfg, nqa, 7))
    _, kw, _ = U.case_args(g, "padded")
    rec = Recorder(monkeypatch)
    score = m(**kw)
    plain = rec.names()
    rec.calls.clear()
    labels = torch.tensor([10, -100, 0])
    loss, score2 = m(**kw, labels=labels)
    assert isinstance(score, torch.Tensor) and torch.equal(score, score2)
    assert rec.names() == plain + ["vk_cross_entropy", "vk_loss_reduce"]
    td = TDT[m.lxmert.dt]
    r = U.ce_reference(score2, labels.numpy())
    ref = U.reduce_reference(r["ref"], labels=labels.numpy())
    bound = U.ce_bound(r, U.ce_form(nqa, score2.stride(0), td), td)[r["keep"]].mean() + U.U32 * abs(ref)
    assert loss.dtype == torch.float32 and abs(float(loss) - ref) <= bound, (float(loss), ref, bound)
    with pytest.raises(IndexError):
        m(**kw, labels=torch.tensor([11, 0, 0]))
    with pytest.raises(ValueError):
        m(**kw, labels=torch.tensor([1, 0]))


# ---- 8. default geometry -----------------------------------------------------------------------------------------------------------
def test_default_geometry_runs_both_cross_entropy_forms(monkeypatch):
    """transformers' default geometry at B = 2, bf16, all labels: the masked-LM and the visual cross-entropies run the vector form
    (30 522 columns at a stride of 30 528; slices of the 4048-column visual GEMM), the matched head the scalar one; the losses are
    finite and are the float64 losses of the returned logits; loss-only gives the same mlm to 2e-3 (its decoder GEMM has other
    rows, so an accumulation-order difference may flip single bf16 roundings of a logit, 4e-3 of about 1 against a loss of 10)."""
    cfg = LP.lxmert_pretraining_config()
    m = LP.LxmertForPreTraining(cfg, precision="bf16").load_state_dict(LP.make_lxmert_pretraining_state_dict(cfg, 1))
    gen = np.random.Generator(np.random.PCG64(0))
    B, Lt, V = 2, 20, 36
    kw = dict(input_ids=torch.from_numpy(gen.integers(1, cfg["vocab_size"], (B, Lt))),
              visual_feats=torch.from_numpy(np.maximum(gen.standard_normal((B, V, 2048)), 0).astype(np.float32)),
              visual_pos=torch.from_numpy(gen.uniform(0, 1, (B, V, 4)).astype(np.float32)))
    labels = torch.from_numpy(np.where(gen.uniform(size=(B, Lt)) < 0.15, gen.integers(0, cfg["vocab_size"], (B, Lt)), -100))
    labels[0, 0] = cfg["vocab_size"] - 1
    lab = dict(labels=labels, matched_label=torch.tensor([1, 0]), ans=torch.tensor([9499, -100]),
               obj_labels={"obj": (torch.from_numpy(gen.integers(0, 1600, (B, V))), torch.from_numpy(gen.uniform(0, 1, (B, V)).astype(np.float32))),
                           "attr": (torch.from_numpy(gen.integers(0, 400, (B, V))), torch.from_numpy(gen.uniform(0, 1, (B, V)).astype(np.float32))),
                           "feat": (torch.from_numpy(gen.standard_normal((B, V, 2048)).astype(np.float32)), torch.ones((B, V)))})
    rec = Recorder(monkeypatch)
    out = m(**kw, **lab)
    forms = []
    for name, a in rec.calls:
        if name == "vk_cross_entropy":
            forms.append((a[3], L.load().vk_cross_entropy_form(a[3], a[1], a[7], int(a[0] % 16 == 0))))
    assert forms == [(30522, L.VK_CE_FORM_VEC), (2, L.VK_CE_FORM_SCALAR), (1600, L.VK_CE_FORM_VEC), (400, L.VK_CE_FORM_VEC),
                     (9500, L.VK_CE_FORM_VEC)]
    assert out.prediction_logits.shape == (B, Lt, 30522) and out.question_answering_score.shape == (B, 9500)
    assert all(np.isfinite(float(v)) for v in out.losses.values()) and np.isfinite(float(out.loss))
    _, own = U.losses_reference(cfg, logits_of(out), lab)
    assert set(own) == set(TERM_KEYS)
    for k, v in own.items():
        assert close(out.losses[k], v, 1e-5), (k, float(out.losses[k]), v)
    only = m(**kw, **lab, logits=False)
    assert only.prediction_logits is None and close(only.losses["mlm"], out.losses["mlm"], 2e-3)
