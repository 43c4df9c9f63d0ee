"""-m gpu: attention at any sequence length: attention_tiled_kernel (matrix cores, online soft-max) and
attention_stream_kernel (strict fp32) through vk_attention_tiled and vk_attention, each launch with the route it must take;
then the encoder at 40 text / 140 visual tokens against transformers' vectors, and the grid-feature chain at 140 rows.

The op-level reference is test_gpu_lxmert.py::test_attention's: fp32 soft-max, the probabilities rounded to the storage type
where a matrix-core kernel runs (they round P before the second product) and unrounded otherwise, at that file's EPS."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.lxmert_oracle import LxmertOracle          # noqa: E402
from vltk_amd import _lib as L                         # noqa: E402
from vltk_amd.lxmert import LxmertEncoder, LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict, \
    make_lxmert_state_dict                            # noqa: E402

import gpu_util as G                                   # noqa: E402
from lxmert_util import case_kwargs, golden_inputs     # noqa: E402
from test_gpu_lxmert import EPS, TDT, rel              # noqa: E402

IDS = {L.VK_F32: "fp32", L.VK_F16: "fp16", L.VK_BF16: "bf16"}
ALL = [L.VK_F32, L.VK_F16, L.VK_BF16]
ROUTES = ("mfma", "lds", "tiled", "stream")            # VK_ATT_ROUTE_* by value
FMIN = float(np.finfo(np.float32).min)


def attention(entry, q, k, v, mask, B, heads, Lq, Lk, d, dt, expect):
    """One launch of `entry` on device tensors (q / k / v may be column slices: the row stride is the parent's width), with the
    kernel it must run on asked of the dispatcher immediately before, under the same environment."""
    aligned = int((q.data_ptr() | k.data_ptr() | v.data_ptr()) % 16 == 0)
    got = L.load().vk_attention_route(Lq, Lk, d, dt, q.stride(0), k.stride(0), v.stride(0), aligned, int(entry == "vk_attention_tiled"))
    assert got >= 0 and ROUTES[got] == expect, f"{entry} at Lq={Lq} Lk={Lk} d={d}: route {got}, the test expects {expect}"
    out = torch.empty((B * Lq, heads * d), dtype=TDT[dt], device=G.DEV)
    L.call(entry, G.P(q), q.stride(0), G.P(k), k.stride(0), G.P(v), v.stride(0), G.P(mask), G.P(out), heads * d, B, heads, Lq, Lk, d,
           dt, G.stream())
    torch.cuda.synchronize()
    return out


def old_route(dt, Lq, Lk, d):
    """vk_attention's rule on aligned fused projections."""
    if dt != L.VK_F32 and d in (32, 64) and Lq <= 48 and Lk <= 64:
        return "mfma"
    if ((Lq + Lk) * (d + 1) + Lk * d + Lq * (Lk + 1)) * 4 <= 160 * 1024:
        return "lds"
    return "tiled" if dt != L.VK_F32 and d in (32, 64) else "stream"


def new_route(dt, d):
    return "tiled" if dt != L.VK_F32 and d in (32, 64) else "stream"


def mixed_mask(B, Lk):
    """Batch 0: the second half of the keys masked; batch 1: only the last key live (every leading tile is all finfo.min);
    batch 2: everything masked (the soft-max of equal scores: the uniform average, finite); further batches unmasked."""
    m = np.ones((B, Lk), np.float32)
    m[0, Lk // 2:] = 0
    if B > 1:
        m[1, :Lk - 1] = 0
    if B > 2:
        m[2, :] = 0
    return torch.from_numpy((1.0 - m) * np.finfo(np.float32).min)


def reference(q, k, v, add, B, heads, Lq, Lk, d, td, round_p):
    H = heads * d
    qh = q.float().view(B, Lq, heads, d).transpose(1, 2)
    kh = k.float().reshape(B, Lk, heads, d).transpose(1, 2)
    vh = v.float().reshape(B, Lk, heads, d).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / d ** 0.5
    if add is not None:
        s = s + add[:, None, None, :]
    p = F.softmax(s, -1)
    return ((p.to(td).float() if round_p else p) @ vh).permute(0, 2, 1, 3).reshape(B * Lq, H).to(td).float()


def check_vs_torch(dt, B, heads, Lq, Lk, d, masked=True, entries=("vk_attention_tiled", "vk_attention")):
    """q, k, v are column slices of fused projections [rows, 2H] (q the second half of its own); B * heads is no multiple of 4."""
    assert (B * heads) % 4 != 0
    gen = np.random.Generator(np.random.PCG64(Lq * Lk))
    td, H = TDT[dt], heads * d
    qq = torch.from_numpy(gen.standard_normal((B * Lq, 2 * H)).astype(np.float32)).to(td)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H)).astype(np.float32)).to(td)
    add = mixed_mask(B, Lk) if masked else None
    qd, kvd, md = qq.to(G.DEV), kv.to(G.DEV), add.to(G.DEV) if masked else None
    refs = {}
    worst = 0.0
    for entry in entries:
        route = new_route(dt, d) if entry == "vk_attention_tiled" else old_route(dt, Lq, Lk, d)
        out = attention(entry, qd[:, H:], kvd[:, :H], kvd[:, H:], md, B, heads, Lq, Lk, d, dt, route)
        round_p = route in ("mfma", "tiled")
        if round_p not in refs:
            refs[round_p] = reference(qq[:, H:], kv[:, :H], kv[:, H:], add, B, heads, Lq, Lk, d, td, round_p)
        assert torch.isfinite(out.float()).all()
        e = rel(out, refs[round_p])
        worst = max(worst, e)
        print(f"\n[attention {IDS[dt]} {entry} -> {route}] Lq {Lq} Lk {Lk} d {d}: rel err {e:.2e} (bound {EPS[dt]:.0e})", end="")
        assert e <= EPS[dt], (entry, route, Lq, Lk, d, e)
    return worst


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("Lk", [63, 64, 65, 96, 97, 127, 128, 129, 192, 193, 257])
def test_key_lengths_vs_torch(dt, Lk):
    """Around every 16-, 32- and 64-key boundary of the tiles, 17 queries (a second, one-row query block)."""
    check_vs_torch(dt, 3, 3, 17, Lk, 64)


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("Lq", [1, 15, 16, 17, 48, 49, 65, 100])
def test_query_lengths_vs_torch(dt, Lq):
    """One query, the 16- and 32-query blocks' edges, the small kernel's last length and the first past it."""
    check_vs_torch(dt, 3, 3, Lq, 100, 64)
    check_vs_torch(dt, 3, 3, Lq, 100, 64, masked=False, entries=("vk_attention_tiled",))


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("Lq,Lk,d", [(196, 196, 64), (200, 333, 32)])
def test_grid_sized_vs_torch(dt, Lq, Lk, d):
    check_vs_torch(dt, 3, 3, Lq, Lk, d)


@pytest.mark.parametrize("dt", [L.VK_F32, L.VK_BF16], ids=["fp32", "bf16"])
def test_1024_vs_torch(dt):
    """The longest the extractor emits.  fp16 is left out: a CPU emulation of the tiled arithmetic reached 9.5e-4 of EPS's 1e-3
    at this length."""
    check_vs_torch(dt, 3, 1, 1024, 1024, 64)


@pytest.mark.parametrize("d,ld_extra", [(48, 0), (64, 4)])
def test_sixteen_bit_streams_what_the_matrix_cores_refuse(d, ld_extra):
    """Head dim 48, and rows 8 bytes off the 16-byte grid: the streaming kernel, P not rounded."""
    B, heads, Lq, Lk, dt = 3, 3, 37, 150, L.VK_BF16
    gen = np.random.Generator(np.random.PCG64(d + ld_extra))
    H = heads * d
    ld = H + ld_extra
    q = torch.from_numpy(gen.standard_normal((B * Lq, ld)).astype(np.float32)).to(torch.bfloat16)
    k = torch.from_numpy(gen.standard_normal((B * Lk, ld)).astype(np.float32)).to(torch.bfloat16)
    v = torch.from_numpy(gen.standard_normal((B * Lk, ld)).astype(np.float32)).to(torch.bfloat16)
    add = mixed_mask(B, Lk)
    qd, kd, vd = q.to(G.DEV), k.to(G.DEV), v.to(G.DEV)
    ref = reference(q[:, :H].contiguous(), k[:, :H].contiguous(), v[:, :H].contiguous(), add, B, heads, Lq, Lk, d, torch.bfloat16, False)
    for entry in ("vk_attention_tiled", "vk_attention"):
        route = "stream" if entry == "vk_attention_tiled" or old_route(L.VK_F32, Lq, Lk, d) == "stream" else "lds"
        out = attention(entry, qd[:, :H], kd[:, :H], vd[:, :H], add.to(G.DEV), B, heads, Lq, Lk, d, dt, route)
        assert rel(out, ref) <= EPS[dt]


# ---- exact ------------------------------------------------------------------------------------------------------------
def kernels_of(dt, monkeypatch):
    """(label, set-up) of the new kernels that take this type: tiled needs a 16-bit type, streaming takes every type (a 16-bit
    call reaches it with the matrix cores switched off)."""
    if dt == L.VK_F32:
        return [("stream", lambda: None)]
    return [("tiled", lambda: monkeypatch.delenv("VK_ATTENTION_MFMA", raising=False)),
            ("stream", lambda: monkeypatch.setenv("VK_ATTENTION_MFMA", "0"))]


# (Lk, d): the head dim 64 cases keep the ids they had before d = 32 (the tiled kernel's D = 32 builds) joined them
UNIFORM = [(Lk, d) for d in (64, 32) for Lk in (128, 256, 1024)]
UNIFORM_IDS = [str(Lk) if d == 64 else f"{Lk}-d{d}" for Lk, d in UNIFORM]


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
@pytest.mark.parametrize("Lk,d", UNIFORM, ids=UNIFORM_IDS)
def test_exact_uniform_average(dt, Lk, d, monkeypatch):
    """q = 0: every live key weighs the same, so with integer v the output is the fp32 value sum(v) / count rounded once to the
    storage type, whatever the tiling: unmasked, the first half of the keys masked (leading tiles all masked) and every odd key
    masked.  Head dim 64 and 32 (the seed is Lk alone, so the d = 64 data is what it was)."""
    B, heads, Lq, td = 1, 3, 33, TDT[dt]
    gen = np.random.Generator(np.random.PCG64(Lk))
    H = heads * d
    q = torch.zeros((B * Lq, H), dtype=td, device=G.DEV)
    k = torch.from_numpy(gen.standard_normal((B * Lk, H)).astype(np.float32)).to(td).to(G.DEV)
    vi = torch.from_numpy(gen.integers(-8, 9, (B * Lk, H)).astype(np.float32))
    v = vi.to(td).to(G.DEV)
    lives = [np.ones(Lk, bool), np.arange(Lk) >= Lk // 2, np.arange(Lk) % 2 == 0]
    for label, setup in kernels_of(dt, monkeypatch):
        setup()
        for live in lives:
            add = None if live.all() else torch.from_numpy(np.where(live, 0.0, FMIN).astype(np.float32)[None]).to(G.DEV)
            out = attention("vk_attention_tiled", q, k, v, add, B, heads, Lq, Lk, d, dt, label)
            want = (vi[torch.from_numpy(live)].sum(0) / np.float32(live.sum())).to(td)
            assert torch.equal(out.cpu(), want[None].expand(B * Lq, H)), (label, int(live.sum()))


ONE_HOT = [(dt, d) for d in (64, 32) for dt in ALL]


@pytest.mark.parametrize("dt,d", ONE_HOT, ids=[IDS[dt] if d == 64 else f"{IDS[dt]}-d{d}" for dt, d in ONE_HOT])
def test_exact_one_hot(dt, d, monkeypatch):
    """q = 32 e0 and one key j* = 32 e0, the others 0: the scaled gap is 1024 / sqrt(d) >= 128, every other weight underflows to 0
    and the output row is v[j*] bit for bit.  One batch per j*: first, last, and both sides of every multiple of 32 up to Lk = 257."""
    Lk, Lq, td = 257, 5, TDT[dt]
    stars = sorted({0, Lk - 1} | {m - 1 for m in range(32, Lk, 32)} | {m for m in range(32, Lk, 32)})
    B = len(stars)
    gen = np.random.Generator(np.random.PCG64(7))
    q = torch.zeros((B * Lq, d), dtype=td)
    q[:, 0] = 32
    k = torch.zeros((B, Lk, d), dtype=td)
    for b, j in enumerate(stars):
        k[b, j, 0] = 32
    v = torch.from_numpy(gen.standard_normal((B, Lk, d)).astype(np.float32)).to(td)
    want = torch.stack([v[b, j] for b, j in enumerate(stars)])[:, None, :].expand(B, Lq, d).reshape(B * Lq, d)
    for label, setup in kernels_of(dt, monkeypatch):
        setup()
        out = attention("vk_attention_tiled", q.to(G.DEV), k.view(B * Lk, d).to(G.DEV), v.view(B * Lk, d).to(G.DEV), None, B, 1, Lq, Lk,
                        d, dt, label)
        assert torch.equal(out.cpu(), want), label


@pytest.mark.parametrize("dt", ALL, ids=[IDS[d] for d in ALL])
def test_two_calls_same_bytes(dt):
    B, heads, Lq, Lk, d, td = 2, 3, 70, 200, 64, TDT[dt]
    gen = np.random.Generator(np.random.PCG64(3))
    H = heads * d
    q = torch.from_numpy(gen.standard_normal((B * Lq, H)).astype(np.float32)).to(td).to(G.DEV)
    kv = torch.from_numpy(gen.standard_normal((B * Lk, 2 * H)).astype(np.float32)).to(td).to(G.DEV)
    add = mixed_mask(B, Lk).to(G.DEV)
    a = attention("vk_attention_tiled", q, kv[:, :H], kv[:, H:], add, B, heads, Lq, Lk, d, dt, new_route(dt, d))
    b = attention("vk_attention_tiled", q, kv[:, :H], kv[:, H:], add, B, heads, Lq, Lk, d, dt, new_route(dt, d))
    assert torch.equal(a, b)


# ---- the encoder ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lxmert_long.npz"))


@pytest.fixture(scope="module")
def long_inputs(g):
    cfg, sd, feats = golden_inputs(g)
    return cfg, sd, torch.from_numpy(g["input_ids"]), torch.from_numpy(feats), torch.from_numpy(g["visual_pos"])


@pytest.mark.parametrize("tag", ["masked", "plain"])
def test_encoder_fp32_vs_transformers_long(g, long_inputs, tag):
    """40 text and 140 visual tokens: the 140 x 140 self-attention is past the LDS kernel in fp32 (the streaming kernel)."""
    cfg, sd, ids, feats, pos = long_inputs
    assert L.load().vk_attention_route(140, 140, 64, L.VK_F32, 384, 384, 384, 1, 0) == L.VK_ATT_ROUTE_STREAM
    m = LxmertEncoder(cfg, precision="fp32").load_state_dict(sd)
    kw = {k: torch.from_numpy(v) for k, v in case_kwargs(g, tag).items()}
    lang, visn, pooled = m(ids, feats, pos, **kw)
    errs = (rel(lang, g[f"{tag}/language_output"]), rel(visn, g[f"{tag}/vision_output"]), rel(pooled, g[f"{tag}/pooled_output"]))
    print(f"\n[LXMERT 40 + 140 tokens fp32 vs transformers, {tag}] rel err lang {errs[0]:.2e} visn {errs[1]:.2e} pooled {errs[2]:.2e}")
    assert max(errs) <= 1e-3


@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("fp16", 6e-3)])
def test_encoder_reduced_precision_vs_emulating_oracle_long(g, long_inputs, precision, tol):
    """Every attention of this geometry runs the tiled kernel, which rounds P where the emulating oracle always has."""
    cfg, sd, ids, feats, pos = long_inputs
    m = LxmertEncoder(cfg, precision=precision).load_state_dict(sd)
    kw = case_kwargs(g, "masked")
    lang, visn, pooled = m(ids, feats, pos, **{k: torch.from_numpy(v) for k, v in kw.items()})
    o_lang, o_visn, o_pooled = LxmertOracle(cfg, sd, emulate=precision).forward(g["input_ids"], feats.numpy(), g["visual_pos"], **kw)
    errs = (rel(lang, o_lang), rel(visn, o_visn), rel(pooled, o_pooled))
    print(f"\n[LXMERT 40 + 140 tokens {precision} vs emulating oracle] lang {errs[0]:.2e} visn {errs[1]:.2e} pooled {errs[2]:.2e}"
          f" (bound {tol:.0e})")
    assert max(errs) <= tol


def test_graph_replay_matches_eager_long(g, long_inputs):
    cfg, sd, ids, feats, pos = long_inputs
    m = LxmertEncoder(cfg, precision="bf16").load_state_dict(sd)
    am, vm = torch.from_numpy(g["attention_mask"]), torch.from_numpy(g["visual_attention_mask"])
    eager = [t.clone() for t in m(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)]
    replay = m.capture(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)
    got = replay(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    ids2 = torch.roll(ids, 1, dims=1)
    eager2 = [t.clone() for t in m(ids2, feats, pos, attention_mask=am, visual_attention_mask=vm)]
    got2 = replay(ids2, feats, pos, attention_mask=am, visual_attention_mask=vm)
    torch.cuda.synchronize()
    for a, b in zip(got2, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(eager2[0], eager[0])


@pytest.fixture(scope="module")
def full_size():
    cfg = lxmert_config()
    return cfg, LxmertEncoder(cfg, precision="bf16").load_state_dict(make_lxmert_state_dict(cfg, 1))


@pytest.mark.parametrize("V", [100, 196])
def test_encoder_full_size_more_visual_tokens(full_size, V):
    """transformers' default geometry with 100 boxes and a 14 x 14 grid's cells: finite, bit-reproducible, correctly shaped."""
    cfg, m = full_size
    gen = np.random.Generator(np.random.PCG64(V))
    ids = torch.from_numpy(gen.integers(1, cfg["vocab_size"], (2, 20)))
    feats = torch.from_numpy(np.maximum(gen.standard_normal((2, V, 2048)), 0).astype(np.float32))
    pos = torch.from_numpy(gen.uniform(0, 1, (2, V, 4)).astype(np.float32))
    a = m(ids, feats, pos)
    b = m(ids, feats, pos)
    for u, w in zip(a, b):
        assert torch.isfinite(u.float()).all() and torch.equal(u, w)
    assert a[0].shape == (2, 20, 768) and a[1].shape == (2, V, 768) and a[2].shape == (2, 768)


def test_question_answering_long(g, long_inputs):
    """LxmertForQuestionAnswering inherits the routing: its bf16 answers are its fp32 run's."""
    cfg, _, ids, feats, pos = long_inputs
    nqa = 40
    sd = make_lxmert_qa_state_dict(cfg, nqa, int(g["seed"]))
    kw = {k: torch.from_numpy(v) for k, v in case_kwargs(g, "masked").items()}
    s32 = LxmertForQuestionAnswering(cfg, nqa, precision="fp32").load_state_dict(sd)(ids, feats, pos, **kw)
    s16 = LxmertForQuestionAnswering(cfg, nqa, precision="bf16").load_state_dict(sd)(ids, feats, pos, **kw)
    ref = LxmertOracle(cfg, sd).qa_forward(g["input_ids"], feats.numpy(), g["visual_pos"], **case_kwargs(g, "masked"))
    assert s32.shape == (2, nqa) and rel(s32, ref) <= 1e-3
    assert s16.float().argmax(-1).cpu().tolist() == s32.argmax(-1).cpu().tolist()


def test_encoder_200_text_1024_visual_tokens():
    """Nothing else of the encoder depends on length: the embedding's position walk, the pooler's stride-Lq row pick and
    capture() at 200 text tokens and 1024 visual rows (hidden 128, one layer of each kind), fp32 against the oracle."""
    cfg = lxmert_config(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, l_layers=1, x_layers=1, r_layers=1,
                        max_position_embeddings=256, visual_feat_dim=128)
    sd = make_lxmert_state_dict(cfg, 11)
    gen = np.random.Generator(np.random.PCG64(11))
    B, Lq, V = 2, 200, 1024
    ids = torch.from_numpy(gen.integers(1, 300, (B, Lq)))
    feats = torch.from_numpy(np.maximum(gen.standard_normal((B, V, 128)), 0).astype(np.float32))
    pos = torch.from_numpy(gen.uniform(0, 1, (B, V, 4)).astype(np.float32))
    am = torch.ones((B, Lq))
    am[1, 150:] = 0
    vm = torch.ones((B, V))
    vm[0, 1000:] = 0
    got = LxmertEncoder(cfg, precision="fp32").load_state_dict(sd)(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)
    ref = LxmertOracle(cfg, sd).forward(ids.numpy(), feats.numpy(), pos.numpy(), attention_mask=am.numpy(), visual_attention_mask=vm.numpy())
    for a, b in zip(got, ref):
        assert rel(a, b) <= 1e-3
    m = LxmertEncoder(cfg, precision="bf16").load_state_dict(sd)
    eager = [t.clone() for t in m(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)]
    replay = m.capture(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)
    out = replay(ids, feats, pos, attention_mask=am, visual_attention_mask=vm)
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_grid_features_into_lxmert_chain():
    """FRCNN (C4, depth 50, fp16) grid features of a 10 x 14 grid -> 140 rows per image -> LXMERT (fp32), checked against the
    LXMERT oracle fed with the same features."""
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    fcfg = vg_c4_config(depth=50, post_nms_topk=30, detections=12)
    det = FRCNN(fcfg).load_state_dict(make_state_dict(fcfg, seed=1234)).eval()
    x = torch.from_numpy(synthetic_images(2, 160, 224, seed=9))
    out = det(x, torch.tensor([[160, 224], [160, 224]]), grid=(10, 14), padding="max_detections", max_detections=140, return_tensors="pt")
    feats, boxes = out["roi_features"].float().cpu(), out["normalized_boxes"].float().cpu()
    assert feats.shape == (2, 140, 2048) and boxes.shape == (2, 140, 4) and out["preds_per_image"].tolist() == [140, 140]
    cfg = lxmert_config(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, l_layers=1, x_layers=2, r_layers=1,
                        max_position_embeddings=16)
    sd = make_lxmert_state_dict(cfg, 5)
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).integers(1, 300, (2, 7)))
    got = LxmertEncoder(cfg, precision="fp32").load_state_dict(sd)(ids, feats, boxes)
    ref = LxmertOracle(cfg, sd).forward(ids.numpy(), feats.numpy(), boxes.numpy())
    for a, b in zip(got, ref):
        assert rel(a, b) <= 1e-3
