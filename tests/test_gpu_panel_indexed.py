"""-m gpu: the 3x3 panel kernel reading its input through a row index (csrc/conv3x3_panel.hip, IDX) against
the path it replaces in Res5 block 0: vk_gather_rows into the dense tensor, then the unindexed launch.

Nothing here has a tolerance.  A row's bits do not depend on where its input row lives: the two paths bring the same bytes
into the same LDS places and issue the same matrix instructions on them in the same order, so the outputs are torch.equal
on the f16 bits.  The route and vk_panel_phase_indexed -- the function the launcher itself reads -- are asserted around every
launch, so a test cannot pass on the wrong form.  Equality of the two paths could hide a bug they share (they share the
whole K loop), so one shape also runs on the integer data of tests/exact_util.py against float64 arithmetic rounded once,
and the small model runs with the switch on and off.

The index is a contract: every entry lies in [0, x_rows).  No test feeds the device an index outside it.  The host-side
answers (the query under each switch, the refusals) are in tests/test_panel_indexed_host.py, which needs no GPU.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_util as X                         # noqa: E402
import gpu_util as G                           # noqa: E402
import test_gpu_conv_exact as E                # noqa: E402
import test_gpu_panel_tall as T                # noqa: E402
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

F16 = L.VK_F16
SWITCHES = ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_DYNAMIC", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_CONV3X3_PANEL")

# ((N, H, W, Cin, Cout), residual, ReLU), all 3x3, dilation 2, pad 2: the smallest shapes at which the form can go wrong.  The
# route needs N a multiple of 16, Cin >= 128 and Cout a multiple of 256.
CASES = [(T.ONE_GROUP, False, 0),                       # W/2 = 7, 6.125 row tiles, one looped stage pair
         (T.TWO_GROUPS, False, 0),                      # two groups: halo pieces come from the neighbouring group
         (T.CENTRE_ONLY, False, 0),                     # W/2 = 1: every piece clamped, centre tap only
         ((16, 4, 4, 128, 256), False, 0),              # the three windows overlap
         ((16, 10, 6, 128, 256), False, 0),             # non-square, ragged
         ((16, 14, 14, 192, 512), True, 1)]             # six stages x four column tiles, with residual and ReLU
KINDS = ("identity", "zeros", "last", "repeats", "one_row", "permutation")


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _indexed(shape):
    N, H, W, _, cout = shape
    return L.load().vk_panel_phase_indexed(N, H, W, 2, cout)


def _index(kind, M, seed):
    """(rows of x, idx [M] int32 on the device): every entry in [0, rows)."""
    g = torch.Generator().manual_seed(seed)
    U = max(M // 5, 1)
    if kind == "identity":
        U, idx = M, torch.arange(M)
    elif kind == "zeros":
        idx = torch.zeros(M, dtype=torch.int64)
    elif kind == "last":
        idx = torch.full((M,), U - 1)
    elif kind == "repeats":
        idx = torch.randint(0, U, (M,), generator=g)
    elif kind == "one_row":
        U, idx = 1, torch.zeros(M, dtype=torch.int64)
    else:
        U, idx = M, torch.randperm(M, generator=g)
    assert int(idx.min()) >= 0 and int(idx.max()) < U
    return U, idx.to(torch.int32).to(G.DEV)


def _launch_indexed(shape, res, relu, xu, U, idx):
    """The indexed launch on (xu [U, cin], idx), the form asserted on both sides of it."""
    N, H, W, cin, cout = shape
    _, wd, bd, rd = T._data(shape)
    assert xu.shape == (U, cin) and xu.is_contiguous() and idx.numel() == N * H * W
    y = torch.full((N * H * W, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    assert G.conv_route(N, H, W, cin, cout, k=3, pad=2, dil=2, relu=relu, res=res) == "panel" and _indexed(shape) == 1
    L.call("vk_conv2d_rows", G.P(xu), U, G.P(idx), N, H, W, cin, G.P(wd), G.P(bd), G.P(rd if res else None), G.P(y), cout, 2, relu,
           G.stream())
    assert _indexed(shape) == 1
    torch.cuda.synchronize()
    return y


def _launch_gathered(shape, res, relu, xu, idx):
    """Today's path: vk_gather_rows into the dense [M, cin] tensor, then the unindexed launch (route asserted by G.launch)."""
    N, H, W, cin, cout = shape
    _, wd, bd, rd = T._data(shape)
    M = N * H * W
    dense = torch.full((M, cin), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_gather_rows", G.P(xu), G.P(idx), M, cin * 2, G.P(dense), G.stream())
    y = torch.full((M, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    G.launch("vk_conv2d", G.P(dense), N, H, W, cin, G.P(wd), G.P(bd), G.P(rd if res else None), G.P(y), cout, cout, 3, 3, 1, 2, 2, 1,
             relu, F16, F16, G.stream(), expect_route="panel")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=T._id)
def test_indexed_equals_gather_then_dense(case, kind, monkeypatch):
    shape, res, relu = case
    _clear(monkeypatch)
    N, H, W, cin, _ = shape
    M = N * H * W
    U, idx = _index(kind, M, 100 * M + cin + KINDS.index(kind))
    xu = T._data(shape)[0].view(M, cin)[:U].contiguous()
    want = _launch_gathered(shape, res, relu, xu, idx)
    got = _launch_indexed(shape, res, relu, xu, U, idx)
    T._same_bits(f"{T._id(case)} {kind}", got, want)
    if kind == "identity":                     # ... and the plain unindexed launch on the same tensor
        T._same_bits(f"{T._id(case)} identity, unindexed", T._launch(shape, res, relu), want)


def test_dynamic_tail_same_bits(monkeypatch):
    """4116 tiles: the last sixteenth is drawn from the counter.  The static walk, the default and VK_PANEL_INDEXED=0 (gather,
    then the dense launch) give the same tensor."""
    _clear(monkeypatch)
    N, H, W, cin, cout = T.TAIL
    M = N * H * W
    assert -(-M // 512) * (cout // 128) >= 4096
    U, idx = _index("repeats", M, 4116)
    xu = T._data(T.TAIL)[0].view(M, cin)[:U].contiguous()
    monkeypatch.setenv("VK_PANEL_DYNAMIC", "0")
    want = _launch_indexed(T.TAIL, True, 1, xu, U, idx)
    monkeypatch.delenv("VK_PANEL_DYNAMIC")
    got = _launch_indexed(T.TAIL, True, 1, xu, U, idx)
    T._same_bits("dynamic tail, indexed", got, want)
    del got
    monkeypatch.setenv("VK_PANEL_INDEXED", "0")
    assert _indexed(T.TAIL) == 0
    dense = _launch_gathered(T.TAIL, True, 1, xu, idx)
    T._same_bits("dynamic tail, gather + dense", dense, want)


ANCHOR = X.Case("panel_indexed/16x14x14_512", "panel", "conv", 16, 14, 14, 128, 512, 3, 1, 2, 2, res=True, relu=1)


def test_indexed_exact_on_integer_data(monkeypatch):
    """The absolute anchor: the integer data of tests/exact_util.py through a repeated index (U = M / 5 distinct rows), against
    float64 arithmetic on the gathered tensor rounded once, whole-tensor equality."""
    _clear(monkeypatch)
    c = ANCHOR
    M = c.M
    U, idx = _index("repeats", M, 14)
    x, w, bias, res = X.make_inputs(c, G.DEV)
    xu64 = E._rows(x)[:U]                                          # [U, cin] float64 integers
    x = xu64[idx.long()].view(c.N, c.H, c.W, c.cin).permute(0, 3, 1, 2).contiguous()       # the tensor the launch stands for
    v, want = X.expected(c, x, w, bias, res)
    X.check_conditions(c, x, w, bias, res, v, want)
    del v
    wd, bd = E._pack(c, w, bias)
    xu = xu64.to(torch.float16).contiguous()
    rd = E._rows(res).to(torch.float16).contiguous()
    y = torch.full((M, c.cout), float("nan"), dtype=torch.float16, device=G.DEV)
    assert G.conv_route(**c.route_geometry()) == "panel" and L.load().vk_panel_phase_indexed(c.N, c.H, c.W, c.dil, c.cout) == 1
    L.call("vk_conv2d_rows", G.P(xu), U, G.P(idx), c.N, c.H, c.W, c.cin, G.P(wd), G.P(bd), G.P(rd), G.P(y), c.cout, c.dil, c.relu,
           G.stream())
    assert L.load().vk_panel_phase_indexed(c.N, c.H, c.W, c.dil, c.cout) == 1
    torch.cuda.synchronize()
    E.assert_exact(c, y, E._rows(want))


STAGES = ("res4", "feature_pooled", "obj_logits", "attr_logits")


def _model_on_off(monkeypatch, topk, chunk):
    """The small model with VK_PANEL_INDEXED=0 and with the default (the switch is re-read per launch): every output and stage
    torch.equal.  Returns the (dedupe_chunks, indexed_chunks) each of the two forwards added."""
    _clear(monkeypatch)
    monkeypatch.setenv("VK_CONV_GEMM4", "2")        # conv_gemm4, and with it the dedupe path, also at the few tiles of these shapes
    cfg = vg_c4_config(post_nms_topk=topk, detections=12)
    sd = make_state_dict(cfg, seed=1234)
    shapes = torch.tensor([[160, 224], [144, 200]])
    x = synthetic_images(2, 160, 224, seed=21)
    for i, (hh, ww) in enumerate(shapes.tolist()):
        x[i, :, hh:, :] = 0
        x[i, :, :, ww:] = 0
    x = torch.from_numpy(x).cuda()
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    if chunk:
        m.set_option("head_chunk", chunk)

    def run():
        n0 = [m.get_option(k) for k in ("dedupe_chunks", "indexed_chunks")]
        out = {k: v.clone() for k, v in m.forward_async(images=x, image_shapes=shapes).wait_raw().items()}
        st = {s: m.get_stage(s).clone() for s in STAGES}
        return out, st, tuple(m.get_option(k) - a for k, a in zip(("dedupe_chunks", "indexed_chunks"), n0))

    monkeypatch.setenv("VK_PANEL_INDEXED", "0")
    ref, ref_st, n_ref = run()
    monkeypatch.delenv("VK_PANEL_INDEXED")
    got, got_st, n_got = run()
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    for s in STAGES:
        assert torch.equal(got_st[s], ref_st[s]), s
    assert float(ref_st["feature_pooled"].float().abs().max()) > 0 and ref_st["feature_pooled"].shape[0] == 2 * topk
    return n_ref, n_got


def test_model_same_bits(monkeypatch):
    """2 x 32 = 64 RoIs, one chunk of four groups of 16: conv2 of block 0 reads through the index, and only with the switch on."""
    assert L.load().vk_panel_phase_indexed(64, 14, 14, 2, 512) == 1
    n_ref, n_got = _model_on_off(monkeypatch, 32, 0)
    assert n_ref == (1, 0) and n_got == (1, 1)


def test_model_chunk_not_of_whole_groups(monkeypatch):
    """2 x 36 = 72 RoIs in chunks of 40: the chunk of 40 (40 % 16 != 0) takes the gather and the dense launch, whatever the
    switch says; the tail of 32 reads through the index.  Both chunks take the dedupe path either way."""
    lib = L.load()
    assert lib.vk_panel_phase_indexed(40, 14, 14, 2, 512) == 0 and lib.vk_panel_phase_indexed(32, 14, 14, 2, 512) == 1
    n_ref, n_got = _model_on_off(monkeypatch, 36, 40)
    assert n_ref == (2, 0) and n_got == (2, 1)
