"""-m gpu: the 3x3 panel kernel storing its rows through an index (csrc/conv3x3_panel.hip, OIDX) against the
path it replaces in Res5 block 0: the dense-output launch, then a gather of the rows that are kept.

Nothing here has a tolerance.  The indexed store changes where a row goes and whether it is stored, not one bit of it, so the
kernel under test (vk_conv2d_rows_out) is held torch.equal to vk_conv2d_rows followed by a row gather done here, on the exact
integer data of tests/exact_util.py; one shape also holds that dense launch to float64 arithmetic rounded once.  The output
buffer is the dense row count plus guard rows on both sides (so that even a launch that ignored the index would stay inside
it), every element pre-filled with one NaN bit pattern: each row the index does not name, and every guard row, must keep the
pattern bit for bit, so neither a stray nor a dropped store can hide.  The route and the two queries the launcher itself
reads are asserted around every launch.  The host-side answers and refusals are in tests/test_panel_out_indexed_host.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_util as X                         # noqa: E402
import gpu_util as G                           # noqa: E402
import test_gpu_conv_exact as E                # noqa: E402
from roi_dedupe_util import crafted_boxes     # noqa: E402
from roi_nbr_util import neighbourhood_table  # noqa: E402
from roi_out_rows_util import out_rows        # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

SWITCHES = ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_DYNAMIC", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_PANEL_OUT_INDEXED",
            "VK_CONV3X3_PANEL")
GUARD = 64                                     # rows in front of and behind the output
PATTERN = 0x7E55                               # a quiet f16 NaN with a payload no arithmetic produces

# (N, H, W, Cin, Cout), all 3x3, dilation 2, pad 2: the smallest shapes at which the form can go wrong
SHAPES = [(16, 14, 14, 512, 512),              # 3136 rows: six full 512-row tiles and a ragged one, four column tiles, sixteen stages
          (32, 14, 14, 128, 256),              # two groups of 16 RoIs, 12.25 row tiles, no dynamic tail
          (16, 10, 6, 128, 256)]               # non-square even map, 960 rows: the second tile is ragged
KINDS = ("identity", "one_row", "every_second", "reversed", "table")


def _case(shape, relu):
    N, H, W, cin, cout = shape
    return X.Case(f"panel_out_indexed/{N}x{H}x{W}_{cin}_{cout}", "panel", "conv", N, H, W, cin, cout, 3, 1, 2, 2, relu=relu,
                  seed_name=f"panel_out_indexed/{N}x{H}x{W}_{cin}_{cout}")


def _id(shape):
    return "x".join(str(v) for v in shape[:3]) + f"_{shape[3]}_{shape[4]}"


def _clear(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _queries(c):
    lib = L.load()
    return (G.conv_route(**c.route_geometry()), lib.vk_panel_phase_indexed(c.N, c.H, c.W, c.dil, c.cout),
            lib.vk_panel_out_indexed(c.N, c.H, c.W, c.dil, c.cout))


@functools.lru_cache(maxsize=None)
def _inputs(shape, with_x_idx):
    """(x rows f16 [U, cin], x_idx i32 [M] (identity over the dense rows without an input index), packed w, bias, the float64
    tensors): made once per shape and never written.  With an input index x holds U = M / 5 rows, read with repeats."""
    c = _case(shape, 0)                         # (the data does not depend on the ReLU: seed_name, and no residual)
    M = c.M
    x, w, bias, _ = X.make_inputs(c, G.DEV)
    rows64 = E._rows(x)
    if with_x_idx:
        U = max(M // 5, 1)
        g = torch.Generator().manual_seed(1000 * M + shape[3])
        idx = torch.randint(0, U, (M,), generator=g).to(torch.int32).to(G.DEV)
        rows64 = rows64[:U]
    else:
        U = M
        idx = torch.arange(M, dtype=torch.int32, device=G.DEV)
    wd, bd = E._pack(c, w, bias)
    return rows64.to(torch.float16).contiguous(), idx, wd, bd, (rows64, w, bias)


@functools.lru_cache(maxsize=None)
def _dense(shape, with_x_idx, relu):
    """The reference: the dense-output launch (vk_conv2d_rows) on the same input, [M, cout]; computed once, never written."""
    c = _case(shape, relu)
    xu, idx, wd, bd, _ = _inputs(shape, with_x_idx)
    y = torch.full((c.M, c.cout), float("nan"), dtype=torch.float16, device=G.DEV)
    assert _queries(c)[:2] == ("panel", 1)
    L.call("vk_conv2d_rows", G.P(xu), xu.shape[0], G.P(idx), c.N, c.H, c.W, c.cin, G.P(wd), G.P(bd), None, G.P(y), c.cout, c.dil, relu,
           G.stream())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any()) and float(y.float().abs().max()) > 0
    return y


@functools.lru_cache(maxsize=None)
def _crafted_keep():
    """Which dense rows are their neighbourhood's representative on crafted_boxes over two images (32 RoIs, 6272 rows), and the
    table itself."""
    rois = crafted_boxes([(10, 14), (10, 14)])
    assert len(rois) == 32
    _, nid, rep, _ = neighbourhood_table(rois, 2, 10, 14, 14, 2)
    o = out_rows(nid, rep)
    return o >= 0, o


def _y_index(kind, M):
    """(V, y_idx [M] int64 numpy): every entry -1 or in [0, V), every id of [0, V) exactly once."""
    m = np.arange(M, dtype=np.int64)
    if kind == "identity":
        o = m
    elif kind == "one_row":                     # every row -1 but one, inside the ragged last tile's neighbourhood
        o = np.where(m == (2 * M) // 3 + 1, 0, -1)
    elif kind == "every_second":
        o = np.where(m % 2 == 0, m // 2, -1)
    elif kind == "reversed":
        o = M - 1 - m
    else:                                       # the real table: the kept rows of crafted_boxes, numbered in row order as rep is
        keep, table = _crafted_keep()
        keep = keep[:M]
        o = np.where(keep, np.cumsum(keep) - 1, -1)
        if M == len(table):
            assert np.array_equal(o, table)     # (the whole table is exactly that numbering)
        assert 0 < int(keep.sum()) < M
    V = int(o.max()) + 1
    assert np.array_equal(np.sort(o[o >= 0]), np.arange(V)) and int(o.min()) >= -1
    return V, o


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_x_idx", [False, True], ids=["dense_in", "indexed_in"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_indexed_store_equals_dense_then_gather(shape, with_x_idx, kind, relu, monkeypatch):
    _clear(monkeypatch)
    c = _case(shape, relu)
    M = c.M
    xu, idx, wd, bd, _ = _inputs(shape, with_x_idx)
    want_dense = _dense(shape, with_x_idx, relu)
    V, o = _y_index(kind, M)
    y_idx = torch.from_numpy(o.astype(np.int32)).to(G.DEV)
    buf = torch.full((GUARD + M + GUARD, c.cout), PATTERN, dtype=torch.int16, device=G.DEV)
    want = buf.clone()
    kept = torch.from_numpy(np.nonzero(o >= 0)[0]).to(G.DEV)
    want[GUARD + torch.from_numpy(o[o >= 0]).to(G.DEV)] = want_dense.view(torch.int16)[kept]      # the row gather, here
    y = buf[GUARD:]
    assert _queries(c) == ("panel", 1, 1)
    L.call("vk_conv2d_rows_out", G.P(xu), xu.shape[0], G.P(idx) if with_x_idx else None, c.N, c.H, c.W, c.cin, G.P(wd), G.P(bd), None,
           G.P(y), V, G.P(y_idx), c.cout, c.dil, relu, G.stream())
    assert _queries(c) == ("panel", 1, 1)
    torch.cuda.synchronize()
    if not torch.equal(buf, want):
        bad = (buf != want).any(dim=1).nonzero().flatten() - GUARD
        stored = ((buf != PATTERN).any(dim=1).nonzero().flatten() - GUARD)
        raise AssertionError(f"{_id(shape)} {kind}: {bad.numel()} rows of the buffer differ (row numbers relative to y, V = {V}): "
                             f"{bad[:12].tolist()}...; rows written: {stored.numel()}, last {stored[-3:].tolist()}")
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + V:] == PATTERN).all())


def test_dense_reference_exact_on_integer_data(monkeypatch):
    """The absolute anchor for the reference above: the dense launch on the first shape, through the repeated input index, against
    float64 arithmetic on the gathered tensor rounded once, whole-tensor equality."""
    _clear(monkeypatch)
    shape = SHAPES[0]
    c = _case(shape, 1)
    _, idx, _, _, (rows64, w, bias) = _inputs(shape, True)
    x = rows64[idx.long()].view(c.N, c.H, c.W, c.cin).permute(0, 3, 1, 2).contiguous()
    v, want = X.expected(c, x, w, bias, None)
    X.check_conditions(c, x, w, bias, None, v, want)
    del v
    E.assert_exact(c, _dense(shape, True, 1), E._rows(want))
