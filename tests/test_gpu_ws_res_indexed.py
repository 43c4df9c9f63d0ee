"""-m gpu: conv_ws's indexed-residual build (csrc/conv_ws.hip RIDX) through vk_conv1x1_res_rows against the path
it replaces: vk_gather_rows of the residual into the dense tensor, then the plain build.  Whole-tensor bit equality.

The index is a contract: every entry is a row of the residual.  No test feeds the device an index outside it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                           # noqa: E402
from test_gpu_roi_dedupe import conv_weights   # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

KINDS = ("identity", "zeros", "last", "permutation", "repeats")
# The entry point launches the kernel whatever the row count (the dispatcher sends it layers from 1024 rows on).  Row counts: one
# tile; a ragged last tile (200 = 3 * 64 + 8); 16 tiles, one per workgroup and most workgroups without any; and 4100 rows of 2048
# channels, 65 tiles (the last of 4 rows) on 32 M lanes: workgroups with three tiles, two tiles, and the index a tile ahead of each
SHAPES = [(64, 256), (200, 256), (1000, 256), (64, 512), (200, 512), (1000, 512), (4100, 2048)]


def index(kind, M, seed):
    """(rows of the residual, idx [M] int32 on the device): every entry in [0, rows)."""
    g = torch.Generator().manual_seed(seed)
    V = max(M // 5, 1)
    if kind == "identity":
        V, idx = M, torch.arange(M)
    elif kind == "zeros":
        idx = torch.zeros(M, dtype=torch.int64)
    elif kind == "last":
        idx = torch.full((M,), V - 1)
    elif kind == "repeats":
        idx = torch.randint(0, V, (M,), generator=g)
    else:
        V, idx = M, torch.randperm(M, generator=g)
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    return V, idx.to(torch.int32).to(G.DEV)


@pytest.fixture(scope="module")
def data():
    """Per (M, cout): x [M, 512], a residual pool of M rows, weights and bias, made once."""
    out = {}
    for M, cout in SHAPES:
        g = torch.Generator().manual_seed(M + cout)
        x = torch.randn((M, 512), generator=g).half().to(G.DEV)
        res = torch.randn((M, cout), generator=g).half().to(G.DEV)
        out[(M, cout)] = (x, res) + tuple(conv_weights(cout, 512, M + cout))
    return out


def launch(x, w, b, res, idx, cout, relu):
    M = x.shape[0]
    y = torch.full((M, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_conv1x1_res_rows", G.P(x), 512, M, G.P(w), G.P(b), G.P(res), G.P(idx), G.P(y), cout, relu, G.stream())
    torch.cuda.synchronize()
    return y


@pytest.fixture(autouse=True)
def small_launches(monkeypatch):
    monkeypatch.delenv("VK_CONV_WS", raising=False)
    monkeypatch.delenv("VK_WS_WAVES", raising=False)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,cout", SHAPES)
def test_indexed_equals_gather_then_plain(data, M, cout, kind, relu):
    x, pool, w, b = data[(M, cout)]
    V, idx = index(kind, M, 7 * M + cout + KINDS.index(kind))
    res_v = pool[:V].contiguous()
    dense = torch.full((M, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_gather_rows", G.P(res_v), G.P(idx), M, cout * 2, G.P(dense), G.stream())
    want = launch(x, w, b, dense, None, cout, relu)
    # the plain build through this entry point is the dispatcher's launch of the layer: on this kernel from 1024 rows on, on
    # another one below (a layer's bits do not depend on the kernel that runs it)
    via_dispatcher = torch.full((M, cout), float("nan"), dtype=torch.float16, device=G.DEV)
    G.launch("vk_conv2d", G.P(x), 1, 1, M, 512, G.P(w), G.P(b), G.P(dense), G.P(via_dispatcher), cout, cout, 1, 1, 1, 0, 1, 1, relu,
             L.VK_F16, L.VK_F16, G.stream(), expect_route="ws" if M >= 1024 else G.conv_route(1, 1, M, 512, cout, relu=relu, res=True))
    torch.cuda.synchronize()
    assert torch.equal(via_dispatcher.view(torch.int16), want.view(torch.int16)), (M, cout, kind, relu, "plain build")
    got = launch(x, w, b, res_v, idx, cout, relu)
    assert not bool(torch.isnan(want.float()).any())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (M, cout, kind, relu)
    if kind == "repeats":                      # the residual matters: another index gives another tensor
        other = launch(x, w, b, res_v, torch.zeros_like(idx), cout, relu)
        assert not torch.equal(other.view(torch.int16), want.view(torch.int16))
