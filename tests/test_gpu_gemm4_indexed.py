"""-m gpu: the fused conv3 + shortcut GEMM of Res5 block 0 over the distinct neighbourhoods as the head launches
it -- vk_gather_rows_dev of the first input's representative rows, then the DD form of conv_gemm4 with the row count on the
device and the second input read through the index -- against today's launch on both inputs gathered.  Bit equality.

conv_gemm4 is launched from 2048 rows on (eight row tiles), so the dense row counts are 2156 (ragged: 8 * 256 + 108) and 2560;
the first input is gathered in front of the launch, not indexed inside it (DESIGN.md 6h says why).
No test feeds a kernel an index outside its range."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                           # noqa: E402
from test_gpu_roi_dedupe import conv_weights   # noqa: E402
from vltk_amd import _lib as L                 # noqa: E402

KINDS = ("identity", "zeros", "last", "permutation", "repeats", "one_row")


@pytest.fixture(autouse=True)
def small_grids(monkeypatch):
    monkeypatch.setenv("VK_CONV_GEMM4", "2")        # conv_gemm4 also at the few tiles of these shapes (re-read per launch)


def families(kind, M, seed):
    """(V, rep [M] rows of the first input, idx_rep [M] rows of the second, U rows of the second): entries from V on are filled
    with -1 and must never be read."""
    g = torch.Generator().manual_seed(seed)
    V = U = max(M // 5, 1)
    if kind == "identity":
        V = U = M
        rep, ir = torch.arange(M), torch.arange(M)
    elif kind == "zeros":
        rep, ir = torch.zeros(V, dtype=torch.int64), torch.zeros(V, dtype=torch.int64)
    elif kind == "last":
        rep, ir = torch.full((V,), M - 1), torch.full((V,), U - 1)
    elif kind == "permutation":
        V = U = M
        rep, ir = torch.randperm(M, generator=g), torch.randperm(M, generator=g)
    elif kind == "repeats":
        rep, ir = torch.randint(0, M, (V,), generator=g), torch.randint(0, U, (V,), generator=g)
    else:
        V, U = 1, 3
        rep, ir = torch.tensor([M - 1]), torch.tensor([2])
    pad = torch.full((M - V,), -1, dtype=torch.int64)
    return V, torch.cat([rep, pad]).to(torch.int32).to(G.DEV), torch.cat([ir, pad]).to(torch.int32).to(G.DEV), U


@pytest.fixture(scope="module")
def data():
    out = {}
    for M in (2156, 2560):
        g = torch.Generator().manual_seed(M)
        out[M] = (torch.randn((M, 512), generator=g).half().to(G.DEV), torch.randn((M, 1024), generator=g).half().to(G.DEV))
    w = {cout: conv_weights(cout, 512 + 1024, cout) for cout in (256, 512)}
    return out, w


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cout", [256, 512])
@pytest.mark.parametrize("M", [2156, 2560])
def test_over_distinct_rows(data, M, cout, kind):
    xs, ws = data
    t2, pool = xs[M]
    w, b = ws[cout]
    V, rep, idx_rep, U = families(kind, M, M + cout + KINDS.index(kind))
    pooled_u = pool[:U].contiguous()
    v_dev = torch.tensor([V], dtype=torch.int32, device=G.DEV)
    # the head's launches
    t2_v = torch.full((M, 512), float("nan"), dtype=torch.float16, device=G.DEV)
    L.call("vk_gather_rows_dev", G.P(t2), G.P(rep), M, G.P(v_dev), 1024, G.P(t2_v), G.stream())
    y_v = torch.full((M, cout), 3.0, dtype=torch.float16, device=G.DEV)
    L.call("vk_conv1x1_rows", G.P(t2_v), 512, G.P(pooled_u), 1024, M, G.P(v_dev), G.P(idx_rep), G.P(w), G.P(b), G.P(y_v), cout, 1, G.stream())
    # today's: both inputs dense
    x1 = torch.zeros((M, 512), dtype=torch.float16, device=G.DEV)
    x2 = torch.zeros((M, 1024), dtype=torch.float16, device=G.DEV)
    x1[:V] = t2[rep[:V].long()]
    x2[:V] = pooled_u[idx_rep[:V].long()]
    y_ref = torch.zeros((M, cout), dtype=torch.float16, device=G.DEV)
    G.launch("vk_conv1x1_dual", G.P(x1), 512, G.P(x2), 1024, M, G.P(w), G.P(b), None, G.P(y_ref), cout, 1, G.stream(), expect_route="gemm4")
    torch.cuda.synchronize()
    assert bool(torch.isnan(t2_v[V:].float()).all()) and not bool(torch.isnan(t2_v[:V].float()).any())     # the gather stops at V
    assert bool((y_v[V:] == 3.0).all())                                                                    # ... and so does the GEMM
    assert torch.equal(y_v[:V].view(torch.int16), y_ref[:V].view(torch.int16)), (M, cout, kind)
    assert float(y_ref[:V].float().abs().max()) > 0.5
    if kind not in ("identity", "permutation"):
        assert (V + 255) // 256 < (M + 255) // 256          # the device's row count leaves row tiles of the grid unwalked
