"""CPU: the exact-integer data of tests/test_gpu_conv_exact.py is sound for every case of its table, proven without a GPU.

For each case (a large one on its first ~3000 output rows, with the full case's weights and bias): conditions (i) - (iii)
of tests/exact_util.py -- every partial sum below 2^24, the rounding and its ties exercised, nothing non-finite outside the
overflow case -- and the claim the method rests on: fp32 arithmetic gives the float64 result whatever the order, shown by
running the convolution in fp32 in two channel orders."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as X
import test_gpu_conv_exact as E


@pytest.mark.parametrize("case", E.EXACT_CASES, ids=[c.name for c in E.EXACT_CASES])
def test_exact_case_is_sound(case):
    c = X.host_subset(case)
    x, w, bias, res = X.make_inputs(c)
    v, y = X.expected(c, x, w, bias, res)
    exact_bound = float(X.conv64(x.abs(), w.abs(), c).max())
    total, (rounded, ties) = X.check_conditions(c, x, w, bias, res, v, y, bound=exact_bound)
    X.check_conditions(c, x, w, bias, res, v, y)            # and with the cheap bound the GPU test uses
    # fp32, two channel orders (per group): both equal the float64 result
    cg = x.shape[1] // c.groups
    perm = torch.cat([torch.randperm(cg, generator=torch.Generator().manual_seed(1)) + g * cg for g in range(c.groups)])
    wperm = torch.randperm(cg, generator=torch.Generator().manual_seed(1))
    s = 2.0 ** 12 if c.edge == "subnormal" else 1.0         # (the scaled case: compare the integers)
    ref = X.conv64(x * s, w * s, c)
    for xs, ws_ in ((x, w), (x[:, perm], w[:, wperm])):
        got = F.conv2d((xs * s).float(), (ws_ * s).float(), None, c.stride, c.pad, c.dil, c.groups)
        assert torch.equal(got.double(), ref), c.name


def test_table_names_every_route_and_edge():
    routes = {c.route for c in E.EXACT_CASES}
    assert routes == {"generic", "ring", "duo", "ws", "gemm4", "panel", "blk"}
    for r in routes:
        for edge in X.EDGES[1:]:
            assert any(c.route == r and c.edge == edge for c in E.EXACT_CASES), (r, edge)
        assert any(c.route == r and c.edge == "overflow" and not c.relu for c in E.EXACT_CASES), r      # -inf, not only +inf and 0
    for c in E.EXACT_CASES:                                 # VK_PANEL_MI=9 where 9 row tiles are illegal would silently run 8
        if ("VK_PANEL_MI", "9") in c.env:
            assert E.S.panel_mi9_legal(c.W, c.dil), c.name
    assert {c.route for c in E.EXACT_CASES if c.kind == "mean"} == {"ws", "duo"}
    assert any(c.dt == X.BF16 and c.route == "duo" for c in E.EXACT_CASES)


def test_a_truncating_store_would_be_seen():
    """What the method is for: on this data a store that truncates instead of rounding to nearest even differs on more than a
    tenth of the outputs (the max-normalised 1e-3 of the parity tests admits it)."""
    c = next(c for c in E.EXACT_CASES if c.name == "generic/f16/1x1")
    x, w, bias, res = X.make_inputs(c)
    v, y = X.expected(c, x, w, bias, res)
    trunc = torch.where(y.double().abs() > v.abs(), (y.view(torch.int16) - 1).view(torch.float16), y)
    assert float((trunc != y).float().mean()) > 0.10
    assert float((trunc.double() - v).abs().max() / v.abs().max()) < 1e-3


@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("shape", E.BNECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bottleneck64_data_is_sound(shape, proj):
    p = X.make_bneck(proj, *shape)
    layers, bounds = X.bneck_expected(p, proj)
    stats = X.check_bneck_conditions(layers, bounds)
    print(shape, proj, bounds, stats)


@pytest.mark.parametrize("shape,caffe", E.STEM_CASES)
def test_stem_data_is_sound(shape, caffe):
    import numpy as np
    x, w, beta = X.make_stem(*shape)
    v, y, pooled = X.stem_expected(x, w, beta, caffe)
    assert float(F.conv2d(x, w.abs(), None, 2, 3).max() + beta.abs().max()) < X.LIMIT
    assert bool(torch.isfinite(y.double()).all())
    rounded, ties = X.rounding_stats(v, y)
    assert rounded >= 0.20 and ties >= 0.03, (rounded, ties)
    wp, bp = E.pack_stem(w, beta)
    got = np.sort(wp.view(np.float16).astype(np.float64))
    want = np.sort(np.concatenate([w.numpy().ravel(), np.zeros(got.size - w.numel())]))
    np.testing.assert_array_equal(got, want)                # the packed bytes decode to the integers (and padding zeros)
    np.testing.assert_array_equal(bp[:64], beta.numpy().astype(np.float32))


@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
@pytest.mark.parametrize("edge", X.EDGES[1:])
def test_bottleneck64_edge_data_is_sound(edge, proj):
    p = X.make_bneck(proj, *E.BNECK_SHAPES[0], edge=edge)
    layers, bounds = X.bneck_expected(p, proj)
    X.check_bneck_conditions(layers, bounds, edge)
    y = layers[2][1].double()
    if edge == "overflow":                                  # the ReLU leaves +inf and 0
        assert bool((y == float("inf")).any()) and bool((y[:, 2::16] == 0).all())
    if edge == "spike":                                     # the spike's trace stands three orders above the typical output
        assert float(y.max()) >= 1000 * max(float(y.median()), 1.0)


@pytest.mark.parametrize("edge", X.EDGES[1:])
def test_stem_edge_data_is_sound(edge):
    import numpy as np
    shape, caffe = E.STEM_CASES[0]
    x, w, beta = X.make_stem(*shape, edge=edge)
    v, y, pooled = X.stem_expected(x, w, beta, caffe)
    scale = 2.0 ** 24 if edge == "subnormal" else 1.0
    assert float(F.conv2d(x, w.abs(), None, 2, 3).max()) * scale + float(beta.abs().max()) < X.LIMIT
    assert torch.equal(x.half().double(), x) and torch.equal(w.half().double(), w)        # exact in f16
    if edge == "overflow":
        assert bool((pooled.double() == float("inf")).any()) and not bool(torch.isnan(pooled.double()).any())
    else:
        assert bool(torch.isfinite(y.double()).all())
    if edge == "subnormal":
        a = pooled.double().abs()
        assert float(((a > 0) & (a < 2.0 ** -14)).float().mean()) >= 0.05
    wp, bp = E.pack_stem(w, beta)
    got = np.sort(wp.view(np.float16).astype(np.float64))
    np.testing.assert_array_equal(got, np.sort(np.concatenate([w.numpy().ravel(), np.zeros(got.size - w.numel())])))
    np.testing.assert_array_equal(bp[:64], beta.numpy().astype(np.float32))
