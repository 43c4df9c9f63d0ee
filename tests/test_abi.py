"""CPU (-m "not gpu"): the C-ABI library loads and exports every symbol include/vltk_hip.h declares;
host-only entry points (weight packing, geometry helpers, argument validation) behave."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vltk_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(L.SIGNATURES), (declared ^ set(L.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.vk_version() == 1


def test_struct_layout_matches_header(lib):
    # vk_config: 7 ints, int+8f, int+8f, f, int, f, (pad) double, 2 ints, 4f, 6 ints, 4f, int  -> checked via sizeof
    assert C.sizeof(L.vk_roi_params) == 8 + 8 * 8 + 8
    assert C.sizeof(L.vk_outputs) == 7 * 8
    assert L.vk_config.rpn_nms_thresh.offset % 8 == 0


def test_stem_geometry(lib):
    ho, wo = C.c_int(), C.c_int()
    lib.vk_stem_out_hw(800, 1333, 1, C.byref(ho), C.byref(wo))
    assert (ho.value, wo.value) == (200, 333)
    lib.vk_stem_out_hw(800, 1333, 0, C.byref(ho), C.byref(wo))
    assert (ho.value, wo.value) == (200, 334)
    lib.vk_stem_out_hw(160, 224, 1, C.byref(ho), C.byref(wo))
    assert (ho.value, wo.value) == (40, 56)



def _resnet101_blocks(H, W):
    """(stage, block, cin, bottleneck width, cout, stride, projection, input H, input W) of every res2..res5 block of
    ResNet-101 behind a stem that gives H x W."""
    cin = 64
    for name, n, mid, cout, stride in (("res2", 3, 64, 256, 1), ("res3", 4, 128, 512, 2), ("res4", 23, 256, 1024, 2),
                                       ("res5", 3, 512, 2048, 2)):
        for b in range(n):
            s = stride if b == 0 else 1
            yield name, b, cin, mid, cout, s, b == 0, H, W
            H, W, cin = (H - 1) // s + 1, (W - 1) // s + 1, cout


@pytest.mark.parametrize("dt", [L.VK_F16, L.VK_F32], ids=["fp16", "fp32"])
def test_block_rules_resnet101(lib, dt, monkeypatch):
    """The two block predicates the C4 model and the FPN detector both ask, for every ResNet-101 block of a
    32 x 800 x 1333 batch (the FPN detector's stem: 200 x 334 into res2): in fp16 res2.0's projection shortcut is part of
    conv3's GEMM (the other stages start with stride 2) and res2's three blocks run as vk_bottleneck64; in fp32 neither."""
    for v in ("VK_BNECK_FUSED", "VK_BNECK_ROWS", "VK_NO_FUSED_SHORTCUT"):
        monkeypatch.delenv(v, raising=False)
    ho, wo = C.c_int(), C.c_int()
    lib.vk_stem_out_hw(800, 1333, 0, C.byref(ho), C.byref(wo))
    fused, whole = set(), set()
    for name, b, cin, mid, cout, s, proj, H, W in _resnet101_blocks(ho.value, wo.value):
        f = proj and lib.vk_fuse_shortcut(mid, cin, cout, s, dt) == 1
        if f:
            fused.add((name, b))
        if lib.vk_bottleneck64_eligible(cin, mid, cout, s, 1, 1, int(proj), int(f), 32, H, W, dt):
            whole.add((name, b))
    f16 = dt == L.VK_F16
    assert fused == ({("res2", 0)} if f16 else set())
    assert whole == ({("res2", 0), ("res2", 1), ("res2", 2)} if f16 else set())
    # the row form's 32-bit offsets: 64 images of 200 x 334 (2.19 GB of res2 map) still fit, 128 do not
    assert lib.vk_bottleneck64_eligible(256, 64, 256, 1, 1, 1, 0, 0, 64, 200, 334, dt) == int(f16)
    assert lib.vk_bottleneck64_eligible(256, 64, 256, 1, 1, 1, 0, 0, 128, 200, 334, dt) == 0
    monkeypatch.setenv("VK_BNECK_FUSED", "0")
    assert lib.vk_bottleneck64_eligible(256, 64, 256, 1, 1, 1, 0, 0, 32, 200, 334, dt) == 0

def _half_bits(a):
    return np.asarray(a, dtype=np.float16).view(np.uint16)


@pytest.mark.parametrize("dt,npdt", [(L.VK_F32, np.float32), (L.VK_F16, np.float16)])
def test_pack_conv_weight_folds_bn(lib, dt, npdt):
    g = np.random.Generator(np.random.PCG64(0))
    cout, cin, k = 5, 64, 3
    w = g.standard_normal((cout, cin, k, k)).astype(np.float32)
    bn = np.concatenate([g.uniform(0.5, 1.5, cout), g.standard_normal(cout), g.standard_normal(cout),
                         g.uniform(0.5, 1.5, cout)]).astype(np.float32)
    nbytes = lib.vk_packed_weight_bytes(cout, cin, k, k, 1, dt)
    cp = lib.vk_packed_cout(cout)
    assert cp == 128 and nbytes == cp * k * k * cin * np.dtype(npdt).itemsize
    wp = np.zeros(nbytes, np.uint8)
    bp = np.zeros(cp, np.float32)
    L.call("vk_pack_conv_weight", w.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p), None, cout, cin, k, k, 1, dt,
           wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    s = bn[:cout].astype(np.float64) / np.sqrt(bn[3 * cout:].astype(np.float64) + 1e-5)
    ref_w = (w.astype(np.float64) * s[:, None, None, None]).astype(np.float32).transpose(0, 2, 3, 1).reshape(cout, -1)
    ref_b = (bn[cout:2 * cout].astype(np.float64) - bn[2 * cout:3 * cout].astype(np.float64) * s).astype(np.float32)
    got = wp.view(npdt).reshape(cp, -1)
    np.testing.assert_array_equal(got[:cout], ref_w.astype(npdt))
    assert (got[cout:] == 0).all()
    np.testing.assert_array_equal(bp[:cout], ref_b)
    assert (bp[cout:] == 0).all()


@pytest.mark.parametrize("c,groups", [(128, 32), (256, 8), (256, 2), (32, 8)])
def test_pack_grouped_is_slice_diagonal(lib, c, groups):
    """Grouped 3x3 weights (BottleneckBlock conv2, frcnn.py:942-952) are packed as dense rows over the
    input-channel slice of each 64-channel output tile, zero outside the channel's own group."""
    g = np.random.Generator(np.random.PCG64(5))
    cpg, k = c // groups, 3
    w = g.standard_normal((c, cpg, k, k)).astype(np.float32)
    sw = lib.vk_conv_slice_channels(c, groups)
    assert sw == min(max(cpg, 64), c)
    nbytes = lib.vk_packed_weight_bytes(c, c, k, k, groups, L.VK_F32)
    cp = lib.vk_packed_cout(c)
    assert nbytes == cp * k * k * sw * 4
    wp = np.zeros(nbytes, np.uint8)
    bp = np.zeros(cp, np.float32)
    L.call("vk_pack_conv_weight", w.ctypes.data_as(C.c_void_p), None, None, c, c, k, k, groups, L.VK_F32,
           wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    got = wp.view(np.float32).reshape(cp, k * k, sw)
    for co in range(c):
        slice0 = (co // 64 * 64) // sw * sw
        g0 = co // cpg * cpg
        ref = np.zeros((k * k, sw), np.float32)
        ref[:, g0 - slice0:g0 - slice0 + cpg] = w[co].transpose(1, 2, 0).reshape(k * k, cpg)
        np.testing.assert_array_equal(got[co], ref)
    assert (got[c:] == 0).all()


def test_pack_grouped_rejects_odd_width(lib):
    assert lib.vk_conv_slice_channels(96, 8) == -1          # 12 channels per group: not a power of two
    w = np.zeros((96, 12, 3, 3), np.float32)
    out = np.zeros(1 << 20, np.uint8)
    b = np.zeros(128, np.float32)
    with pytest.raises(ValueError, match="power of two"):
        L.call("vk_pack_conv_weight", w.ctypes.data_as(C.c_void_p), None, None, 96, 96, 3, 3, 8, L.VK_F32,
               out.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))


def test_pack_rejects_bad_cin(lib):
    w = np.zeros((4, 3, 1, 1), np.float32)
    out = np.zeros(1 << 16, np.uint8)
    b = np.zeros(128, np.float32)
    with pytest.raises(ValueError, match="K-tiles"):
        L.call("vk_pack_conv_weight", w.ctypes.data_as(C.c_void_p), None, None, 4, 3, 1, 1, 1, L.VK_F16,
               out.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))


def test_workspace_sizes(lib):
    assert lib.vk_rpn_workspace_bytes(2, 63000, 6000) > 2 * 6000 * 94 * 8
    assert lib.vk_nms_workspace_bytes(300) > 300 * 16
    assert lib.vk_stem_workspace_bytes(1, 800, 1333, 64, L.VK_F16) > 400 * 667 * 64 * 2


def _clear_switches(monkeypatch):
    for v in list(os.environ):
        if v.startswith("VK_"):
            monkeypatch.delenv(v)


def _resnet101_c4_convs(lib, dt, batch=32, rois=300):
    """(layer, gpu_util.conv_route arguments) of every convolution launch of ResNet-101-C4 on a batch of 800 x 1333 images:
    res2 whole, res3 / res4 as the two half-batches the model runs on two streams, the RPN head on res4, res5 (stride 1,
    dilation 2) on batch x rois RoIs of 14 x 14 with the spatial mean folded into the last conv3 in fp16 (model.hip
    run_block).  res2's blocks are listed layer by layer although fp16 runs them as vk_bottleneck64
    (test_block_rules_resnet101): that is what VK_BNECK_FUSED=0 launches."""
    ho, wo = C.c_int(), C.c_int()
    lib.vk_stem_out_hw(800, 1333, 1, C.byref(ho), C.byref(wo))
    blocks = [(n, b, cin, mid, cout, s, proj, batch if n == "res2" else batch // 2, H, W, 1)
              for n, b, cin, mid, cout, s, proj, H, W in _resnet101_blocks(ho.value, wo.value) if n != "res5"]
    H4, W4 = [((H - 1) // s + 1, (W - 1) // s + 1) for n, b, _, _, _, s, _, H, W in _resnet101_blocks(ho.value, wo.value) if n == "res4"][-1]
    blocks += [("res5", b, 1024 if b == 0 else 2048, 512, 2048, 1, b == 0, batch * rois, 14, 14, 2) for b in range(3)]
    for name, b, cin, mid, cout, s, proj, N, H, W, dil in blocks:
        tag = f"{name}.{b}"
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        fused = proj and lib.vk_fuse_shortcut(mid, cin, cout, s, dt) == 1
        mean = name == "res5" and b == 2 and dt == L.VK_F16
        if proj and not fused:
            yield tag + ".shortcut", dict(N=N, H=H, W=W, cin=cin, cout=cout, stride=s, dt=dt)
        yield tag + ".conv1", dict(N=N, H=H, W=W, cin=cin, cout=mid, stride=s, relu=1, dt=dt)
        yield tag + ".conv2", dict(N=N, H=Ho, W=Wo, cin=mid, cout=mid, k=3, pad=dil, dil=dil, relu=1, dt=dt)
        if fused:
            yield tag + ".conv3", dict(N=N, H=Ho, W=Wo, cin=mid, cin2=cin, cout=cout, relu=1, dt=dt)
        else:
            yield tag + ".conv3", dict(N=N, H=Ho, W=Wo, cin=mid, cout=cout, relu=1, res=True, mean=mean, dt=dt)
    yield "rpn.conv", dict(N=batch, H=H4, W=W4, cin=1024, cout=1024, k=3, pad=1, relu=1, dt=dt)
    yield "rpn.heads", dict(N=batch, H=H4, W=W4, cin=1024, cout=75, dt=dt, out_dt=L.VK_F32)


# fp16 production routing, layer by layer ("*": every block of the stage not listed on its own)
RESNET101_C4_ROUTES = {
    "res2.*.conv1": "generic", "res2.*.conv2": "blk", "res2.*.conv3": "ws",              # (res2.0.conv3: 64 + 64 channels, two inputs)
    "res3.0.shortcut": "ws", "res3.*.conv1": "generic", "res3.*.conv2": "generic", "res3.*.conv3": "ws",
    "res4.0.shortcut": "ws", "res4.0.conv1": "ws", "res4.*.conv1": "gemm4", "res4.*.conv2": "panel", "res4.*.conv3": "ws",
    "res5.*.conv1": "gemm4", "res5.*.conv2": "panel", "res5.0.conv3": "gemm4", "res5.*.conv3": "ws",   # (res5.2.conv3: the fused mean)
    "rpn.conv": "panel", "rpn.heads": "generic",
}


@pytest.mark.parametrize("dt", [L.VK_F16, L.VK_F32], ids=["fp16", "fp32"])
def test_conv_routes_resnet101_c4(lib, dt, monkeypatch):
    """Which kernel runs every convolution of the flagship model at the benchmark's size (32 x 800 x 1333, 300 RoIs per image),
    as a table: a change of production routing is a visible diff here.  fp32 strict mode runs the generic kernel throughout."""
    import gpu_util as G
    _clear_switches(monkeypatch)
    got = {}
    for layer, geom in _resnet101_c4_convs(lib, dt):
        got[layer] = G.conv_route(**geom)
    if dt == L.VK_F32:
        assert set(got.values()) == {"generic"}
        return
    want = {}
    for layer in got:
        want[layer] = RESNET101_C4_ROUTES.get(layer) or RESNET101_C4_ROUTES["{}.*.{}".format(*layer.split(".")[::2])]
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert len(got) == 3 * 33 + 2 + 2           # 33 blocks, a shortcut conv in res3.0 / res4.0 (res2.0's and res5.0's ride in conv3), the RPN's two


def test_gpu_tests_run_the_kernels_they_name(lib, monkeypatch):
    """Every launch of the GPU conv tests that names its kernel (`expect_route=` in tests/test_gpu_stages.py,
    test_gpu_bneck_fused.py, test_gpu_lxmert.py::test_linear, test_gpu_conv_exact.py, test_gpu_linear.py), asked of the dispatcher
    here, under that run's environment: no A/B test compares a kernel with itself, and each table covers every kernel its test is about."""
    import gpu_util as G
    import test_gpu_bneck_fused
    import test_gpu_conv_exact
    import test_gpu_linear
    import test_gpu_lxmert
    import test_gpu_stages
    seen, duo_builds = {}, set()
    for mod in (test_gpu_stages, test_gpu_bneck_fused, test_gpu_lxmert, test_gpu_conv_exact, test_gpu_linear):
        n = 0
        for label, env, geom, route in mod.route_plan():
            if mod is test_gpu_linear and route == "duo":
                duo_builds.add((geom["dt"], min(geom["relu"], 2) // 2 * 2))      # the GELU build, or the one of act <= 1
            _clear_switches(monkeypatch)
            for k, v in env.items():
                if v is not None:
                    monkeypatch.setenv(k, v)
            assert G.conv_route(**geom) == route, (label, env, geom)
            seen.setdefault(mod.__name__, set()).add(route)
            n += 1
        assert n > 0
    assert seen["test_gpu_stages"] == set(G.ROUTES) and seen["test_gpu_conv_exact"] == set(G.ROUTES)
    assert seen["test_gpu_lxmert"] == {"generic", "duo"}
    # the epilogue tests: both kernels vk_linear runs on, and both bf16 builds of the two-per-CU kernel (GELU; act <= 1) beside the f16 one
    assert seen["test_gpu_linear"] == {"generic", "duo"}
    assert duo_builds == {(L.VK_BF16, 2), (L.VK_BF16, 0), (L.VK_F16, 0)}


def test_conv_route_refuses_what_the_launch_refuses(lib):
    import gpu_util as G
    with pytest.raises(ValueError, match="multiple of"):
        G.conv_route(1, 8, 8, 48, 64)                       # Cin not a whole number of K-tiles
    with pytest.raises(ValueError, match="dual-source"):
        G.conv_route(1, 1, 4096, 64, 100, cin2=64)          # Cout % 256 != 0
    with pytest.raises(ValueError, match="fused-mean"):
        G.conv_route(4, 1, 64, 512, 512, mean=True, res=True)       # fewer than 128 rows per image
    assert lib.vk_conv_route(0, 8, 8, 64, 0, 0, 0, 64, 64, 1, 1, 1, 0, 1, 1, 0, L.VK_F16, L.VK_F16) == -L.VK_EINVAL
    for act in (4, -1):                                     # an activation no epilogue knows, on every route's geometry
        with pytest.raises(ValueError, match="activation"):
            G.conv_route(1, 1, 2600, 768, 768, relu=act, dt=L.VK_BF16)
        with pytest.raises(ValueError, match="activation"):
            G.conv_route(4, 14, 14, 128, 256, k=3, pad=1, relu=act)
    assert G.conv_route(1, 1, 2600, 768, 768, relu=3, dt=L.VK_BF16) == "generic"


def test_every_pinned_launch_states_its_route():
    """No test of the three GPU files that sets a kernel switch launches without `expect_route=` (the switch may be set through
    a `*_legs` / `*_env` table: then the test calls `_set_env`): such a test states a route, and none of its launches of the four
    entry points is a bare `L.call`."""
    pat = re.compile(r"VK_(CONV|WS|GEMM4|PANEL)\w*|_set_env\(")
    for name in ("test_gpu_stages.py", "test_gpu_bneck_fused.py", "test_gpu_lxmert.py"):
        src = open(os.path.join(ROOT, "tests", name)).read()
        for body in re.split(r"\n(?=def |@pytest)", src):
            m = re.match(r"def (test_\w+)", body)
            if m and pat.search(body) and ("setenv(" in body or "_set_env(" in body):
                assert "expect_route=" in body, f"{name}::{m.group(1)} sets a kernel switch and launches without expect_route"
                bare = re.search(r'L\.call\("(vk_conv2d|vk_conv1x1_dual|vk_conv1x1_meanpool|vk_linear)"', body)
                assert not bare, f"{name}::{m.group(1)} launches {bare.group(1)} under a kernel switch without stating its route"
