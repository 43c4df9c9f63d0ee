"""CPU: the routing rule of the attention entry points (vk_attention_route, host only): which of the four kernels
vk_attention / vk_attention_tiled launch for a shape, under the A/B switches, and what they refuse before any device call."""
import ctypes as C
import os
import re

import pytest

from vltk_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfma", "lds", "tiled", "stream")          # VK_ATT_ROUTE_* by value
NEW = ("vk_attention_tiled", "vk_attention_route")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("VK_ATTENTION_MFMA", raising=False)
    monkeypatch.delenv("VK_ATTENTION_TILED", raising=False)


def route(lib, Lq, Lk, d, dt, tiled_entry, ld=None, aligned=1):
    ldq, ldk, ldv = ld if ld is not None else (d, d, d)
    r = lib.vk_attention_route(Lq, Lk, d, dt, ldq, ldk, ldv, aligned, tiled_entry)
    if r < 0:
        L.check(-r)
    return NAMES[r]


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared"
        assert name in L.SIGNATURES and hasattr(lib, name)
    values = {n: int(re.search(r"#define\s+VK_ATT_ROUTE_%s\s+(\d+)" % n.upper(), header).group(1)) for n in NAMES}
    assert values == {n: i for i, n in enumerate(NAMES)}
    assert (L.VK_ATT_ROUTE_MFMA, L.VK_ATT_ROUTE_LDS, L.VK_ATT_ROUTE_TILED, L.VK_ATT_ROUTE_STREAM) == (0, 1, 2, 3)
    assert L.SIGNATURES["vk_attention_tiled"] == L.SIGNATURES["vk_attention"]
    assert lib.vk_version() == 1


def test_todays_shapes_keep_their_kernels(lib):
    """Every row of test_gpu_lxmert.py::test_attention runs where it ran: the matrix-core kernel for 16-bit d 32 / 64 within 48
    queries and 64 keys, the LDS kernel otherwise; vk_attention_tiled with VK_ATTENTION_TILED=0 follows the same rule."""
    import test_gpu_lxmert
    marks = [m for m in test_gpu_lxmert.test_attention.pytestmark if m.name == "parametrize" and m.args[0].startswith("B,")]
    rows = marks[0].args[1]
    assert len(rows) == 8
    for B, heads, Lq, Lk, d, masked in rows:
        H = heads * d
        for dt in (L.VK_F32, L.VK_F16, L.VK_BF16):
            want = "mfma" if dt != L.VK_F32 and d in (32, 64) and Lq <= 48 and Lk <= 64 else "lds"
            assert route(lib, Lq, Lk, d, dt, 0, ld=(H, 2 * H, 2 * H)) == want, (Lq, Lk, d, dt)
    os.environ["VK_ATTENTION_TILED"] = "0"
    try:
        for B, heads, Lq, Lk, d, masked in rows:
            for dt in (L.VK_F32, L.VK_BF16):
                assert route(lib, Lq, Lk, d, dt, 1) == route(lib, Lq, Lk, d, dt, 0)
    finally:
        del os.environ["VK_ATTENTION_TILED"]


@pytest.mark.parametrize("dt", [L.VK_F16, L.VK_BF16])
@pytest.mark.parametrize("Lq,Lk", [(49, 20), (100, 100), (20, 100)])
def test_sixteen_bit_past_the_small_kernel(lib, dt, Lq, Lk):
    assert route(lib, Lq, Lk, 64, dt, 0) == "lds"
    assert route(lib, Lq, Lk, 64, dt, 1) == "tiled"
    assert route(lib, Lq, Lk, 32, dt, 1) == "tiled"


def test_past_the_lds_kernel(lib):
    for dt in (L.VK_F16, L.VK_BF16):
        assert route(lib, 128, 128, 64, dt, 0) == "tiled"
        assert route(lib, 128, 128, 64, dt, 1) == "tiled"
    assert route(lib, 128, 128, 64, L.VK_F32, 0) == "stream"
    assert route(lib, 128, 128, 64, L.VK_F32, 1) == "stream"
    assert route(lib, 127, 127, 64, L.VK_F32, 0) == "lds"        # the last self-attention one head's LDS image holds
    assert route(lib, 127, 127, 64, L.VK_F32, 1) == "stream"
    assert route(lib, 1024, 1024, 64, L.VK_BF16, 0) == "tiled"


def test_what_the_matrix_cores_refuse_streams(lib):
    assert route(lib, 200, 200, 48, L.VK_BF16, 0) == "stream"                    # head dim
    assert route(lib, 20, 36, 48, L.VK_BF16, 1) == "stream"
    assert route(lib, 20, 36, 48, L.VK_BF16, 0) == "lds"
    assert route(lib, 200, 200, 64, L.VK_BF16, 0, ld=(132, 128, 128)) == "stream"      # ldq % 8 != 0
    assert route(lib, 200, 200, 64, L.VK_BF16, 1, ld=(132, 128, 128)) == "stream"
    assert route(lib, 200, 200, 64, L.VK_BF16, 1, ld=(128, 128, 130)) == "stream"
    assert route(lib, 200, 200, 64, L.VK_F16, 1, aligned=0) == "stream"          # a pointer off the 16-byte grid
    assert route(lib, 200, 200, 256, L.VK_F32, 1) == "stream"


def test_environment_switches_are_read_per_call(lib, monkeypatch):
    assert route(lib, 20, 36, 64, L.VK_BF16, 0) == "mfma"
    assert route(lib, 100, 100, 64, L.VK_BF16, 1) == "tiled"
    monkeypatch.setenv("VK_ATTENTION_TILED", "0")
    assert route(lib, 100, 100, 64, L.VK_BF16, 1) == "lds"        # vk_attention_tiled behaves as vk_attention
    assert route(lib, 20, 36, 64, L.VK_BF16, 1) == "mfma"
    assert route(lib, 200, 200, 64, L.VK_BF16, 1) == "tiled"      # ... which itself tiles past the LDS kernel
    monkeypatch.setenv("VK_ATTENTION_TILED", "1")
    assert route(lib, 100, 100, 64, L.VK_BF16, 1) == "tiled"
    monkeypatch.delenv("VK_ATTENTION_TILED")
    monkeypatch.setenv("VK_ATTENTION_MFMA", "0")                  # no matrix cores in either entry
    assert route(lib, 20, 36, 64, L.VK_BF16, 0) == "lds"
    assert route(lib, 100, 100, 64, L.VK_BF16, 1) == "stream"
    assert route(lib, 200, 200, 64, L.VK_BF16, 0) == "stream"
    monkeypatch.delenv("VK_ATTENTION_MFMA")
    assert route(lib, 20, 36, 64, L.VK_BF16, 0) == "mfma"


def test_routes_the_every_build_and_head_dim_tests_expect(lib, monkeypatch):
    """The kernel of every (shape, dtype, entry) that test_gpu_attention_builds.py, the long rows of test_gpu_attention_small.py's
    surroundings test and the forward / backward pair of test_gpu_attention_grad.py launch, on the strides those tests use (column
    slices of [rows, 2 H] buffers; the trainer's packed [rows, 3 H]): a change of the rule cannot quietly move one of them to
    another kernel.  The shapes are read from the GPU file, the routes are written out here."""
    import test_gpu_attention_builds as TB
    sixteen = (L.VK_F16, L.VK_BF16)

    def on(entry, dt, Lq, Lk, d, B_heads, width=2):
        ld = width * B_heads[1] * d
        return route(lib, Lq, Lk, d, dt, int(entry == "vk_attention_tiled"), ld=(ld, ld, ld))

    # 1. every build: (3, 3) everywhere, (1, 1) and (2, 2) at two pairs
    assert len(TB.BUILD_PAIRS) == 10 and TB.HEAD_DIMS == [32, 64]
    for Lq, Lk in TB.BUILD_PAIRS:
        for d in TB.HEAD_DIMS:
            for bh in [(3, 3)] + ([(1, 1), (2, 2)] if (Lq, Lk) in TB.OTHER_BH else []):
                for dt in sixteen:
                    assert on("vk_attention_tiled", dt, Lq, Lk, d, bh) == "tiled", (Lq, Lk, d, bh)
                assert on("vk_attention_tiled", L.VK_F32, Lq, Lk, d, bh) == "stream", (Lq, Lk, d, bh)
    # 2. the permutation across three key tiles (contiguous rows), 3. the surroundings at (36, 70) and (17, 70)
    for Lq, Lk, width in ((50, 150, 1), (13, 150, 1), (36, 70, 2), (17, 70, 2)):
        for d in (32, 64) if width == 1 else (64,):
            for dt in sixteen:
                assert on("vk_attention_tiled", dt, Lq, Lk, d, (3, 3), width) == "tiled"
            assert on("vk_attention_tiled", L.VK_F32, Lq, Lk, d, (3, 3), width) == "stream"
    # 4. head dims: what the matrix cores do not take streams at the tiled entry whatever the switch says
    assert len(TB.STREAM_DIMS) == 15
    for dt, d in TB.STREAM_DIMS:
        for Lq, Lk in ((17, 65), (33, 129)):
            assert on("vk_attention_tiled", dt, Lq, Lk, d, (3, 2)) == "stream", (dt, d)
    for dt in (L.VK_F32,) + sixteen:
        for d in (128, 256):
            assert on("vk_attention_tiled", dt, 50, 150, d, (2, 3), 1) == "stream"
            assert on("vk_attention", dt, 20, 36, d, (3, 3)) == "lds"
        assert on("vk_attention", dt, 31, 128, 128, (2, 3), 1) == "lds"          # 163 576 bytes: the largest image, as (127, 127, 64)
        assert on("vk_attention", dt, 32, 128, 128, (2, 3), 1) == "stream"
    assert on("vk_attention", L.VK_F32, 127, 127, 64, (3, 3)) == "lds"
    assert on("vk_attention", L.VK_F32, 128, 128, 64, (3, 3)) == "stream"
    # 5. the forward of the pair, on the trainer's packed projection
    assert on("vk_attention", L.VK_F32, 35, 35, 16, (3, 2), 3) == "lds"
    assert on("vk_attention_tiled", L.VK_F32, 35, 35, 16, (3, 2), 3) == "stream"
    assert on("vk_attention", L.VK_F32, 140, 140, 64, (3, 2), 3) == "stream"
    assert route(lib, 140, 140, 64, L.VK_F32, 0, ld=(384, 384, 384)) == "stream"          # the trainer's fixture at Lx = 140
    # the 16-bit types reach the LDS and streaming kernels of these tests with the matrix cores switched off
    monkeypatch.setenv("VK_ATTENTION_MFMA", "0")
    for dt in sixteen:
        for Lq, Lk in TB.BUILD_PAIRS + [(50, 150), (36, 70), (17, 70)]:
            for d in TB.HEAD_DIMS:
                assert on("vk_attention_tiled", dt, Lq, Lk, d, (3, 3)) == "stream"


def test_refusals_come_before_any_device_call(lib):
    """Head dims past 256 are refused by name of the limit, through the launch entry points themselves with made-up pointers:
    the refusal is decided on the host."""
    fake = C.c_void_p(4096)
    for name in ("vk_attention", "vk_attention_tiled"):
        for dt in (L.VK_F32, L.VK_BF16):
            with pytest.raises(ValueError, match="256"):
                L.call(name, fake, 257, fake, 257, fake, 257, None, fake, 257, 1, 1, 128, 128, 257, dt, None)
    with pytest.raises(ValueError, match="256"):
        route(lib, 128, 128, 257, L.VK_F32, 0)
    with pytest.raises(ValueError, match="256"):
        route(lib, 8, 8, 257, L.VK_F32, 1)
    assert lib.vk_attention_route(0, 8, 64, L.VK_F32, 64, 64, 64, 1, 0) == -L.VK_EINVAL
    assert lib.vk_attention_route(8, 8, 64, L.VK_I32, 64, 64, 64, 1, 1) == -L.VK_EINVAL
    with pytest.raises(ValueError, match="null"):
        L.call("vk_attention_tiled", None, 64, fake, 64, fake, 64, None, fake, 64, 1, 1, 8, 8, 64, L.VK_F32, None)


def test_the_encoders_rule_for_picking_an_entry_point(lib, monkeypatch):
    """BertOps.attention_entry, the one statement of what a forward calls: 16-bit goes to vk_attention where the small
    matrix-core kernel reaches and to vk_attention_tiled everywhere else, fp32 always to vk_attention.  The table is written
    out, not computed; d = 64, 12 heads, ld = 3 * 768, aligned pointers unless a row says otherwise."""
    from vltk_amd.bert_ops import BertOps

    def entry(dt, Lq, Lk, d=64, aligned=1):
        ops = object.__new__(BertOps)
        ops.cfg, ops.dt = dict(hidden_size=12 * d, num_attention_heads=12), dt
        name, r = ops.attention_entry(Lq, Lk, 3 * 768, 3 * 768, 3 * 768, aligned)
        return name, NAMES[r]

    for dt in (L.VK_BF16, L.VK_F16):
        for Lq, Lk in ((20, 20), (36, 36), (20, 36), (36, 20), (47, 47), (48, 64)):
            assert entry(dt, Lq, Lk) == ("vk_attention", "mfma"), (dt, Lq, Lk)
        for Lq, Lk in ((49, 49), (48, 65), (56, 56), (197, 197), (577, 577)):
            assert entry(dt, Lq, Lk) == ("vk_attention_tiled", "tiled"), (dt, Lq, Lk)
    assert entry(L.VK_BF16, 100, 100, d=48) == ("vk_attention_tiled", "stream")
    assert entry(L.VK_BF16, 20, 36, aligned=0) == ("vk_attention_tiled", "stream")
    for Lq, Lk in ((20, 36), (100, 100), (127, 127)):
        assert entry(L.VK_F32, Lq, Lk) == ("vk_attention", "lds"), (Lq, Lk)
    for Lq, Lk in ((128, 128), (197, 197)):
        assert entry(L.VK_F32, Lq, Lk) == ("vk_attention", "stream"), (Lq, Lk)
    monkeypatch.setenv("VK_ATTENTION_MFMA", "0")
    assert entry(L.VK_BF16, 20, 36) == ("vk_attention_tiled", "stream")
