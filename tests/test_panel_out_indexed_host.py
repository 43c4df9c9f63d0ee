"""The indexed store of the 3x3 panel kernel (csrc/conv3x3_panel.hip, OIDX) on the host: what
vk_panel_out_indexed answers, under each switch, and what vk_conv2d_rows_out refuses before it touches a device.  The GPU side
is tests/test_gpu_panel_out_indexed.py.

The query and the launcher read the same function (conv3x3_panel_out_indexed), so a launch given an output index runs an
instantiation that stores through it or is refused: it never stores every row where the dense form would."""
import ctypes as C

import pytest

from vltk_amd import _lib as L

SWITCHES = ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_PANEL_OUT_INDEXED", "VK_CONV3X3_PANEL")


@pytest.fixture
def lib(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return L.load()


def test_query(lib, monkeypatch):
    q = lib.vk_panel_out_indexed
    for N in (16, 32, 64, 9600):
        assert q(N, 14, 14, 2, 512) == 1 and q(N, 14, 14, 2, 256) == 1
    assert q(16, 2, 2, 2, 256) == 1 and q(16, 10, 6, 2, 256) == 1
    assert q(20, 14, 14, 2, 512) == 0          # N % 16 != 0: four images would run the plain form
    assert q(8, 14, 14, 2, 512) == 0
    assert q(16, 14, 14, 1, 512) == 0          # dilation 1: no phase form
    assert q(16, 14, 16, 2, 512) == 0          # W = 16: halo beyond 128 rows
    assert q(16, 13, 14, 2, 512) == 0          # odd H
    assert q(16, 14, 14, 2, 384) == 0          # not a panel launch
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_OUT_INDEXED"):
        monkeypatch.setenv(k, "0")             # (re-read per call)
        assert q(16, 14, 14, 2, 512) == 0, k
        monkeypatch.setenv(k, "1")
        assert q(16, 14, 14, 2, 512) == 1, k
        monkeypatch.delenv(k)
    assert q(16, 14, 14, 2, 512) == 1
    # the two indices are independent: each query reads its own switch and not the other's
    monkeypatch.setenv("VK_PANEL_INDEXED", "0")
    assert q(16, 14, 14, 2, 512) == 1 and lib.vk_panel_phase_indexed(16, 14, 14, 2, 512) == 0
    monkeypatch.delenv("VK_PANEL_INDEXED")
    monkeypatch.setenv("VK_PANEL_OUT_INDEXED", "0")
    assert q(16, 14, 14, 2, 512) == 0 and lib.vk_panel_phase_indexed(16, 14, 14, 2, 512) == 1
    assert lib.vk_panel_phase_images(16, 14, 14, 2) == 16 and lib.vk_panel_phase_reuse(16, 14, 14, 2, 512) == 1


def _launch(lib, N, H, W, cin, cout, dil=2, x_idx=False, y_idx=True, y_rows=7, res=False):
    """vk_conv2d_rows_out on host memory: only ever called where the launch is refused before any device call."""
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))
    return lib.vk_conv2d_rows_out(p, 7, p if x_idx else None, N, H, W, cin, p, p, p if res else None, p, y_rows, p if y_idx else None,
                                  cout, dil, 1, None)


@pytest.mark.parametrize("x_idx", [False, True], ids=["dense_in", "indexed_in"])
def test_launch_with_an_output_index_is_refused_off_the_form(lib, monkeypatch, x_idx):
    # (with an input index as well the launch is refused all the same; which of the two indices the text names is not fixed there)
    names = (b"y_idx", b"x_idx") if x_idx else (b"y_idx",)

    def refused(*a, **kw):
        assert _launch(lib, *a, x_idx=x_idx, **kw) == L.VK_EINVAL, (a, kw)
        assert any(n in lib.vk_last_error() for n in names), (a, kw, lib.vk_last_error())

    for geom in ((20, 14, 14, 128, 256),           # N % 16 != 0
                 (8, 14, 14, 128, 256),            # no phase part at all
                 (16, 14, 16, 128, 256),           # W = 16
                 (16, 13, 14, 128, 256)):          # odd H
        refused(*geom)
    refused(16, 14, 14, 128, 256, dil=1)
    refused(16, 14, 14, 64, 256)                   # not a panel launch: Cin < 128
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_OUT_INDEXED", "VK_CONV3X3_PANEL"):
        monkeypatch.setenv(k, "0")
        refused(16, 14, 14, 128, 256)
        monkeypatch.delenv(k)


def test_refusals_name_their_reason(lib, monkeypatch):
    assert _launch(lib, 20, 14, 14, 128, 256) == L.VK_EINVAL
    assert b"y_idx needs the whole launch" in lib.vk_last_error() and b"N=20" in lib.vk_last_error()
    monkeypatch.setenv("VK_PANEL_OUT_INDEXED", "0")
    assert _launch(lib, 16, 14, 14, 128, 256) == L.VK_EINVAL and b"OUT_INDEXED" in lib.vk_last_error()
    monkeypatch.delenv("VK_PANEL_OUT_INDEXED")
    assert _launch(lib, 16, 14, 14, 128, 256, res=True) == L.VK_EINVAL
    assert b"y_idx takes no residual" in lib.vk_last_error()
    for rows in (0, -3):
        assert _launch(lib, 16, 14, 14, 128, 256, y_rows=rows) == L.VK_EINVAL
        assert b"y_idx needs y_rows > 0" in lib.vk_last_error()
    assert _launch(lib, 16, 14, 14, 128, 256, y_idx=False) == L.VK_EINVAL and b"conv2d_rows_out" in lib.vk_last_error()
    # the input index's own refusal still stands beside an output index
    monkeypatch.setenv("VK_PANEL_INDEXED", "0")
    assert _launch(lib, 16, 14, 14, 128, 256, x_idx=True) == L.VK_EINVAL and b"x_idx" in lib.vk_last_error()
