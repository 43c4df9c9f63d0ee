"""The indexed form of the 3x3 panel kernel (csrc/conv3x3_panel.hip, IDX) on the host: what
vk_panel_phase_indexed answers, under each switch, and what vk_conv2d_rows refuses before it touches a device.  The GPU
side is tests/test_gpu_panel_indexed.py.

The query and the launcher read the same function (conv3x3_panel_phase_indexed), so a launch given an index runs the one
instantiation that reads it or is refused: it never runs another form on the wrong rows."""
import ctypes as C

import pytest

from vltk_amd import _lib as L

SWITCHES = ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_CONV3X3_PANEL")


@pytest.fixture
def lib(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return L.load()


def test_query(lib, monkeypatch):
    q = lib.vk_panel_phase_indexed
    for N in (16, 32, 64, 9600):
        assert q(N, 14, 14, 2, 512) == 1 and q(N, 14, 14, 2, 256) == 1
    assert q(16, 2, 2, 2, 256) == 1 and q(16, 10, 6, 2, 256) == 1
    assert q(20, 14, 14, 2, 512) == 0          # 16 images in the phase form, 4 in a second, plain launch
    assert q(8, 14, 14, 2, 512) == 0
    assert q(16, 14, 14, 1, 512) == 0          # dilation 1: no phase form
    assert q(16, 14, 16, 2, 512) == 0          # W = 16: halo beyond 128 rows
    assert q(16, 13, 14, 2, 512) == 0          # odd H
    assert q(16, 14, 14, 2, 384) == 0          # not a panel launch
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED"):
        monkeypatch.setenv(k, "0")             # (re-read per call)
        assert q(16, 14, 14, 2, 512) == 0, k
        monkeypatch.setenv(k, "1")
        assert q(16, 14, 14, 2, 512) == 1, k
        monkeypatch.delenv(k)
    assert q(16, 14, 14, 2, 512) == 1
    # the other queries do not read the new switch
    monkeypatch.setenv("VK_PANEL_INDEXED", "0")
    assert lib.vk_panel_phase_images(16, 14, 14, 2) == 16 and lib.vk_panel_phase_reuse(16, 14, 14, 2, 512) == 1


def _rows_launch(lib, N, H, W, cin, cout, dil=2, x_rows=7, idx=True):
    """vk_conv2d_rows on host memory: only ever called where the launch is refused before any device call."""
    buf = (C.c_char * 256)()
    p = C.c_void_p(C.addressof(buf))
    return lib.vk_conv2d_rows(p, x_rows, p if idx else None, N, H, W, cin, p, p, None, p, cout, dil, 1, None)


def test_launch_with_an_index_is_refused_off_the_form(lib, monkeypatch):
    for geom in ((20, 14, 14, 128, 256),           # a remainder of four images would run the plain form
                 (8, 14, 14, 128, 256),            # no phase part at all
                 (16, 14, 16, 128, 256),           # W = 16
                 (16, 13, 14, 128, 256)):          # odd H
        assert _rows_launch(lib, *geom) == L.VK_EINVAL, geom
        assert b"x_idx" in lib.vk_last_error(), geom
    assert _rows_launch(lib, 16, 14, 14, 128, 256, dil=1) == L.VK_EINVAL and b"x_idx" in lib.vk_last_error()
    assert _rows_launch(lib, 16, 14, 14, 64, 256) == L.VK_EINVAL and b"x_idx" in lib.vk_last_error()       # not a panel launch: Cin < 128
    assert _rows_launch(lib, 16, 14, 14, 128, 256, x_rows=1 << 24) == L.VK_EINVAL                          # 2^24 rows x 256 B: beyond 32-bit offsets
    assert b"x_idx" in lib.vk_last_error()
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE", "VK_PANEL_INDEXED", "VK_CONV3X3_PANEL"):
        monkeypatch.setenv(k, "0")
        assert _rows_launch(lib, 16, 14, 14, 128, 256) == L.VK_EINVAL, k
        assert b"x_idx" in lib.vk_last_error(), k
        monkeypatch.delenv(k)
    assert _rows_launch(lib, 16, 14, 14, 128, 256, idx=False) == L.VK_EINVAL and b"conv2d_rows" in lib.vk_last_error()
    assert _rows_launch(lib, 16, 14, 14, 128, 256, x_rows=0) == L.VK_EINVAL and b"conv2d_rows" in lib.vk_last_error()
