"""CPU: which A-fragment schedule the phase part of a 3x3 panel launch takes (vk_panel_phase_reuse, the function the launcher
itself reads): the shared window on 512-row tiles, the read-per-tap schedule under VK_PANEL_REUSE=0, 0 where the launch has
no 512-row phase tile."""
import pytest

from vltk_amd import _lib as L


@pytest.fixture()
def lib(monkeypatch):
    for k in ("VK_PANEL_PHASE", "VK_PANEL_TALL", "VK_PANEL_REUSE"):
        monkeypatch.delenv(k, raising=False)
    return L.load()


@pytest.mark.parametrize("N,H,W,cout", [(16, 14, 14, 256), (32, 14, 14, 512), (16, 6, 10, 256), (16, 4, 4, 256), (16, 2, 2, 256),
                                        (20, 14, 14, 256), (9600, 14, 14, 512)])
def test_window_is_the_default_of_the_tall_tile(lib, monkeypatch, N, H, W, cout):
    assert lib.vk_panel_phase_reuse(N, H, W, 2, cout) == 1
    for k in ("VK_PANEL_REUSE", "VK_PANEL_TALL", "VK_PANEL_PHASE"):      # each re-read per call
        monkeypatch.setenv(k, "0")
        assert lib.vk_panel_phase_reuse(N, H, W, 2, cout) == 0, k
        monkeypatch.setenv(k, "1")
        assert lib.vk_panel_phase_reuse(N, H, W, 2, cout) == 1, k
        monkeypatch.delenv(k)
    monkeypatch.setenv("VK_PANEL_REUSE", "0")                            # the switch leaves the tile alone
    assert lib.vk_panel_phase_tile_rows(N, H, W, 2, cout) == 512


@pytest.mark.parametrize("N,H,W,dil", [(32, 14, 14, 1), (32, 14, 13, 2), (32, 14, 16, 2), (8, 14, 14, 2)])
def test_no_phase_tile_no_window(lib, N, H, W, dil):
    assert lib.vk_panel_phase_tile_rows(N, H, W, dil, 512) == 0
    assert lib.vk_panel_phase_reuse(N, H, W, dil, 512) == 0
