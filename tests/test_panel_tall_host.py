"""CPU: which tile the phase part of a 3x3 panel launch takes (vk_panel_phase_tile_rows, the function the launcher itself
reads): 512 rows x 128 columns, 256 x 256 under VK_PANEL_TALL=0, 0 where no image takes the phase form."""
import pytest

from vltk_amd import _lib as L


@pytest.fixture()
def lib(monkeypatch):
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    monkeypatch.delenv("VK_PANEL_TALL", raising=False)
    return L.load()


@pytest.mark.parametrize("N,H,W,cout", [(16, 14, 14, 256), (32, 14, 14, 512), (16, 6, 10, 256), (16, 2, 2, 256), (9600, 14, 14, 512)])
def test_eligible_is_tall_or_wide_under_the_switch(lib, monkeypatch, N, H, W, cout):
    assert lib.vk_panel_phase_tile_rows(N, H, W, 2, cout) == 512
    monkeypatch.setenv("VK_PANEL_TALL", "0")          # re-read per call
    assert lib.vk_panel_phase_tile_rows(N, H, W, 2, cout) == 256
    monkeypatch.setenv("VK_PANEL_TALL", "1")
    assert lib.vk_panel_phase_tile_rows(N, H, W, 2, cout) == 512
    monkeypatch.setenv("VK_PANEL_PHASE", "0")         # no phase form, no phase tile
    assert lib.vk_panel_phase_tile_rows(N, H, W, 2, cout) == 0


@pytest.mark.parametrize("N,H,W,dil", [(32, 14, 14, 1),       # dilation 1 has no phases
                                       (32, 14, 13, 2),       # odd W
                                       (32, 14, 16, 2),       # halo (W / 2 + 1) * 16 > 128 rows
                                       (8, 14, 14, 2)])       # fewer than one group of 16 images
@pytest.mark.parametrize("tall", [None, "0"])
def test_ineligible_is_zero(lib, monkeypatch, N, H, W, dil, tall):
    if tall is not None:
        monkeypatch.setenv("VK_PANEL_TALL", tall)
    assert lib.vk_panel_phase_images(N, H, W, dil) == 0
    assert lib.vk_panel_phase_tile_rows(N, H, W, dil, 512) == 0


def test_remainder_answers_for_the_phase_part(lib, monkeypatch):
    assert lib.vk_panel_phase_images(20, 14, 14, 2) == 16      # 16 images in the phase form, 4 in a plain launch
    assert lib.vk_panel_phase_tile_rows(20, 14, 14, 2, 256) == 512
    monkeypatch.setenv("VK_PANEL_TALL", "0")
    assert lib.vk_panel_phase_tile_rows(20, 14, 14, 2, 256) == 256
