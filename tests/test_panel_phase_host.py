"""CPU: which images of a 3x3 panel launch take the kernel's phase-interleaved form (vk_panel_phase_images, the function the
launcher itself splits on), and that the form never changes the route."""
import pytest

import gpu_util as G
from vltk_amd import _lib as L


@pytest.fixture()
def lib(monkeypatch):
    monkeypatch.delenv("VK_PANEL_PHASE", raising=False)
    return L.load()


@pytest.mark.parametrize("N,want", [(1, 0), (8, 0), (15, 0), (16, 16), (17, 16), (20, 16), (31, 16), (32, 32), (300, 288), (9600, 9600)])
def test_whole_groups_of_16_lead(lib, N, want):
    assert lib.vk_panel_phase_images(N, 14, 14, 2) == want


@pytest.mark.parametrize("H,W,dil,ok", [(14, 14, 2, True), (6, 10, 2, True), (2, 2, 2, True), (1024, 14, 2, True),
                                        (14, 14, 1, False), (14, 14, 3, False),      # a dilation other than 2 has no phases
                                        (13, 14, 2, False), (14, 13, 2, False),      # odd sides
                                        (14, 16, 2, False), (50, 84, 2, False),      # halo (W / 2 + 1) * 16 > 128 rows
                                        (1026, 14, 2, False)])                       # beyond the exact range of the W / 2 reciprocal
def test_eligible_geometry(lib, H, W, dil, ok):
    assert lib.vk_panel_phase_images(32, H, W, dil) == (32 if ok else 0)


def test_switch_is_read_per_call(lib, monkeypatch):
    assert lib.vk_panel_phase_images(32, 14, 14, 2) == 32
    monkeypatch.setenv("VK_PANEL_PHASE", "0")
    assert lib.vk_panel_phase_images(32, 14, 14, 2) == 0
    monkeypatch.setenv("VK_PANEL_PHASE", "1")
    assert lib.vk_panel_phase_images(32, 14, 14, 2) == 32


@pytest.mark.parametrize("phase", ["0", "1"])
def test_route_stays_panel(lib, monkeypatch, phase):
    monkeypatch.setenv("VK_PANEL_PHASE", phase)
    for N in (8, 16, 20, 9600):
        assert G.conv_route(N, 14, 14, 512, 512, k=3, pad=2, dil=2, relu=1) == "panel"
