"""-m gpu: every kernel of csrc/fpn.hip on its own, per element or bit for bit.

vk_roi_align: each of its three forms launched with the form asserted (vk_roi_align_form), in f32, f16 and bf16 -- the exact
sets of fpn_exact_util bit for bit against roi_align_fp64 rounded once to the storage type, the four-level pyramid bit for
bit with the rule's levels and with permuted ones, and the cases that are not exact (sampling ratio 3, P = 20, boxes outside /
empty / larger than the map / inverted / below one cell) per element under the bound derived in fpn_exact_util.
tests/test_fpn_exact_host.py proves on the CPU what these rely on.  The vector forms only ever see 16-byte-aligned tensors.
vk_upsample2x_add, vk_subsample2, vk_relu_copy: bit-equal to their one-line definitions in three dtypes, special values
included, with a sentinel behind every output."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L                          # noqa: E402

import fpn_exact_util as X                              # noqa: E402
import gpu_util as G                                    # noqa: E402
import roi_align_c4_util as U                           # noqa: E402

DTS = (X.F32, X.F16, X.BF16)
IDT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("VK_ROIALIGN_TABLES", raising=False)


def nhwc(x_nchw, td):
    return torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).to(td).to(G.DEV)


def expect_bits(ref64, td):
    """[K, C, P, P] float64 -> [K, P, P, C] in the storage type: one rounding (every exact value is an fp32 number)."""
    return torch.from_numpy(np.ascontiguousarray(ref64.transpose(0, 2, 3, 1))).to(torch.float32).to(td)


def differing_rois(got, expect):
    return (got.view(IDT[got.dtype]) != expect.view(IDT[expect.dtype])).flatten(1).any(1).nonzero().flatten().tolist()


_MAPS = {}


def exact_device_map(C_, dt):
    if (C_, dt) not in _MAPS:
        _MAPS[(C_, dt)] = nhwc(X.exact_map_wide()[:, :C_], X.TD[dt])
    return _MAPS[(C_, dt)]


def run_exact(dt, C_, P, sr, aligned, scale, expect_form):
    rois, ref = X.exact_reference(P, sr, aligned, scale, C_)
    got = X.run_roi_align([exact_device_map(C_, dt)], [scale], torch.from_numpy(rois).to(G.DEV), None, P, sr, aligned, dt, expect_form)
    bad = differing_rois(got, expect_bits(ref, X.TD[dt]))
    assert not bad, f"{expect_form} {X.NAME[dt]} C={C_} P={P} sr={sr} aligned={aligned} scale=1/{round(1 / scale)}: RoIs {bad} differ"
    return got


def ids(cases):
    return [f"{X.NAME[dt]}-C{c}" for dt, c in cases]


# ---- vk_roi_align, exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C_", X.SCALAR_CASES, ids=ids(X.SCALAR_CASES))
def test_roi_align_scalar_form_exact(dt, C_):
    """64-thread blocks part filled (C = 6, 12) and in two passes (70); 256-thread blocks in two passes (260, 1028)."""
    for sr, aligned, scale in X.SCALAR_GEOMS + (X.SCALAR_SCALE_GEOMS if (dt, C_) == (X.F32, 6) else ()):
        run_exact(dt, C_, 7, sr, aligned, scale, "scalar")


@pytest.mark.parametrize("P", [7, 14])
@pytest.mark.parametrize("dt,C_", X.SEP_CASES, ids=ids(X.SEP_CASES))
def test_roi_align_sep_form_exact(dt, C_, P):
    """One lane per bin (C = 8), 10 lanes and trimmed groups (f32 C = 40), the FPN head's 32 lanes, 256 lanes in one group."""
    for sr, aligned, scale in X.SEP_GEOMS:
        run_exact(dt, C_, P, sr, aligned, scale, "sep")


@pytest.mark.parametrize("P", sorted(X.SEP_MORE_GEOMS))
@pytest.mark.parametrize("dt,C_", [(X.F16, 256), (X.F32, 40), (X.BF16, 8)], ids=["f16-C256", "f32-C40", "bf16-C8"])
def test_roi_align_sep_form_exact_more_geometries(dt, C_, P):
    """Sampling ratios 1 and 4, `aligned` off, P = 16, and P = 7 at the pyramid's other scales."""
    for sr, aligned, scale in X.SEP_MORE_GEOMS[P]:
        run_exact(dt, C_, P, sr, aligned, scale, "sep")


@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_roi_align_vec_form_exact_p32(dt):
    for sr, aligned, scale in X.VEC_P32_GEOMS:
        run_exact(dt, 256, 32, sr, aligned, scale, "vec")


@pytest.mark.parametrize("P", [7, 14])
@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_roi_align_vec_form_under_the_switch_gives_the_sep_bytes(dt, P, monkeypatch):
    """VK_ROIALIGN_TABLES=0 (read per call) sends P <= 16 to the vec kernel: the exact bits, and the sep kernel's bytes."""
    for sr, aligned, scale in X.VEC_ENV_GEOMS:
        monkeypatch.delenv("VK_ROIALIGN_TABLES", raising=False)
        sep = run_exact(dt, 256, P, sr, aligned, scale, "sep")
        monkeypatch.setenv("VK_ROIALIGN_TABLES", "0")
        vec = run_exact(dt, 256, P, sr, aligned, scale, "vec")
        assert torch.equal(sep.view(IDT[sep.dtype]), vec.view(IDT[vec.dtype]))


# ---- the pyramid, exact ---------------------------------------------------------------------------------------------------------
_PYR = {}


def pyramid_device(C_, dt):
    if (C_, dt) not in _PYR:
        _PYR[(C_, dt)] = [nhwc(m, X.TD[dt]) for m in X.pyramid_maps(C_)]
    return _PYR[(C_, dt)]


def rule_levels(rois):
    boxes = torch.from_numpy(np.ascontiguousarray(rois[:, 1:])).to(G.DEV)
    out = torch.empty(len(rois), dtype=torch.int32, device=G.DEV)
    L.call("vk_assign_levels", G.P(boxes), 4, len(rois), 2, 5, 224.0, 4, G.P(out), G.stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("which,sr", [("rule", X.PYR_SR), ("permuted", X.PYR_SR), ("rule", 0)])
@pytest.mark.parametrize("dt,C_", [(X.F16, 256), (X.BF16, 256), (X.F32, 64)], ids=["f16-C256", "bf16-C256", "f32-C64"])
def test_roi_align_pyramid_exact(dt, C_, which, sr):
    """Four maps of different data, sizes and scales: a RoI read from the wrong level's map, H, W or scale gives other bits."""
    rois = U.exact_rois()
    lv = rule_levels(rois)
    assert set(lv.tolist()) == {0, 1, 2, 3}
    if which == "permuted":
        moved = X.permuted_levels(lv)
        assert (moved != lv).sum() >= 10
        lv = moved
    ref = X.pyramid_reference(lv, C_, sr)
    got = X.run_roi_align(pyramid_device(C_, dt), X.PYR_SCALES, torch.from_numpy(rois).to(G.DEV),
                          torch.from_numpy(lv.astype(np.int32)).to(G.DEV), X.PYR_P, sr, True, dt, "sep")
    bad = differing_rois(got, expect_bits(ref, X.TD[dt]))
    assert not bad, f"{X.NAME[dt]} {which} sr={sr}: RoIs {bad} (levels {lv[bad].tolist()}) differ"


# ---- vk_roi_align, not exact: per element under the derived bound ----------------------------------------------------------------------
ROUGH = [(f, dt, C_, *g) for f in X.FORMS for dt, C_ in X.ROUGH_CASES[f] for g in X.ROUGH_GEOMS[f]]


@pytest.mark.parametrize("f,dt,C_,P,sr,aligned", ROUGH, ids=[f"{f}-{X.NAME[dt]}-C{c}-P{P}-sr{sr}-{'al' if al else 'un'}" for f, dt, c, P, sr, al in ROUGH])
def test_roi_align_per_element_bound(f, dt, C_, P, sr, aligned):
    td = X.TD[dt]
    x, rois = X.rough_map(C_, td), X.rough_rois()
    ref, bound = X.rough_reference(x, rois, P, X.S16, sr, aligned, td)
    got = X.run_roi_align([nhwc(x, td)], [X.S16], torch.from_numpy(rois).to(G.DEV), None, P, sr, aligned, dt, f)
    worst = X.worst_ratio(got.float().permute(0, 3, 1, 2).numpy(), ref, bound)
    print(f"\n[vk_roi_align {X.NAME[dt]} {f} P={P} sr={sr} aligned={int(aligned)}] worst |out - ref| / bound {worst:.3f}")
    assert np.abs(ref).max() > 0.5 and worst <= 1


# ---- the FPN glue: bit-equal ----------------------------------------------------------------------------------------------------------
def same_bits_outside_nan(got, expect):
    """NaN where expect is NaN (a NaN's sign and payload are the adder's choice), the same bytes everywhere else."""
    nan = torch.isnan(expect)
    assert torch.equal(torch.isnan(got), nan)
    return torch.equal(got.view(IDT[got.dtype])[~nan], expect.view(IDT[expect.dtype])[~nan])


def device_copy(t, shift):
    """A device copy of t with one sentinel element behind it, starting `shift` elements into its allocation
    (shift = 1: base % 16 == 2 or 4, never 16-byte aligned) -> (the view shaped as t, the whole flat buffer)."""
    flat = torch.full((t.numel() + shift + 1,), X.SENTINEL, dtype=t.dtype, device=G.DEV)
    flat[shift:shift + t.numel()] = t.flatten().to(G.DEV)
    view = flat[shift:shift + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == (shift * t.element_size()) % 16
    return view, flat


def guards_intact(flat, shift, n):
    g = torch.cat([flat[:shift], flat[shift + n:]]).cpu()
    return bool((g == X.SENTINEL).all())


def special_values(td):
    return torch.tensor([float("inf"), -float("inf"), float("nan"), -0.0, 0.0, torch.finfo(td).max, -torch.finfo(td).max, 65504.0, 1.0,
                         torch.finfo(td).tiny / 2], dtype=torch.float32).to(td)


UPS_SHAPES = ((1, 1, 1, 1), (5, 7, 3, 4), (6, 8, 3, 4), (4, 6, 3, 5))        # H, W, Ht, Wt; the last top map is larger than needed


@pytest.mark.parametrize("C_", [8, 12, 256])
@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_upsample2x_add_bit_equal(dt, C_):
    """y = lateral + nearest-2x(top): the fp32 sum rounded once.  16-bit types with C % 8 == 0 run the 16-byte form on aligned
    tensors and the scalar form on views one element into their allocations: the same bytes."""
    td, N = X.TD[dt], 2
    gen = torch.Generator().manual_seed(C_)
    for H, W, Ht, Wt in UPS_SHAPES:
        lat = (torch.randn((N, H, W, C_), generator=gen) * 4).to(td)
        top = (torch.randn((N, Ht, Wt, C_), generator=gen) * 4).to(td)
        sp = special_values(td)[:8]
        lat[0, 0, 0, :8] = sp                                    # special + ordinary
        top[1, 0, 0, :8] = sp                                    # ordinary + special, read by up to four pixels
        big = torch.finfo(td).max
        lat[-1, -1, -1, :8] = torch.tensor([float("inf"), -float("inf"), big, -big, float("nan"), -0.0, 65504.0, -0.0]).to(td)
        top[-1, (H - 1) // 2, (W - 1) // 2, :8] = torch.tensor([-float("inf"), -float("inf"), big, -big, 1.0, -0.0, 65504.0, 0.0]).to(td)
        hh, ww = torch.arange(H) // 2, torch.arange(W) // 2
        expect = (lat.float() + top[:, hh][:, :, ww].float()).to(td)
        assert torch.isinf(expect).any() and torch.isnan(expect).any()
        outs = []
        for shift in (0, 1):
            (a, _), (b, _), (y, yflat) = device_copy(lat, shift), device_copy(top, shift), device_copy(torch.full_like(lat, 3.0), shift)
            L.call("vk_upsample2x_add", G.P(a), G.P(b), G.P(y), N, H, W, Ht, Wt, C_, dt, G.stream())
            torch.cuda.synchronize()
            assert guards_intact(yflat, shift, lat.numel()), (H, W, shift)
            outs.append(y.cpu())
            assert same_bits_outside_nan(outs[-1], expect), (H, W, Ht, Wt, shift)
        nan = torch.isnan(expect)
        assert torch.equal(outs[0].view(IDT[td])[~nan], outs[1].view(IDT[td])[~nan])


@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_upsample2x_add_refuses_a_top_map_that_is_too_small(dt):
    td = X.TD[dt]
    lat, top = torch.ones((2, 5, 7, 8), dtype=td, device=G.DEV), torch.ones((2, 3, 4, 8), dtype=td, device=G.DEV)
    y = torch.full((2, 5, 7, 8), X.SENTINEL, dtype=td, device=G.DEV)
    lib = L.load()
    for Ht, Wt in ((2, 4), (3, 3), (0, 4)):
        assert lib.vk_upsample2x_add(G.P(lat), G.P(top), G.P(y), 2, 5, 7, Ht, Wt, 8, dt, G.stream()) == L.VK_EINVAL
    torch.cuda.synchronize()
    assert bool((y == X.SENTINEL).all())


def random_bits(shape, td, seed):
    """Every bit pattern of the type can occur: NaNs with payloads, infinities, subnormals, both zeros."""
    gen = torch.Generator().manual_seed(seed)
    info = torch.iinfo(IDT[td])
    return torch.randint(info.min, info.max + 1, shape, generator=gen, dtype=torch.int64).to(IDT[td]).view(td)


@pytest.mark.parametrize("C_", [3, 8, 256])
@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_subsample2_is_every_second_pixel(dt, C_):
    td, N = X.TD[dt], 2
    for H, W in ((1, 1), (2, 2), (5, 7), (6, 8)):
        x = random_bits((N, H, W, C_), td, H * 100 + C_)
        x.view(IDT[td]).view(-1)[-1] = 0x7FA5 if td != torch.float32 else 0x7FA5A5A5          # a NaN with a payload, last pixel kept
        assert torch.isnan(x).any()
        expect = x[:, ::2, ::2].contiguous()
        y, yflat = device_copy(torch.zeros_like(expect), 0)
        L.call("vk_subsample2", G.P(x.to(G.DEV)), G.P(y), N, H, W, C_, dt, G.stream())
        torch.cuda.synchronize()
        assert guards_intact(yflat, 0, expect.numel())
        assert torch.equal(y.cpu().view(IDT[td]), expect.view(IDT[td])), (H, W)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
@pytest.mark.parametrize("dt", DTS, ids=[X.NAME[d] for d in DTS])
def test_relu_copy_is_torch_relu(dt, n):
    """Finite and infinite outputs are torch.relu's bytes on the CPU (-0.0 stays -0.0, subnormals stay); a NaN stays a NaN."""
    td = X.TD[dt]
    x = random_bits((n,), td, n + 1)
    sp = torch.cat([special_values(td), -special_values(td)])[:n]
    x[:len(sp)] = sp
    assert n < 20 or (torch.isnan(x).any() and (x.view(IDT[td]) == torch.tensor(-0.0, dtype=td).view(IDT[td])).any())
    expect = torch.relu(x)
    xd = torch.cat([x, torch.ones(1, dtype=td)]).to(G.DEV)             # never a null pointer, n = 0 included
    y, yflat = device_copy(torch.full((n,), 3.0, dtype=td), 0)
    L.call("vk_relu_copy", G.P(xd), G.P(yflat), n, dt, G.stream())
    torch.cuda.synchronize()
    assert guards_intact(yflat, 0, n)
    nan = torch.isnan(x)
    got = yflat[:n].cpu()
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(expect), nan)
    assert torch.equal(got.view(IDT[td])[~nan], expect.view(IDT[td])[~nan])
