"""GPU (-m gpu): `vk_index_add_rows` and `vk_embed_sum_f32` (csrc/index_add.hip) through their op wrappers.  Exact: integer `src` in
[-8, 8], sums far below 2^24, so the result equals `np.add.at` in float64 cast to float32 bit for bit; `dst` is pre-filled with NaN and
its columns past C and a guard row behind it stay NaN.  S = 32 is the chunk of the segmented sum, 1024 the tile of a sort workgroup.
Bound: Gaussian `src`, |out - ref| <= 2^-24 |ref| + 2^-32 sum |terms| (one fp32 rounding; an fp64 sum of at most 2^21 terms)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd.train import embed_sum_f32, index_add_rows                                 # noqa: E402

S = 32
DEV = "cuda:0"


def indices(kind, n, R, g):
    if kind == "same":
        return np.full(n, R // 2)
    if kind == "distinct":
        return g.permutation(R)[:n]
    if kind == "boundary":                   # the run of row 0 fills chunk 0 exactly; row 1 crosses from chunk 1 into chunk 2
        return g.permutation(np.repeat(np.arange(3), (S, S + 3, n - 2 * S - 3)))
    idx = g.integers(0, R, n)
    idx[0] = R - 1                           # the last row is named: every digit of the key counts
    if kind == "oob":
        idx[::5] = g.choice([-1, -R, R, R + 7, 2 ** 31 - 1], len(idx[::5]))
    return idx


# id: (n, R, C, index kind, options: ld_src, ld_dst, pad, rows (None | "repeat" | "two" | "oob"))
CASES = {
    "n=1": (1, 5, 4, "rand", {}), "R=1": (70, 1, 3, "rand", {}), "one-run": (3 * S + 5, 40, 4, "same", {}),
    "distinct": (100, 100, 4, "distinct", {}), "n=S-1": (S - 1, 7, 4, "rand", {}), "n=S": (S, 7, 4, "rand", {}),
    "n=S+1": (S + 1, 7, 4, "rand", {}), "n=2S+1": (2 * S + 1, 7, 4, "rand", {}), "R=255": (300, 255, 4, "rand", {}),
    "R=256": (300, 256, 4, "rand", {}), "R=257": (300, 257, 4, "rand", {}), "R=65537": (300, 65537, 4, "rand", {}),
    "C=1": (2 * S + 1, 50, 1, "rand", {}), "C=3": (2 * S + 1, 50, 3, "rand", {}), "C=768": (2 * S + 1, 50, 768, "rand", {}),
    "ld-chunked": (90, 9, 4, "rand", dict(ld_src=8, ld_dst=12)), "ld-scalar": (90, 9, 4, "rand", dict(ld_src=6, ld_dst=7)),
    "ld-C=3": (90, 9, 3, "rand", dict(ld_src=5, ld_dst=4)), "pad-named": (200, 9, 4, "rand", dict(pad=8)),
    "pad-unnamed": (200, 9, 4, "rand", dict(pad=8, n_rows=8)), "rows-repeat": (200, 30, 4, "rand", dict(rows="repeat")),
    "two-columns": (2 * 77, 30, 4, "rand", dict(rows="two")), "idx-outside": (300, 40, 4, "oob", {}),
    "rows-outside": (300, 40, 4, "rand", dict(rows="oob")), "boundary": (3 * S, 3, 4, "boundary", {}),
    "three-tiles": (2500, 300, 8, "rand", {}),
}


def problem(name, gaussian=False):
    n, R, C, kind, opt = CASES[name]
    g = np.random.Generator(np.random.PCG64([11, sum(map(ord, name))]))
    idx = indices(kind, n, opt.get("n_rows", R), g)          # n_rows < R: the rows past it are named by no entry
    M = {"repeat": 20, "two": n // 2, "oob": 50}.get(opt.get("rows"), n)         # src_row: repeats, two index columns, outside [0, M)
    rows = {"repeat": lambda: g.integers(0, M, n), "two": lambda: np.tile(np.arange(M), 2),
            "oob": lambda: g.integers(-3, M + 3, n)}.get(opt.get("rows"), lambda: None)()
    ld_src, ld_dst = opt.get("ld_src", C), opt.get("ld_dst", C)
    src = np.full((M, ld_src), np.nan, np.float32)
    src[:, :C] = g.standard_normal((M, C)) if gaussian else g.integers(-8, 9, (M, C))
    r = np.arange(n) if rows is None else rows
    pad = opt.get("pad", -1)
    keep = (idx >= 0) & (idx < R) & (idx != pad) & (r >= 0) & (r < M)
    terms = src[r[keep], :C].astype(np.float64)
    ref, mag = np.zeros((R, C)), np.zeros((R, C))
    np.add.at(ref, idx[keep], terms)
    np.add.at(mag, idx[keep], np.abs(terms))
    return dict(src=src, idx=idx.astype(np.int32), rows=None if rows is None else rows.astype(np.int32), R=R, C=C, pad=pad, ld_dst=ld_dst,
                ref=ref, mag=mag)


def launch(p):
    buf = torch.full((p["R"] + 1, p["ld_dst"]), float("nan"), dtype=torch.float32, device=DEV)
    src = torch.from_numpy(p["src"]).to(DEV)
    rows = None if p["rows"] is None else torch.from_numpy(p["rows"]).to(DEV)
    index_add_rows(src[:, :p["C"]], torch.from_numpy(p["idx"]).to(DEV), p["R"], rows, p["pad"], out=buf[:p["R"], :p["C"]])
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_exact(name):
    p = problem(name)
    assert np.abs(p["mag"]).max() < 2 ** 24
    got = launch(p)
    np.testing.assert_array_equal(got[:p["R"], :p["C"]].view(np.uint32), p["ref"].astype(np.float32).view(np.uint32))
    assert np.isnan(got[p["R"]]).all() and np.isnan(got[:, p["C"]:]).all()


@pytest.mark.parametrize("name", ["one-run", "C=768", "rows-repeat", "three-tiles"])
def test_bound_and_repeatable(name):
    p = problem(name, gaussian=True)
    got, again = launch(p), launch(p)
    np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    err = np.abs(got[:p["R"], :p["C"]].astype(np.float64) - p["ref"])
    bound = 2.0 ** -24 * np.abs(p["ref"]) + 2.0 ** -32 * p["mag"]
    assert (err <= bound).all()


@pytest.mark.parametrize("C", [3, 32])
@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("T", [1, 3, 9])
def test_embed_sum(T, base, C):
    g = np.random.Generator(np.random.PCG64([12, T, C]))
    M = 37
    sizes = g.integers(1, 20, T)
    tables = [g.standard_normal((r, C)).astype(np.float32) for r in sizes]
    idx = np.stack([g.integers(0, r, M) for r in sizes]).astype(np.int32)
    idx[-1, 5], idx[0, 6] = sizes[-1] + 3, -2                                      # past its table and below it: clamped
    b = g.standard_normal((M, C)).astype(np.float32) if base else None
    terms = ([] if b is None else [b]) + [tab[np.clip(idx[t], 0, sizes[t] - 1)] for t, tab in enumerate(tables)]
    ref = functools.reduce(np.add, terms)                                          # the same fp32 adds, left to right
    out = embed_sum_f32([torch.from_numpy(t).to(DEV) for t in tables], torch.from_numpy(idx).to(DEV),
                        base=None if b is None else torch.from_numpy(b).to(DEV))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
