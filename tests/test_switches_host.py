"""CPU: how every VK_* switch with a host-side query reads its text (csrc/runtime.hip env_*; the switches are listed in
DESIGN.md).  One geometry per switch, from the route tables of the GPU tests, at which the switch decides the answer; each
text of TEXTS is set in turn and the query's answer compared with the table below.  The table was written by running this
file as a script (`python tests/test_switches_host.py`) against the library as it was before the switches went through one
reader, and is kept as literals: a change of a reading rule has to change it here."""
import os
import subprocess
import sys

import pytest

from vltk_amd import _lib as L

TEXTS = (None, "", "0", "00", "1", "2", "8", "9", "A", "x")          # None: unset
F16, BF16 = L.VK_F16, L.VK_BF16
ROUTES = ("generic", "ring", "duo", "ws", "gemm4", "panel", "blk")      # VK_ROUTE_* by value (tests/gpu_util.py)
ATT = ("mfma", "lds", "tiled", "stream")                                # VK_ATT_ROUTE_* by value
RA = ("sep", "vec", "scalar")                                           # VK_RA_FORM_* by value


def conv_route_args(N, H, W, cin, cout, k=1, stride=1, pad=0, dil=1, groups=1, relu=0, cin2=0, res=False, mean=False):
    """vk_conv_route's argument list for an f16 layer, as tests/gpu_util.py conv_route builds it (no torch here)."""
    return (N, H, W, cin, cin2, int(res), int(mean), cout, (cout + 7) // 8 * 8, k, k, stride, pad, dil, groups, relu, F16, F16)


def conv(**geom):
    def query(lib):
        r = lib.vk_conv_route(*conv_route_args(**geom))
        return ROUTES[r] if r >= 0 else r
    return query


GEMM4_LONG = dict(N=5400, H=14, W=14, cin=1024, cout=512, relu=1)                       # gemm4/tail_dynamic
DUAL = dict(N=1, H=1, W=39917, cin=512, cin2=1024, cout=2048, relu=1)                   # gemm4/many_dual
RING_3X3 = conv_route_args(2, 25, 31, 64, 256, k=3, pad=1, relu=1)                      # ring_3x3
PHASE = (32, 14, 14, 2)

# switch -> (fixed environment, query): re-read per call, so one process sweeps them
PER_CALL = {
    "VK_CONV3X3_BLK": ({}, conv(N=5, H=14, W=14, cin=128, cout=128, k=3, pad=2, dil=2, groups=4)),       # edge/blk_norelu
    "VK_CONV3X3_PANEL": ({}, conv(N=5400, H=14, W=14, cin=512, cout=512, k=3, pad=2, dil=2, relu=1)),    # panel/tail_dynamic
    "VK_CONV_WS": ({}, conv(N=3, H=37, W=41, cin=128, cout=512, res=True, relu=1)),                      # edge/ws
    "VK_WS_POOL": ({}, conv(N=23, H=1, W=196, cin=512, cout=512, res=True, relu=1, mean=True)),          # mean/ws/23x196_512_512
    "VK_WS_STRIDED": ({}, conv(N=3, H=100, W=167, cin=256, cout=512, stride=2)),                         # edge/ws_norelu
    "VK_CONV_GEMM4": ({}, lambda lib: (conv(**GEMM4_LONG)(lib), conv(N=11, H=14, W=14, cin=1024, cout=512, relu=1)(lib))),   # + edge/gemm4
    "VK_GEMM4_MINK": ({}, lambda lib: (conv(**GEMM4_LONG)(lib), conv(**dict(GEMM4_LONG, cin=768))(lib))),
    "VK_CONV_DUO": ({}, conv(N=1, H=33, W=37, cin=192, cout=256, res=True, relu=1)),                     # duo_s6
    "VK_CONV_DUO (forcing)": ({"VK_CONV_GEMM4": "0"}, conv(**GEMM4_LONG)),                               # K = 1024, M >= 400000: the ring kernel's
    "VK_CONV256_DUAL": ({"VK_CONV_GEMM4": "0"}, conv(**DUAL)),
    "VK_PANEL_PHASE": ({}, lambda lib: lib.vk_panel_phase_images(*PHASE)),
    "VK_PANEL_TALL": ({}, lambda lib: lib.vk_panel_phase_tile_rows(*PHASE, 512)),
    "VK_PANEL_REUSE": ({}, lambda lib: lib.vk_panel_phase_reuse(*PHASE, 512)),
    "VK_ATTENTION_MFMA": ({}, lambda lib: ATT[lib.vk_attention_route(20, 36, 64, BF16, 64, 64, 64, 1, 0)]),
    "VK_ATTENTION_TILED": ({}, lambda lib: ATT[lib.vk_attention_route(100, 100, 64, BF16, 64, 64, 64, 1, 1)]),
    "VK_BNECK_FUSED": ({}, lambda lib: lib.vk_bottleneck64_eligible(256, 64, 256, 1, 1, 1, 0, 0, 32, 200, 334, F16)),
    "VK_BNECK_ROWS": ({}, lambda lib: lib.vk_bottleneck64_eligible(256, 64, 256, 1, 1, 1, 0, 0, 64, 200, 334, F16)),    # 2.19 GB of res2 map
    "VK_ROIALIGN_TABLES": ({}, lambda lib: RA[lib.vk_roi_align_form(256, 7, F16)]),                      # the FPN head's shape
}
# the texts an atoi switch tells apart, beyond TEXTS
MORE_TEXTS = {"VK_GEMM4_MINK": ("255", "256", "768", "1025", "-1")}

# read once per process (a `static const bool`): a fresh process per text, which asks both
ONCE_SCRIPT = """import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
print(lib.vk_fuse_shortcut(64, 64, 256, 1, %d), lib.vk_conv_route(*%r))""" % (F16, RING_3X3)
ONCE = ("VK_NO_FUSED_SHORTCUT", "VK_DISABLE_CONV256")       # vk_fuse_shortcut (res2.0); ring_3x3's route

_G, _P, _W, _D, _R = "gemm4", "panel", "ws", "duo", "ring"
EXPECTED = {
    # text:                 unset      ""         "0"        "00"       "1"        "2"        "8"        "9"        "A"        "x"
    "VK_CONV3X3_BLK":      ("blk",     "blk",     "generic", "generic", "blk",     "blk",     "blk",     "blk",     "blk",     "blk"),
    "VK_CONV3X3_PANEL":    (_P,        _P,        _R,        _R,        _P,        _P,        _P,        _P,        _P,        _P),
    "VK_CONV_WS":          (_W,        _W,        _D,        _D,        _W,        _W,        _W,        _W,        _W,        _W),
    "VK_WS_POOL":          (_W,        _W,        _D,        _D,        _W,        _W,        _W,        _W,        _W,        _W),
    "VK_WS_STRIDED":       (_W,        _W,        _D,        _D,        _W,        _W,        _W,        _W,        _W,        _W),
    "VK_CONV_GEMM4":       ((_G, _D),  (_G, _D),  (_R, _D),  (_R, _D),  (_G, _D),  (_G, _G),  (_G, _D),  (_G, _D),  (_G, _D),  (_G, _D)),
    # (K = 1024, K = 768): no text of TEXTS reaches 256, so all mean 1024; then "255", "256", "768", "1025", "-1"
    "VK_GEMM4_MINK":       ((_G, _R),) * 10 + ((_G, _R), (_G, _G), (_G, _G), (_R, _R), (_G, _R)),
    "VK_CONV_DUO":         (_D,        _D,        _R,        _R,        _D,        _D,        _D,        _D,        _D,        _D),
    "VK_CONV_DUO (forcing)": (_R,      _R,        _R,        _R,        _D,        _R,        _R,        _R,        _R,        _R),
    "VK_CONV256_DUAL":     (_R,        _R,        _D,        _D,        _R,        _R,        _R,        _R,        _R,        _R),
    "VK_PANEL_PHASE":      (32,        32,        0,         0,         32,        32,        32,        32,        32,        32),
    "VK_PANEL_TALL":       (512,       512,       256,       256,       512,       512,       512,       512,       512,       512),
    "VK_PANEL_REUSE":      (1,         1,         0,         0,         1,         1,         1,         1,         1,         1),
    "VK_ATTENTION_MFMA":   ("mfma",    "mfma",    "lds",     "lds",     "mfma",    "mfma",    "mfma",    "mfma",    "mfma",    "mfma"),
    "VK_ATTENTION_TILED":  ("tiled",   "tiled",   "lds",     "lds",     "tiled",   "tiled",   "tiled",   "tiled",   "tiled",   "tiled"),
    "VK_BNECK_FUSED":      (1,         1,         0,         0,         1,         1,         1,         1,         1,         1),
    "VK_BNECK_ROWS":       (1,         1,         0,         0,         1,         1,         1,         1,         1,         1),
    # set and atoi == 0 takes the tables out, "" and non-numbers included
    "VK_ROIALIGN_TABLES":  ("sep",     "vec",     "vec",     "vec",     "sep",     "sep",     "sep",     "sep",     "vec",     "vec"),
    # presence alone decides, "" included: (vk_fuse_shortcut, route) per text
    "once":                ("1 1",     "0 0",     "0 0",     "0 0",     "0 0",     "0 0",     "0 0",     "0 0",     "0 0",     "0 0"),
}


def texts_of(switch):
    return TEXTS + MORE_TEXTS.get(switch, ())


def sweep(lib, switch, setenv, delenv):
    fixed, query = PER_CALL[switch]
    name = switch.split()[0]
    for k, v in fixed.items():
        setenv(k, v)
    got = []
    for text in texts_of(switch):
        if text is None:
            delenv(name)
        else:
            setenv(name, text)
        got.append(query(lib))
    return tuple(got)


def sweep_once(text):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VK_")}
    if text is not None:
        env.update({name: text for name in ONCE})
    return subprocess.run([sys.executable, "-c", ONCE_SCRIPT, L.LIB_PATH], env=env, check=True, capture_output=True, text=True).stdout.strip()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("VK_")]:
        monkeypatch.delenv(k)


def test_the_table_covers_the_sweep():
    assert set(EXPECTED) == set(PER_CALL) | {"once"}
    for switch in PER_CALL:
        assert len(EXPECTED[switch]) == len(texts_of(switch)), switch
        assert len(set(EXPECTED[switch])) > 1, f"{switch} decides nothing at its geometry"
    assert len(EXPECTED["once"]) == len(TEXTS)


@pytest.mark.parametrize("switch", sorted(PER_CALL))
def test_per_call_switch_reads_as_before(lib, monkeypatch, switch):
    got = sweep(lib, switch, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert got == EXPECTED[switch], dict(zip(texts_of(switch), zip(got, EXPECTED[switch])))


def test_read_once_switches_read_as_before(lib):
    got = tuple(sweep_once(t) for t in TEXTS)
    assert got == EXPECTED["once"], dict(zip(TEXTS, zip(got, EXPECTED["once"])))


if __name__ == "__main__":      # the table, from the library VLTK_AMD_LIB names (or the tree's)
    for k in [k for k in os.environ if k.startswith("VK_")]:
        del os.environ[k]
    for sw in PER_CALL:
        print(f"{sw!r}: {sweep(L.load(), sw, os.environ.__setitem__, lambda k: os.environ.pop(k, None))!r},")
        for k in [k for k in os.environ if k.startswith("VK_")]:
            del os.environ[k]
    print(f"'once': {tuple(sweep_once(t) for t in TEXTS)!r},")
