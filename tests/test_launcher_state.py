"""Launcher state is per device and lives in one place (csrc/runtime.hip: device_state, set_max_lds, Timed).

CPU: no other translation unit raises an LDS limit, queries device properties or keeps function-local state, so a process
may hold handles on several devices; none calls getenv (runtime.hip's env_* read the environment), and the VK_* names they
are asked for are the rows of DESIGN.md's table of switches.  -m gpu (two or more devices): the same model on cuda:1 and then cuda:0 in one
process gives the same bits."""
import glob
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "vltk_amd", "csrc")

# an indented `static` (function-local state, also inside a multi-line macro) other than a constant or a device member function
LOCAL_STATIC = re.compile(r"^[ \t]+static\b(?!\s+(const|constexpr|__device__)\b)")
DEVICE_CALLS = re.compile(r"\b(hipFuncSetAttribute|hipGetDeviceProperties)\b")


def test_launchers_keep_no_state_of_their_own():
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert os.path.join(CSRC, "runtime.hip") in srcs
    assert {"model.hip", "pack.hip", "stage_api.hip"} <= {os.path.basename(p) for p in srcs}      # scanned like every other unit
    bad = []
    for path in srcs:
        if os.path.basename(path) == "runtime.hip":      # where the shared helpers live
            continue
        with open(path) as f:
            for n, line in enumerate(f, 1):
                if DEVICE_CALLS.search(line) or LOCAL_STATIC.search(line):
                    bad.append(f"{os.path.basename(path)}:{n}: {line.strip()}")
    assert not bad, "\n".join(bad)


ENV_CALL = re.compile(r"\benv_(?:text|set|first|off|int)\(\s*\"(VK_[A-Z0-9_]+)\"")


def test_only_the_runtime_reads_the_environment():
    bad = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        if os.path.basename(path) != "runtime.hip":
            with open(path) as f:
                bad += [f"{os.path.basename(path)}:{n}: {line.strip()}" for n, line in enumerate(f, 1) if "getenv" in line]
    assert not bad, "\n".join(bad)


def test_design_lists_every_switch():
    """The VK_* names passed to env_* anywhere in csrc, plus the `env` column of model.hip's kOptions, are the names of the
    table in DESIGN.md's section on the environment switches: no more, no fewer."""
    read = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(path) as f:
            read |= set(ENV_CALL.findall(f.read()))
    with open(os.path.join(CSRC, "model.hip")) as f:
        table = re.search(r"kOptions\[\] = \{(.*?)\n\};", f.read(), re.S).group(1)
    options = set(re.findall(r'"(VK_[A-Z0-9_]+)", ENV_', table))
    assert len(options) == 5 and len(read) > 30, (options, read)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        section = re.search(r"\n## \d+\. The environment switches[^\n]*\n(.*?)(?=\n## |\Z)", f.read(), re.S).group(1)
    rows = re.findall(r"^\| `(VK_[A-Z0-9_]+)` \|", section, re.M)
    assert len(rows) == len(set(rows)), sorted(r for r in rows if rows.count(r) > 1)
    assert set(rows) == read | options, (sorted(set(rows) - read - options), sorted((read | options) - set(rows)))


def test_scan_patterns():
    assert LOCAL_STATIC.search("    static bool attr_set = false;")
    assert LOCAL_STATIC.search("        static char *zero_page = nullptr;   \\")
    assert LOCAL_STATIC.search("    static std::atomic<unsigned> next[VK_MAX_DEVICES];")
    assert not LOCAL_STATIC.search("    static const bool off = getenv(\"X\") != nullptr;")
    assert not LOCAL_STATIC.search("    static constexpr int N = 8;")
    assert not LOCAL_STATIC.search("    static __device__ __forceinline__ floatx4 mfma(vec a, vec b, floatx4 c) {")
    assert not LOCAL_STATIC.search("static int launch_t(const ConvK &k, hipStream_t stream) {")
    assert not LOCAL_STATIC.search("    static const bool off = env_set(\"X\");")
    assert ENV_CALL.findall('if (env_off("VK_A") || env_int( "VK_B2", 1) == 0 || env_off(name)) x = env_text("VK_C_D");') == ["VK_A", "VK_B2", "VK_C_D"]


@pytest.mark.gpu
def test_two_devices_one_process():
    """The fp16 C4 model at 800x1333 (stem_pool, bneck_fused, the panel 3x3, conv_gemm4 and conv_ws: kernels with more than
    64 KiB of LDS) built and run on cuda:1 first, then on cuda:0: the output blocks are bit-equal."""
    import torch

    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    cfg = vg_c4_config(post_nms_topk=300, detections=100)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(4, 800, 1333, seed=0xD2))
    shapes = torch.tensor([[800, 1333]] * 4)
    outs = []
    for i, dev in enumerate(("cuda:1", "cuda:0")):
        m = FRCNN(cfg, precision="fp16", device=dev).load_state_dict(sd).eval()
        if i == 0:
            m.enable_kernel_timing(True)
            m.kernel_timing(reset=True)
        m(x, shapes)
        outs.append({k: v.cpu() for k, v in m.forward_padded().items()})
        if i == 0:
            kt = m.kernel_timing()
            ran = {k: kt[k]["launches"] for k in ("other", "bneck64", "conv3x3_panel", "conv_gemm4", "conv_ws")}
            assert all(n > 0 for n in ran.values()), ran
        del m
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
