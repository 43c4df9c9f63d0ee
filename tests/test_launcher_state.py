"""Launcher state is per device and lives in one place (csrc/runtime.hip: device_state, set_max_lds, Timed).

CPU: no other translation unit raises an LDS limit, queries device properties or keeps function-local state, so a process
may hold handles on several devices.  -m gpu (two or more devices): the same model on cuda:1 and then cuda:0 in one
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


def test_scan_patterns():
    assert LOCAL_STATIC.search("    static bool attr_set = false;")
    assert LOCAL_STATIC.search("        static char *zero_page = nullptr;   \\")
    assert LOCAL_STATIC.search("    static std::atomic<unsigned> next[VK_MAX_DEVICES];")
    assert not LOCAL_STATIC.search("    static const bool off = getenv(\"X\") != nullptr;")
    assert not LOCAL_STATIC.search("    static constexpr int N = 8;")
    assert not LOCAL_STATIC.search("    static __device__ __forceinline__ floatx4 mfma(vec a, vec b, floatx4 c) {")
    assert not LOCAL_STATIC.search("static int launch_t(const ConvK &k, hipStream_t stream) {")


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
