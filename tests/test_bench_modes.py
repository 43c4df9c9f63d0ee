"""bench.py's two modes: a plain run reports the headline only (set-up, warm-up, timed steps, dump, one JSON line);
--full adds the breakdown pass (ms_per_step_with_timers, roofline), the parity record (r101) and the CPU baseline (C4
models only: the CPU oracle has no FPN model)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("ms_per_step_with_timers", "roofline", "parity", "cpu_baseline")


def _bench(*extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], capture_output=True, text=True, env=env,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_full_is_an_option_and_off_by_default():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout
    assert "--no-cpu-baseline" in r.stdout and "--no-parity" in r.stdout


@pytest.mark.parametrize("arch,world,flags,want", [
    ("r101", 1, {}, ["parity", "cpu_baseline"]),
    ("r101", 1, {"no_parity": True, "no_cpu_baseline": True}, []),
    ("r101", 2, {}, ["parity"]),                          # the CPU baseline is a one-GPU figure
    ("x152", 1, {}, ["cpu_baseline"]),                    # parity fixtures are ResNet-101
    ("r101-fpn", 1, {}, []),                              # the CPU oracle is C4 only
])
def test_side_records_follow_the_arch(arch, world, flags, want):
    a = argparse.Namespace(**{"arch": arch, "no_parity": False, "no_cpu_baseline": False, **flags})
    assert bench.side_records(a, world) == want


def test_cpu_baseline_record():
    """What --full runs for the C4 models, at one image and one run instead of 4 images x 3 runs."""
    from vltk_amd import make_state_dict, vg_c4_config
    cfg = vg_c4_config(post_nms_topk=300, detections=100)
    rec = bench.cpu_baseline(cfg, make_state_dict(cfg, seed=1234), 300, 100, seed=0xF2C, n_images=1, repeats=1)
    assert rec["unit"] == "images/sec" and rec["value"] > 0 and rec["cores"] >= 1
    assert rec["sample"].startswith("1 images 800x1333")


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(tmp_path):
    d = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path / "d"))
    assert all(k in d for k in HEADLINE), d
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"] + 1e-2
    assert not [k for k in FULL_ONLY if k in d], d
    assert d["dump_outputs"]["images"] == "4 of 4"
    assert np.load(tmp_path / "d" / "preds_per_image.npy").shape == (4,)


@pytest.mark.gpu
def test_full_run_adds_the_breakdown_and_parity():
    d = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--full", "--no-cpu-baseline")
    assert all(k in d for k in HEADLINE), d
    assert d["ms_per_step_with_timers"] > 0
    rl = d["roofline"]
    assert rl["per_kernel"] and rl["stages_last_step"]["backbone"]["ms"] > 0 and rl["achieved"] > 0
    assert "error" not in d["parity"] and "full_size" in d["parity"], d["parity"]
    assert "cpu_baseline" not in d


@pytest.mark.gpu
def test_full_run_x152():
    d = _bench("--arch", "x152", "--gpus", "1", "--steps", "1", "--warmup", "0", "--batch", "2", "--detections", "36",
               "--full", "--no-cpu-baseline")
    assert d["ms_per_step_with_timers"] > 0 and d["roofline"]["per_kernel"] and d["roofline"]["achieved"] > 0
    assert "ResNeXt-152" in d["config"]["workload"]
    assert "parity" not in d and "cpu_baseline" not in d


@pytest.mark.gpu
def test_full_run_fpn():
    """The FPN detector under --full with the default flags: stage roofline, no parity, no CPU baseline (C4 oracle)."""
    d = _bench("--arch", "r101-fpn", "--gpus", "1", "--steps", "1", "--warmup", "0", "--batch", "2", "--full")
    assert all(k in d for k in HEADLINE), d
    assert d["ms_per_step_with_timers"] > 0
    st = d["roofline"]["stages_last_step"]
    assert st["backbone"]["ms"] > 0 and st["backbone"]["tflops"] > 0 and d["roofline"]["achieved"] > 0
    assert "parity" not in d and "cpu_baseline" not in d
