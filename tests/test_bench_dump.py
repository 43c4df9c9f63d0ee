"""CPU: bench.py --dump-outputs writes the arrays of one step as <name>.npy in float32 / float64, keeps a seeded sample of
the images when they exceed the size limit, and bench.py refuses a run without timed steps."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench
from vltk_amd.parallel import output_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(N=6, D=5, F=16):
    g = torch.Generator().manual_seed(0)
    out = {}
    for k, shape, dt in output_spec(N, D, F):
        out[k] = torch.randint(0, 1601, shape, generator=g, dtype=dt) if dt == torch.int64 else torch.rand(shape, generator=g)
    return out


def test_dump_writes_every_array(tmp_path):
    out = _step()
    rec = bench.dump_outputs(out, str(tmp_path / "d"))
    assert rec["arrays"] == sorted(out) and rec["images"] == "6 of 6"
    for k, v in out.items():
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == (np.float64 if v.dtype == torch.int64 else np.float32), (k, a.dtype)
        np.testing.assert_array_equal(a, v.numpy())           # integer ids are exact in float64
    assert not (tmp_path / "d" / "sample_images.npy").exists()


def test_dump_samples_the_same_images_above_the_limit(tmp_path):
    out = _step(N=40)
    per_image = sum(v[0].numel() * (8 if v.dtype == torch.int64 else 4) for v in out.values()) + 8
    recs = [bench.dump_outputs(out, str(tmp_path / d), limit=10 * per_image) for d in ("a", "b")]
    assert recs[0]["images"] == "10 of 40" and "sample_images" in recs[0]["arrays"]
    idx = np.load(tmp_path / "a" / "sample_images.npy")
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "sample_images.npy"))     # seeded: same rows every run
    rows = idx.astype(np.int64)
    assert len(np.unique(rows)) == 10
    total = 0
    for k, v in out.items():
        a = np.load(tmp_path / "a" / (k + ".npy"))
        np.testing.assert_array_equal(a, v.numpy()[rows])
        total += a.nbytes
    assert total + idx.nbytes <= 10 * per_image


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
