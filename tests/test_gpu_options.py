"""-m gpu: the handle's options (vk_set_option / vk_get_option, csrc/model.hip: kOptions) on real handles.  No forward runs:
a handle of the golden fixture's configuration (ResNet-101-C4, R = 30, D = 12) is created and asked.

The expected values are the header's documented ranges and defaults (include/vltk_hip.h, "Tunables"), written out here and
not read back from the library."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from vltk_amd import FRCNN, vg_c4_config   # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# key: (built-in default, legal values that are not the default, illegal values, the range message)
WRITABLE = {
    "head_chunk": (9600, (0, 1, 4800), (-1, -9600), "head_chunk must be >= 0 (0 = all RoIs at once)"),
    "backbone_streams": (2, (1, 3, 4), (0, 5, -1), "backbone_streams must be 1..4"),
    "head_streams": (1, (2,), (0, 3, -1), "head_streams must be 1 or 2"),
    "forward_lanes": (2, (1,), (0, 3, -1), "forward_lanes must be 1 or 2"),
    "head_dedupe": (1, (0,), (-1, 2), "head_dedupe must be 0 or 1"),
    "head_split_min_rois": (512, (2, 4096), (1, 0, -1), "head_split_min_rois must be >= 2"),
    "backbone_split_min_batch": (8, (2, 64), (1, 0, -1), "backbone_split_min_batch must be >= 2"),
}
ORDER = ("head_chunk", "backbone_streams", "head_streams", "forward_lanes", "head_dedupe", "head_split_min_rois",
         "backbone_split_min_batch")
READ_ONLY = ("dedupe_chunks", "working_sets", "lane_forwards")
VARIABLES = ("VK_HEAD_CHUNK", "VK_BACKBONE_STREAMS", "VK_HEAD_STREAMS", "VK_FORWARD_LANES", "VK_HEAD_DEDUPE")


def fixture_config(golden_dir):
    g = np.load(os.path.join(golden_dir, "e2e_r101_small.npz"))
    return dict(depth=int(g["depth"]), post_nms_topk=int(g["post_topk"]), detections=int(g["det"]))


@pytest.fixture(scope="module")
def model(golden_dir):
    return FRCNN(vg_c4_config(**fixture_config(golden_dir)), precision="fp16")


def test_the_table_here_names_every_writable_key():
    assert set(WRITABLE) == set(ORDER) and len(ORDER) == 7


@pytest.mark.parametrize("key", ORDER)
def test_set_get_round_trip(model, key):
    default, legal, illegal, message = WRITABLE[key]
    for v in legal:
        assert v != default
        model.set_option(key, v)
        assert model.get_option(key) == v, (key, v)
        for bad in illegal:
            with pytest.raises(ValueError, match=re.escape(message)):
                model.set_option(key, bad)
            assert model.get_option(key) == v, (key, bad)       # the stored value is untouched
    model.set_option(key, default)
    assert model.get_option(key) == default


def test_setting_one_option_leaves_the_others(model):
    before = [model.get_option(k) for k in ORDER]
    for i, key in enumerate(ORDER):
        v = WRITABLE[key][1][0]
        model.set_option(key, v)
        want = list(before)
        want[i] = v
        assert [model.get_option(k) for k in ORDER] == want, key
        model.set_option(key, before[i])
    assert [model.get_option(k) for k in ORDER] == before


@pytest.mark.parametrize("key", READ_ONLY)
def test_read_only_keys(model, key):
    assert model.get_option(key) == 0                   # no forward has run on this handle: no chunk, no arena, no lane
    for v in (0, 1):
        with pytest.raises(ValueError, match=re.escape(f"unknown option '{key}'")):
            model.set_option(key, v)
    assert model.get_option(key) == 0


def test_unknown_key(model):
    with pytest.raises(ValueError, match=re.escape("unknown option 'head_chunks'")):
        model.get_option("head_chunks")
    with pytest.raises(ValueError, match=re.escape("unknown option 'head_chunks'")):
        model.set_option("head_chunks", 1)


_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from vltk_amd import FRCNN, vg_c4_config
m = FRCNN(vg_c4_config(**json.loads(sys.argv[2])), precision="fp16")
print(json.dumps([m.get_option(k) for k in json.loads(sys.argv[3])]))
"""


def new_handle_reports(golden_dir, variables):
    """The seven options of a handle created in a fresh process whose only VK_* variables are `variables`."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("VK_")}
    env.update(variables)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(fixture_config(golden_dir)), json.dumps(ORDER)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_defaults_from_the_environment(golden_dir):
    got = new_handle_reports(golden_dir, dict(zip(VARIABLES, ("77", "3", "2", "1", "0"))))
    assert got == [77, 3, 2, 1, 0, 512, 8]


def test_built_in_defaults(golden_dir):
    assert new_handle_reports(golden_dir, {}) == [9600, 2, 1, 2, 1, 512, 8]
    assert [WRITABLE[k][0] for k in ORDER] == [9600, 2, 1, 2, 1, 512, 8]
