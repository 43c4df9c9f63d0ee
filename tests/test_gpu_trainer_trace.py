"""GPU (-m gpu): a step of `EncoderTrainer` and of `HeadTrainer` asks of the library what it asked before the trainers were folded
onto one layer walk, one Linear backward and one base class, and leaves the same bits.

tests/golden/trainer_steps.json was recorded by tools/gen_golden_trainer.py from the trainers of the commit it names
("recorded_at"), on an MI355X, twice in two processes with identical files.  Six scenarios of two steps each (the generator's
docstring lists them); the test runs the generator's own `record()` on the trainers as they are now.

  trace   the second step's calls through `_lib.call`: names, order, every integer and float argument, every pointer argument as
          null / non-null.  Device-independent, always asserted.
  bits    SHA-256 over the two losses, then `grads()` and `state_dict()` after the second step, all of it: nothing had to be left
          out, the parent reproduces every tensor.  Asserted on the device the file was recorded on (by
          `torch.cuda.get_device_name(0)`); on another device this half alone is skipped, with the reason."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tools.gen_golden_trainer import SCENARIOS, record                                   # noqa: E402


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_steps.json")) as f:
        return json.load(f)["scenarios"]


@functools.lru_cache(maxsize=None)
def now(scenario):
    """One run of the scenario, shared by its two tests."""
    return record(scenario)


def test_the_file_holds_every_scenario():
    assert tuple(golden()) == SCENARIOS
    for name, g in golden().items():
        assert g["trace"] and all(len(v) == 64 for v in g["sha256"].values()), name


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_a_step_issues_the_recorded_calls(scenario):
    want, got = golden()[scenario]["trace"], now(scenario)["trace"]
    print(f"{scenario}: {len(got)} calls (recorded {len(want)})")
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert json.dumps(g) == json.dumps(w), f"call {i}"                               # 1 is not 1.0 and not true here


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_two_steps_leave_the_recorded_bits(scenario):
    device, by_device = torch.cuda.get_device_name(0), golden()[scenario]["sha256"]
    if device not in by_device:
        pytest.skip(f"the digests were recorded on {sorted(by_device)}, this device is '{device}': another device may sum in another "
                    "order, so only the calls are compared here")
    got = now(scenario)["sha256"]
    print(f"{scenario} on {device}: sha256 {got}")
    assert got == by_device[device]
