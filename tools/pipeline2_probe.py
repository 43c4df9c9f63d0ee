#!/usr/bin/env python3
"""Probe (GPU box): what do two forward lanes buy?  ONE model instance runs bench.py's loop shape (forward i+1 is begun
before forward i is waited for) with option "forward_lanes" = 1 and = 2, interleaved, ROUNDS times; with 2, batch i+1's
backbone / RPN / proposals run beside batch i's Res5 head in the handle's second working set.  One JSON line per round.
Environment: B (batch, 32), STEPS (12), ROUNDS (3)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config  # noqa: E402


def main():
    B, steps, rounds = (int(os.environ.get(k, d)) for k, d in (("B", "32"), ("STEPS", "12"), ("ROUNDS", "3")))
    cfg = vg_c4_config(post_nms_topk=300, detections=100, device="cuda:0")
    model = FRCNN(cfg, precision="fp16", device="cuda:0").load_state_dict(make_state_dict(cfg, seed=1234)).eval()
    images = torch.from_numpy(synthetic_images(B, 800, 1333, seed=0xF2C)).cuda(0)
    shapes = torch.tensor([[800, 1333]] * B)

    def run(lanes, n):
        model.set_option("forward_lanes", lanes)
        infl, last = [], None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            infl.append(model.forward_async(images, shapes))
            if len(infl) > 1:
                last = infl.pop(0).wait_raw()
        while infl:
            last = infl.pop(0).wait_raw()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, last

    ref = None
    for lanes in (1, 2):
        out = run(lanes, 4)[1]                   # warm-up (the second working set is allocated here); same bits either way
        cur = {k: v.clone() for k, v in out.items()}
        if ref is not None:
            assert all(torch.equal(ref[k], cur[k]) for k in ref), "forward_lanes changes the outputs"
        ref = cur
    for rnd in range(rounds):
        a = run(1, steps)[0]
        b = run(2, steps)[0]
        print(json.dumps({"round": rnd, "batch": B, "steps": steps, "one_lane_ms": round(a * 1e3, 3), "two_lanes_ms": round(b * 1e3, 3),
                          "gain_pct": round(100 * (a / b - 1), 2)}), flush=True)


if __name__ == "__main__":
    main()
