#!/usr/bin/env python3
"""Option "head_dedupe" (Res5 block 0 over the distinct RoIPool windows) on one GPU: the bins-per-window ratio
of the bench's own batch, and the path's worst case -- given boxes whose windows are ALL distinct, where it can save nothing
and pays for the window table and the row gather.

    python tools/dedupe_bench.py [--batch 32 --boxes 300 --steps 10 --warmup 2 --pairs 3 --option head_dedupe --out FILE]

The model, weights and images are bench.py's (ResNet-101-C4 fp16, weights of seed 1234, synthetic_images(seed=0xF2C), R = 300).
Ratio: one detection forward, bins / windows read from the stage "head_windows" (the device-side count).  Worst case: `boxes`
boxes per image, built so that no two of an image's boxes * 196 bins pool the same window (distinct_boxes), forwards with
head_dedupe 0 and 1 interleaved `pairs` times; a timed window is `steps` forwards issued back to back between two device
synchronisations.  Writes one JSON file and prints it.

--option head_dedupe_taps: the same two measurements for the neighbourhood path -- the bench batch's distinct
nine-window neighbourhoods (stage "head_neighbourhoods") beside its windows, and the all-distinct boxes with head_dedupe_taps 0
against 1 (head_dedupe stays 1): what the neighbourhood table, the gather of conv2's rows and the index loads cost where no two
bins share a neighbourhood.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 14


def axis_candidates(cells):
    """[(start, size, mask)]: RoIs of `size` >= P cells from cell `start` on an axis of `cells` cells whose P bin ranges
    [floor(p * size / P), ceil((p + 1) * size / P)) (float32, as RoIPool computes them) are pairwise distinct; mask has one bit
    per distinct (lo, hi) range of the axis."""
    bit = {}
    out = []
    for size in range(P, cells + 1):
        b = np.float32(size) / np.float32(P)
        lo = np.floor(np.arange(P, dtype=np.float32) * b).astype(int)
        hi = np.ceil(np.arange(1, P + 1, dtype=np.float32) * b).astype(int)
        if len(set(zip(lo.tolist(), hi.tolist()))) < P:
            continue
        for start in range(0, cells - size + 1):
            m = 0
            for a, c in zip(lo.tolist(), hi.tolist()):
                m |= 1 << bit.setdefault((start + a, start + c), len(bit))
            out.append((start, size, m))
    return out


def disjoint_family(cands, tries=400, seed=0):
    """A large family of candidates whose range sets are pairwise disjoint: greedy over seeded random orders, the best kept."""
    g = np.random.default_rng(seed)
    best = []
    for _ in range(tries):
        used, fam = 0, []
        for i in g.permutation(len(cands)):
            if cands[i][2] & used == 0:
                used |= cands[i][2]
                fam.append(cands[i])
        if len(fam) > len(best):
            best = fam
    return best


def distinct_boxes(n, map_h, map_w):
    """n boxes (x0, y0, x1, y1 in pixels, stride 16) on a map of map_h x map_w cells with no RoIPool window in common.  Two
    boxes share a window only if they share a row range AND a column range: with row extents whose range sets are pairwise
    disjoint and column extents likewise, every (row extent, column extent) pair is a box, and two different boxes differ in
    an extent whose ranges are disjoint."""
    ys, xs = disjoint_family(axis_candidates(map_h)), disjoint_family(axis_candidates(map_w))
    if len(ys) * len(xs) < n:
        raise SystemExit(f"only {len(ys) * len(xs)} boxes with all-distinct windows found for a {map_h} x {map_w} map")
    boxes = [(16.0 * x0, 16.0 * y0, 16.0 * (x0 + xn - 1), 16.0 * (y0 + yn - 1)) for y0, yn, _ in ys for x0, xn, _ in xs]
    return np.asarray(boxes[:n], dtype=np.float32)


def timed(m, x, hw, steps, **kw):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prev = None
    for _ in range(steps):
        p = m.forward_async(x, hw, **kw)
        if prev is not None:
            prev.wait_raw()
        prev = p
    prev.wait_raw()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def windows(m, stage="head_windows"):
    return [int(v) for v in m.get_stage(stage).cpu().tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--boxes", type=int, default=300)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--option", choices=("head_dedupe", "head_dedupe_taps"), default="head_dedupe")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    taps = a.option == "head_dedupe_taps"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tap_dedupe_worst_case.json" if taps else "dedupe_worst_case.json")
    import torch
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    if not torch.cuda.is_available():
        raise SystemExit("dedupe_bench needs a GPU")
    N, H, W = a.batch, a.height, a.width
    cfg = vg_c4_config(post_nms_topk=300, detections=100)
    m = FRCNN(cfg, precision="fp16").load_state_dict(make_state_dict(cfg, seed=1234)).eval()
    x = torch.from_numpy(synthetic_images(N, H, W, seed=0xF2C)).cuda()
    hw = torch.tensor([[H, W]] * N)
    res = {"batch": N, "image": [H, W], "steps": a.steps, "pairs": a.pairs, "device": torch.cuda.get_device_name(0)}

    m.set_option("head_dedupe", 1)
    m.forward_async(x, hw).wait_raw()
    u = windows(m)
    bins = N * 300 * P * P
    res["bench_batch"] = {"bins": bins, "windows_per_chunk": u, "bins_per_window": round(bins / sum(u), 3)}
    if taps:
        v = windows(m, "head_neighbourhoods")
        res["bench_batch"].update({"neighbourhoods_per_chunk": v, "neighbourhoods_per_bin": round(sum(v) / bins, 4)})
    res["option"] = a.option

    res4 = m.get_stage("res4")
    boxes = distinct_boxes(a.boxes, res4.shape[1], res4.shape[2])
    props = torch.from_numpy(np.broadcast_to(boxes, (N,) + boxes.shape).copy()).cuda()
    runs = {0: [], 1: []}
    for dd in (0, 1):                   # warmed up as timed: overlapped forwards (the second working set is allocated here)
        m.set_option(a.option, dd)
        timed(m, x, hw, max(a.warmup, 2), proposals=props)
    u = windows(m)
    extra = {"neighbourhoods_per_chunk": windows(m, "head_neighbourhoods")} if taps else {}
    for _ in range(a.pairs):
        for dd in (0, 1):
            m.set_option(a.option, dd)
            runs[dd].append(round(timed(m, x, hw, a.steps, proposals=props), 3))
    bins = N * a.boxes * P * P
    res["all_distinct_given_boxes"] = {
        "boxes_per_image": a.boxes, "bins": bins, "windows_per_chunk": u, "bins_per_window": round(bins / sum(u), 4),
        "ms_per_batch_dedupe0": runs[0], "ms_per_batch_dedupe1": runs[1],      # (the option of --option at 0 and at 1)
        "median_cost_ms": round(float(np.median(runs[1]) - np.median(runs[0])), 3), **extra}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
