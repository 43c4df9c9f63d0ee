#!/usr/bin/env python3
"""Images/s of region features for caller-supplied boxes (FRCNN.forward(proposals=...)) beside detection, on one GPU.

    python tools/given_boxes_bench.py [--arch r101|r101-fpn --batch 32 --steps 10 --warmup 3 --ks 10,36,100 --out FILE]

--arch r101 (default): the C4 model, detection with R = 300 proposals; --arch r101-fpn: the FPN detector (fpn_config()),
detection with R = 1000, as `bench.py --arch r101-fpn`.  Per precision (fp16, fp32), in one process: detection (up to
100 detections, as bench.py), then given boxes with K boxes per image for each K, on the same 800x1333 synthetic batch resident in HBM.  Every shape is warmed
up; a timed window is `steps` forwards issued back to back (the next one enqueued before the previous one is waited for,
as the extraction pipeline runs them) between two device synchronisations, read with a host clock.  One stage-timed
forward per mode follows the window (HIP events; not part of the images/s).  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_boxes(N, K, H, W, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, K, generator=g) * (W - 64)
    y0 = torch.rand(N, K, generator=g) * (H - 64)
    w = 16 + torch.rand(N, K, generator=g) * (W / 2)
    h = 16 + torch.rand(N, K, generator=g) * (H / 2)
    return torch.stack([x0, y0, x0 + w, y0 + h], -1)


def timed(m, x, hw, steps, warmup, proposals=None):
    import torch
    kw = {} if proposals is None else {"proposals": proposals}
    for _ in range(warmup):
        m.forward_async(x, hw, **kw).wait_raw()
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
    dt = time.perf_counter() - t0
    m.enable_stage_timing(True)
    m.forward_async(x, hw, **kw).wait_raw()
    stages = {k: round(v, 3) for k, v in m.stage_timing_ms().items()}
    m.enable_stage_timing(False)
    return {"images_per_s": round(x.shape[0] * steps / dt, 2), "ms_per_batch": round(dt / steps * 1e3, 3), "stage_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="r101", choices=["r101", "r101-fpn"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="10,36,100")
    ap.add_argument("--precisions", default="fp16,fp32")
    ap.add_argument("--out", default=None, help="default profiles/given_boxes_bench.json (r101), given_boxes_bench_fpn.json (r101-fpn)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "given_boxes_bench.json" if a.arch == "r101" else "given_boxes_bench_fpn.json")
    import torch
    from vltk_amd import FRCNN, fpn_config, make_state_dict, synthetic_images, vg_c4_config
    if not torch.cuda.is_available():
        raise SystemExit("given_boxes_bench needs a GPU")
    N, H, W = a.batch, a.height, a.width
    R = 1000 if a.arch == "r101-fpn" else 300
    cfg = fpn_config(post_nms_topk=R, detections=100) if a.arch == "r101-fpn" else vg_c4_config(post_nms_topk=R, detections=100)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(N, H, W, seed=1234)).cuda()
    hw = torch.tensor([[H, W]] * N)
    ks = [int(k) for k in a.ks.split(",")]
    res = {"arch": a.arch, "batch": N, "image": [H, W], "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "modes": {}}
    for prec in a.precisions.split(","):
        m = FRCNN(cfg, precision=prec).load_state_dict(sd).eval()
        r = {f"detection_R{R}": timed(m, x, hw, a.steps, a.warmup)}
        for k in ks:
            props = random_boxes(N, k, H, W, seed=k).cuda()
            r[f"given_K{k}"] = timed(m, x, hw, a.steps, a.warmup, props)
        res["modes"][prec] = r
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
