#!/usr/bin/env python3
"""Images/s of grid features (FRCNN.forward(grid=(Gh, Gw))) beside detection, on one GPU.

    python tools/grid_bench.py [--batch 32 --grids 7x7,8x8,10x10 --repeats 3 --out FILE]

Per precision (fp16, fp32), in one process: detection (R = 300 proposals, up to 100 detections, as bench.py) and one grid
forward per grid, on the same 800x1333 synthetic batch resident in HBM.  Every mode is warmed up first.  A timed window is a
run of forwards issued back to back (the next one enqueued before the previous one is waited for, as the extraction
pipeline runs them) between two device synchronisations, read with a host clock, long enough to last about a second in
fp16 (--seconds); the windows of the modes alternate (detection, grid, grid, grid, detection, ...) `repeats` times, and the
median window is reported with the lowest and highest beside it.  One stage-timed forward per mode follows (HIP events; not
part of the images/s); in a grid forward "roi_heads" is Res5 over the map, the pooling and the predictor.  The file also
records which kernel every Res5 layer of the map runs on (vk_conv_route) and bench.py's recorded detection step
(profiles/r03_i_bench.json) beside this job's.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("generic", "ring", "duo", "ws", "gemm4", "panel", "blk")      # VK_ROUTE_* of include/vltk_hip.h, by value


def window(m, x, hw, steps, kw):
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


def res5_routes(N, Hf, Wf, dt):
    """The kernel of every Res5 convolution over an [N, Hf, Wf] res4 map of ResNet-101 (stride 1, dilation 2), by name."""
    from vltk_amd import _lib as L
    lib = L.load()

    def route(cin, cout, k=1, cin2=0, res=0):
        d = 2 if k == 3 else 1
        r = lib.vk_conv_route(N, Hf, Wf, cin, cin2, res, 0, cout, cout, k, k, 1, d if k == 3 else 0, d, 1, 1, dt, dt)
        return ROUTES[r] if r >= 0 else f"refused ({-r})"
    out = {}
    for b in range(3):
        cin = 1024 if b == 0 else 2048
        out[f"res5.{b}.conv1"] = route(cin, 512)
        out[f"res5.{b}.conv2"] = route(512, 512, k=3)
        if b == 0 and lib.vk_fuse_shortcut(512, cin, 2048, 1, dt) == 1:
            out[f"res5.{b}.conv3"] = route(512, 2048, cin2=cin) + " (with the projection shortcut)"
        else:
            if b == 0:
                out[f"res5.{b}.shortcut"] = route(cin, 2048)
            out[f"res5.{b}.conv3"] = route(512, 2048, res=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--grids", default="7x7,8x8,10x10")
    ap.add_argument("--precisions", default="fp16,fp32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="length a window aims at (at least 3 forwards, at most 64)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_bench.json"))
    a = ap.parse_args()
    import torch
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    from vltk_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("grid_bench needs a GPU")
    N, H, W = a.batch, a.height, a.width
    R = 300
    cfg = vg_c4_config(post_nms_topk=R, detections=100)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(N, H, W, seed=1234)).cuda()
    hw = torch.tensor([[H, W]] * N)
    grids = [tuple(int(v) for v in g.split("x")) for g in a.grids.split(",")]
    modes = [(f"detection_R{R}", {})] + [(f"grid_{gh}x{gw}", {"grid": (gh, gw)}) for gh, gw in grids]
    res = {"batch": N, "image": [H, W], "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "modes": {},
           "res5_routes": {}}
    for prec in a.precisions.split(","):
        m = FRCNN(cfg, precision=prec).load_state_dict(sd).eval()
        steps, times = {}, {k: [] for k, _ in modes}
        for k, kw in modes:                                   # warm-up, and the window length from one timed forward
            for _ in range(a.warmup):
                m.forward_async(x, hw, **kw).wait_raw()
            one = window(m, x, hw, 1, kw)
            steps[k] = int(min(64, max(3, round(a.seconds * 1e3 / one))))
        for _ in range(a.repeats):
            for k, kw in modes:
                times[k].append(window(m, x, hw, steps[k], kw))
        r = {}
        for k, kw in modes:
            m.enable_stage_timing(True)
            m.forward_async(x, hw, **kw).wait_raw()
            stages = {s: round(v, 3) for s, v in m.stage_timing_ms().items()}
            m.enable_stage_timing(False)
            med = statistics.median(times[k])
            r[k] = {"images_per_s": round(N / med * 1e3, 2), "ms_per_batch": round(med, 3), "ms_per_batch_min": round(min(times[k]), 3),
                    "ms_per_batch_max": round(max(times[k]), 3), "steps_per_window": steps[k], "stage_ms": stages}
            if "grid" in kw:
                ppi = m.forward_padded()["preds_per_image"].tolist()
                assert ppi == [kw["grid"][0] * kw["grid"][1]] * N, ppi
        res["modes"][prec] = r
        st = m.get_stage("res4").shape
        res["res5_routes"][prec] = res5_routes(N, int(st[1]), int(st[2]), L.VK_F16 if prec == "fp16" else L.VK_F32)
        res["res4_map"] = [int(v) for v in st]
        del m
        torch.cuda.empty_cache()
    base = os.path.join(ROOT, "profiles", "r03_i_bench.json")
    if os.path.exists(base) and "fp16" in res["modes"]:
        with open(base) as f:
            b = json.load(f)
        mine = res["modes"]["fp16"][f"detection_R{R}"]["ms_per_batch"]
        res["detection_vs_recorded"] = {"recorded": "profiles/r03_i_bench.json", "recorded_ms_per_step": b["ms_per_step"],
                                        "this_job_ms_per_step": mine, "ratio": round(mine / b["ms_per_step"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
