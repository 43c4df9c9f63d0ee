#!/usr/bin/env python3
"""ms per batch of detection with roi_outputs.selection = "detections" beside "class_max" and "per_class", on one GPU.

    python tools/detections_bench.py [--batch 32 --steps 10 --warmup 3 --precisions fp16,fp32 --score-thresh 0.05,0.2 --out FILE]

The C4 model (ResNet-101, calibrated head weights of seed 1234), R = 300 proposals, up to 100 outputs per image, on an
800x1333 synthetic batch resident in HBM -- the shape of tools/per_class_bench.py.  Per precision, in one process and on one
model: class-max (nms_thresh [0.3]) once, then for every score_thresh per-class (10 to 100 boxes) and detections (0 to 100
triples), both at nms_thresh 0.3.  The yardsticks of the detections mode are the class-max and per-class steps of the same
job: `over_class_max_ms` is what a mode costs on top of class-max.  Every mode is warmed up; a timed window is `steps`
forwards issued back to back (the next one enqueued before the previous one is waited for) between two device
synchronisations, read with a host clock.  One stage-timed forward per mode follows the window (HIP events; not part of the
window): `predictor_outputs` holds the selection -- in the two all-class modes the soft-max of every class and the bbox_pred
GEMM end at the stage event before it.  Prints one JSON line and writes it to --out.  Per-kernel times: run this tool under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(m, x, hw, steps, warmup):
    import torch
    for _ in range(warmup):
        m.forward_async(x, hw).wait_raw()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prev = None
    for _ in range(steps):
        p = m.forward_async(x, hw)
        if prev is not None:
            prev.wait_raw()
        prev = p
    blk = prev.wait_raw()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m.enable_stage_timing(True)
    m.forward_async(x, hw).wait_raw()
    stages = {k: round(v, 3) for k, v in m.stage_timing_ms().items()}
    m.enable_stage_timing(False)
    counts = blk["preds_per_image"].cpu()
    r = {"ms_per_batch": round(dt / steps * 1e3, 3), "images_per_s": round(x.shape[0] * steps / dt, 2), "stage_ms": stages,
         "outputs_per_image": {"min": int(counts.min()), "mean": round(float(counts.float().mean()), 2), "max": int(counts.max())}}
    if m.roi_outputs.selection == "detections":
        ns = m.get_stage("n_survivors").cpu()
        r["survivors_per_image"] = {"min": int(ns.min()), "mean": round(float(ns.float().mean()), 2), "max": int(ns.max())}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="fp16,fp32")
    ap.add_argument("--nms-thresh", type=float, default=0.3)
    ap.add_argument("--score-thresh", default="0.05,0.2")
    ap.add_argument("--max-detections", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detections_bench.json"))
    a = ap.parse_args()
    import torch
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    if not torch.cuda.is_available():
        raise SystemExit("detections_bench needs a GPU")
    N, H, W, R = a.batch, a.height, a.width, 300
    cfg = vg_c4_config(post_nms_topk=R, detections=a.max_detections)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(N, H, W, seed=1234)).cuda()
    hw = torch.tensor([[H, W]] * N)
    thresholds = [float(t) for t in a.score_thresh.split(",")]
    res = {"arch": "r101", "batch": N, "image": [H, W], "proposals": R, "classes": int(cfg.ROI_HEADS.NUM_CLASSES), "steps": a.steps,
           "warmup": a.warmup, "nms_thresh": a.nms_thresh, "score_thresh": thresholds, "max_detections": a.max_detections,
           "per_class_min_detections": 10, "device": torch.cuda.get_device_name(0), "modes": {}}
    for prec in a.precisions.split(","):
        m = FRCNN(cfg, precision=prec).load_state_dict(sd).eval()
        ro = m.roi_outputs
        ro.nms_thresh, ro.max_detections = [a.nms_thresh], a.max_detections
        ro.selection, ro.min_detections = "class_max", 10
        r = {"class_max": timed(m, x, hw, a.steps, a.warmup)}
        base = r["class_max"]["ms_per_batch"]
        for t in thresholds:
            ro.score_thresh = t
            for sel, lo in (("per_class", 10), ("detections", 0)):
                ro.selection, ro.min_detections = sel, lo
                e = timed(m, x, hw, a.steps, a.warmup)
                e["over_class_max_ms"] = round(e["ms_per_batch"] - base, 3)
                r[f"{sel}@{t:g}"] = e
        res["modes"][prec] = r
        del m
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
