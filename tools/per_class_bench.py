#!/usr/bin/env python3
"""Images/s of detection with roi_outputs.selection = "per_class" beside the default "class_max", on one GPU.

    python tools/per_class_bench.py [--batch 32 --steps 10 --warmup 3 --precisions fp16,fp32 --out FILE]

The C4 model (ResNet-101, calibrated head weights of seed 1234), R = 300 proposals, up to 100 detections, on an 800x1333
synthetic batch resident in HBM.  Per precision, in one process and on one model: class-max (nms_thresh [0.3]; the count
is what NMS leaves, up to 100), then per-class (nms_thresh 0.3, score_thresh 0.2, 10 to 100 boxes).  Every mode is warmed
up; a timed window is `steps` forwards issued back to back (the next one enqueued before the previous one is waited
for) between two device synchronisations, read with a host clock.  One stage-timed forward per mode follows the window
(HIP events; not part of the images/s): `predictor_outputs` holds everything after the class / attribute branches -- in the
per-class mode the all-class soft-max and bbox_pred GEMM end at the stage event before it, the NMS and the finalize are it.
"floors" in the result is shape arithmetic, not a measurement: the bytes each new kernel has to move (every input read once,
every output written once) at the 6.3 TB/s the HBM sustains, and bbox_pred's FLOPs at the fp32 MFMA
peak.  Writes one JSON file and prints it.  Per-kernel times: run this tool under `rocprofv3 --kernel-trace --stats`
(DESIGN.md section 15 sets such a run's kernel table beside the floors).
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
    return {"images_per_s": round(x.shape[0] * steps / dt, 2), "ms_per_batch": round(dt / steps * 1e3, 3), "stage_ms": stages,
            "detections_per_image": {"min": int(counts.min()), "mean": round(float(counts.float().mean()), 2), "max": int(counts.max())}}


HBM_BYTES_PER_S, FP32_MFMA_FLOPS = 6.3e12, 157.3e12


def floors(N, R, C, F, D):
    """Per new kernel: bytes (inputs once + outputs once) and the microseconds they take at HBM_BYTES_PER_S."""
    K, ld = N * R, (C + 1 + 7) // 8 * 8
    b = {"class_probs_kernel": 2 * K * ld * 4,                                   # logits in, probabilities out
         "bbox_pred_gemm": (K * F + 4 * C * F + K * 4 * C) * 4,                  # features, weights, all-class deltas (fp32)
         "per_class_nms_kernel": (K * ld + K * 4 * C + K * 4 + K * 2) * 4,       # scores, deltas, proposals, best words
         "per_class_final_kernel": (K * 8 + K * 4 + 2 * N * D * F * 4)}          # best words, max_conf, the feature gather
    out = {k: {"bytes": int(v), "hbm_floor_us": round(v / HBM_BYTES_PER_S * 1e6, 1)} for k, v in b.items()}
    flop = 2 * K * F * 4 * C
    out["bbox_pred_gemm"].update(gflop=round(flop / 1e9, 1), mfma_floor_us=round(flop / FP32_MFMA_FLOPS * 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="fp16,fp32")
    ap.add_argument("--nms-thresh", type=float, default=0.3)
    ap.add_argument("--score-thresh", type=float, default=0.2)
    ap.add_argument("--min-detections", type=int, default=10)
    ap.add_argument("--max-detections", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_class_bench.json"))
    a = ap.parse_args()
    import torch
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    if not torch.cuda.is_available():
        raise SystemExit("per_class_bench needs a GPU")
    N, H, W, R = a.batch, a.height, a.width, 300
    cfg = vg_c4_config(post_nms_topk=R, detections=a.max_detections)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(N, H, W, seed=1234)).cuda()
    hw = torch.tensor([[H, W]] * N)
    res = {"arch": "r101", "batch": N, "image": [H, W], "proposals": R, "classes": int(cfg.ROI_HEADS.NUM_CLASSES), "steps": a.steps,
           "warmup": a.warmup, "nms_thresh": a.nms_thresh, "score_thresh": a.score_thresh,
           "detections": [a.min_detections, a.max_detections], "device": torch.cuda.get_device_name(0),
           "floors": floors(N, R, int(cfg.ROI_HEADS.NUM_CLASSES), int(cfg.RESNETS.RES2_OUT_CHANNELS) * 8, a.max_detections), "modes": {}}
    for prec in a.precisions.split(","):
        m = FRCNN(cfg, precision=prec).load_state_dict(sd).eval()
        ro = m.roi_outputs
        ro.nms_thresh, ro.score_thresh = [a.nms_thresh], a.score_thresh
        ro.min_detections, ro.max_detections = a.min_detections, a.max_detections
        r = {}
        for sel in ("class_max", "per_class"):
            ro.selection = sel
            r[sel] = timed(m, x, hw, a.steps, a.warmup)
        r["per_class_over_class_max"] = round(r["per_class"]["ms_per_batch"] / r["class_max"]["ms_per_batch"], 4)
        res["modes"][prec] = r
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
