#!/usr/bin/env python3
"""The C4 model's RoIAlign box pooler (ROI_BOX_HEAD.POOLER_TYPE) on one GPU: one job, one JSON file.

    python tools/roi_align_bench.py [--batch 32 --rounds 12 --steps 5 --pairs 3 --parent-tree DIR --out FILE]

Stage level (fp16): the res4 map and the proposal boxes of a real detection forward of bench.py's model (ResNet-101-C4,
weights of seed 1234, synthetic_images(seed=0xF2C), 32 x 800 x 1333, R = 300: 9600 RoIs) pooled to [9600, 14, 14, 1024] by
  (a) vk_roi_pool          (b) vk_roi_align on one level (the pyramid kernel: what the handle would run without the C4 kernel)
  (c) vk_roi_align_c4, an LDS-staged candidate kernel, where the library under test exports it (the shipped one does not: it
      was measured with this tool and lost; profiles/roi_align_c4_bench.json keeps its numbers)
alternating in one process, `rounds` times each, every launch between two HIP events; (b) runs twice per round and the
difference of its two medians is the repeat spread.  (b) and (c) at sampling ratio 0 and 2, aligned.  Also the share of the
RoIs that vk_roi_align_c4_staged says took the staged form.  Acceptance: (c)'s median below (b)'s by more than the spread.

Whole step: four models alternating -- the default (RoIPool, head_dedupe 1), RoIPool with head_dedupe 0 (the like-for-like
yardstick: RoIAlign cannot dedupe), ROIAlignV2 at sampling ratio 0 and 2 -- `steps` forwards issued back to back per window,
`pairs` windows each.  With --parent-tree (a built checkout of the previous commit) the default path of both builds is timed
the same way in child processes, alternating.  --default-only / --tree are what those children run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SCALE = 14, 1.0 / 16


def timed(m, x, hw, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prev = None
    for _ in range(steps):
        p = m.forward_async(x, hw)
        if prev is not None:
            prev.wait_raw()
        prev = p
    prev.wait_raw()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "n": len(v)}


def default_only(a):
    """One process, the default model of the tree it was started on: `pairs` windows of `steps` forwards."""
    import torch
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    cfg = vg_c4_config(post_nms_topk=300, detections=100)
    m = FRCNN(cfg, precision="fp16").load_state_dict(make_state_dict(cfg, seed=1234)).eval()
    x = torch.from_numpy(synthetic_images(a.batch, a.height, a.width, seed=0xF2C)).cuda()
    hw = torch.tensor([[a.height, a.width]] * a.batch)
    timed(m, x, hw, max(a.warmup, 2))
    print(json.dumps({"ms_per_batch": [round(timed(m, x, hw, a.steps), 3) for _ in range(a.pairs)]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the previous commit: its default path is timed too")
    ap.add_argument("--stage-only", action="store_true")
    ap.add_argument("--default-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "roi_align_c4_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("roi_align_bench needs a GPU")
    if a.default_only:
        return default_only(a)
    from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config
    from vltk_amd import _lib as L
    N, H, W = a.batch, a.height, a.width
    kw = dict(post_nms_topk=300, detections=100)
    cfg = vg_c4_config(**kw)
    sd = make_state_dict(cfg, seed=1234)
    x = torch.from_numpy(synthetic_images(N, H, W, seed=0xF2C)).cuda()
    hw = torch.tensor([[H, W]] * N)
    res = {"batch": N, "image": [H, W], "device": torch.cuda.get_device_name(0), "rule": "parity unpinned for the rule",
           "lds_kb": os.environ.get("VK_ROIALIGN_C4_LDS_KB", "default"), "lanes": os.environ.get("VK_ROIALIGN_C4_LANES", "default")}

    # ---- stage level ----
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    m.forward_async(x, hw).wait_raw()
    res4 = m.get_stage("res4").clone()
    boxes = m.get_stage("proposal_boxes").clone()                         # [N, R, 4]; rows beyond an image's count are zero
    counts = m.get_stage("proposal_counts").cpu().tolist()
    del m
    R = boxes.shape[1]
    K, Cc = N * R, res4.shape[3]
    rois = torch.cat([torch.arange(N, device="cuda", dtype=torch.float32).repeat_interleave(R)[:, None], boxes.reshape(K, 4)], 1).contiguous()
    out = torch.empty((K, P, P, Cc), dtype=torch.float16, device="cuda")
    lib, s = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Hf, Wf = res4.shape[1], res4.shape[2]
    maps, Hs, Ws, sc = (C.c_void_p * 1)(res4.data_ptr()), (C.c_int32 * 1)(Hf), (C.c_int32 * 1)(Wf), (C.c_float * 1)(SCALE)
    fp, rp, op = C.c_void_p(res4.data_ptr()), C.c_void_p(rois.data_ptr()), C.c_void_p(out.data_ptr())

    def pool():
        L.call("vk_roi_pool", fp, N, Hf, Wf, Cc, rp, K, SCALE, P, op, L.VK_F16, s)

    def pyramid(sr):
        return lambda: L.call("vk_roi_align", maps, Hs, Ws, sc, 1, N, Cc, rp, None, K, P, sr, 1, op, L.VK_F16, s)

    def c4(sr):
        return lambda: L.check(lib.vk_roi_align_c4(fp, N, Hf, Wf, Cc, rp, K, C.c_float(SCALE), P, sr, 1, op, L.VK_F16, s))

    has_c4 = hasattr(lib, "vk_roi_align_c4")          # the candidate kernel: a build that carries it (none shipped)
    launchers = [("a_roi_pool", pool)]
    for sr in (0, 2):
        launchers += [(f"b_roi_align_sr{sr}", pyramid(sr))] + ([(f"c_roi_align_c4_sr{sr}", c4(sr))] if has_c4 else [])
        launchers += [(f"b_roi_align_sr{sr}_repeat", pyramid(sr))]
    ms = {k: [] for k, _ in launchers}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(a.rounds + 2):                                       # two warm-up rounds
        for name, fn in launchers:
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                ms[name].append(e0.elapsed_time(e1))
    stage = {k: stats(v) for k, v in ms.items()}
    rois_h = rois.cpu().numpy()
    for sr in (0, 2) if has_c4 else ():
        lib.vk_roi_align_c4_staged.argtypes = [C.c_float] * 4 + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 3
        st = [lib.vk_roi_align_c4_staged(float(r[1]), float(r[2]), float(r[3]), float(r[4]), Hf, Wf, Cc, P, SCALE, sr, 1, L.VK_F16)
              for r in rois_h]
        b, b2, c = (stage[f"b_roi_align_sr{sr}"]["median_ms"], stage[f"b_roi_align_sr{sr}_repeat"]["median_ms"],
                    stage[f"c_roi_align_c4_sr{sr}"]["median_ms"])
        stage[f"verdict_sr{sr}"] = {"staged_share": round(float(np.mean(st)), 4), "b_repeat_spread_ms": round(abs(b - b2), 4),
                                    "c_below_b_ms": round(min(b, b2) - c, 4), "accepted": bool(min(b, b2) - c > abs(b - b2))}
    res["stage_fp16"] = dict(rois=K, map=[N, Hf, Wf, Cc], proposals_per_image_min=int(min(counts)), rounds=a.rounds, **stage)
    del out, res4

    # ---- whole step ----
    if not a.stage_only:
        def align_cfg(sr):
            return vg_c4_config(overrides=[("roi_box_head", "pooler_type", "ROIAlignV2"), ("roi_box_head", "pooler_sampling_ratio", sr)], **kw)
        models = {"default": FRCNN(cfg, precision="fp16").load_state_dict(sd).eval(),
                  "roipool_head_dedupe0": FRCNN(cfg, precision="fp16").load_state_dict(sd).eval(),
                  "roialignv2_sr0": FRCNN(align_cfg(0), precision="fp16").load_state_dict(sd).eval(),
                  "roialignv2_sr2": FRCNN(align_cfg(2), precision="fp16").load_state_dict(sd).eval()}
        models["roipool_head_dedupe0"].set_option("head_dedupe", 0)
        runs = {k: [] for k in models}
        for mm in models.values():
            timed(mm, x, hw, max(a.warmup, 2))
        for _ in range(a.pairs):
            for k, mm in models.items():
                runs[k].append(round(timed(mm, x, hw, a.steps), 3))
        res["whole_step_ms_per_batch"] = dict(steps=a.steps, **{k: {"runs": v, "median": round(float(np.median(v)), 3)} for k, v in runs.items()})
        del models
        if a.parent_tree:
            torch.cuda.empty_cache()
            got = {"parent": [], "this": []}
            for _ in range(2):
                for who, tree in (("parent", a.parent_tree), ("this", HERE)):
                    cmd = [sys.executable, os.path.abspath(__file__), "--default-only", "--tree", tree, "--batch", str(N), "--height", str(H),
                           "--width", str(W), "--steps", str(a.steps), "--pairs", str(a.pairs), "--warmup", str(a.warmup)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, check=True)
                    got[who] += json.loads(r.stdout.strip().splitlines()[-1])["ms_per_batch"]
            res["default_path_parent_vs_this_ms_per_batch"] = {
                k: {"runs": v, "median": round(float(np.median(v)), 3), "spread": round(float(np.max(v) - np.min(v)), 3)} for k, v in got.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
