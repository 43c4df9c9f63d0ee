"""-m gpu: option "forward_lanes" = 2 (the default): consecutive forwards of one handle in two working sets on two internal
streams (csrc/model.hip: fwd_route).  Every test compares, bit for bit, forwards that overlap on the device with the same
forwards run one at a time with forward_lanes = 1; the fused mean sums in exact fp64 and the dynamic tile tails change no
bit, so equality is the bar.  Shapes: the golden fixture's configuration (2 images 160x224, ResNet-101-C4, R = 30, D = 12)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import FRCNN, make_state_dict, synthetic_images, vg_c4_config   # noqa: E402

STAGES = ("res4", "feature_pooled", "obj_logits")


@pytest.fixture(scope="module")
def setup(golden_dir):
    g = np.load(os.path.join(golden_dir, "e2e_r101_small.npz"))
    n, h, w = g["nhw"].tolist()
    cfg = vg_c4_config(depth=int(g["depth"]), post_nms_topk=int(g["post_topk"]), detections=int(g["det"]))
    sd = make_state_dict(cfg, seed=int(g["weights_seed"]))
    shapes = torch.tensor(g["shapes"].tolist())
    xs = []
    for seed in (11, 12, 13, 14):                   # four different seeded image batches
        x = synthetic_images(n, h, w, seed=seed)
        for i, (hh, ww) in enumerate(shapes.tolist()):
            x[i, :, hh:, :] = 0
            x[i, :, :, ww:] = 0
        xs.append(torch.from_numpy(x).cuda())
    return cfg, sd, xs, shapes


@pytest.fixture(scope="module")
def models(setup):
    cfg, sd, _, _ = setup
    return {p: FRCNN(cfg, precision=p).load_state_dict(sd).eval() for p in ("fp16", "fp32")}


def block(p):
    return {k: v.clone() for k, v in p.wait_raw().items()}


def serial(m, calls):
    """Each call (kwargs of forward_async) alone, one lane: the reference bits."""
    m.set_option("forward_lanes", 1)
    out = [block(m.forward_async(**kw)) for kw in calls]
    stages = {s: m.get_stage(s).clone() for s in STAGES}
    m.set_option("forward_lanes", 2)
    return out, stages


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_four_overlapped_forwards_same_bits(setup, models, precision):
    """Four forward_async calls begun back to back and waited for in order, two lanes, against the same four alone."""
    _, _, xs, shapes = setup
    m = models[precision]
    calls = [dict(images=x, image_shapes=shapes) for x in xs]
    ref, ref_stages = serial(m, calls)
    lane0 = m.get_option("lane_forwards")
    pend = [m.forward_async(**kw) for kw in calls]
    assert m.get_option("lane_forwards") - lane0 >= 3 and m.get_option("working_sets") == 2     # they did run on the lanes
    for i, (p, r) in enumerate(zip(pend, ref)):
        same(block(p), r, i)
    for s in STAGES:                                # the stages are the last begun forward's, in its own working set
        assert torch.equal(m.get_stage(s), ref_stages[s]), s
    assert any(not torch.equal(ref[0]["roi_features"], r["roi_features"]) for r in ref[1:])


def test_interleaved_begin_and_wait(setup):
    """begin A, begin B, wait A, begin C, wait B, begin D, wait C, wait D with 1, 2, 1 and 2 images: C reuses A's working
    set while B runs.  On a fresh model set 0 only sees the one-image batches and set 1 the two-image ones, so each set
    is allocated once at its own size and nothing is freed here: growing a set beside a running forward is
    test_sets_regrow_beside_a_running_forward's."""
    cfg, sd, xs, shapes = setup
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    calls = [dict(images=x[:n], image_shapes=shapes[:n]) for x, n in zip(xs, (1, 2, 1, 2))]
    ref, _ = serial(FRCNN(cfg, precision="fp16").load_state_dict(sd).eval(), calls)
    a = m.forward_async(**calls[0])
    b = m.forward_async(**calls[1])
    got = [block(a)]
    c = m.forward_async(**calls[2])
    got.append(block(b))
    d = m.forward_async(**calls[3])
    got.append(block(c))
    got.append(block(d))
    for i, (o, r) in enumerate(zip(got, ref)):
        same(o, r, i)


@pytest.mark.parametrize("selection", ["class_max", "per_class"])
def test_sets_regrow_beside_a_running_forward(setup, selection):
    """A fresh model, 1, 1, 2 and 2 images over begin A, begin B, wait A, begin C, wait B, begin D, wait C, wait D.  A and B
    allocate the two sets at the one-image size; C needs a larger set 0 while B is in flight on set 1, and D a larger set
    1 while C is in flight on set 0: both go through the synchronize-and-free path of ensure_arena beside a running
    forward.  With selection = "per_class" the per-class arenas (sized by N * R) grow at the same two points."""
    cfg, sd, xs, shapes = setup

    def fresh():
        m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
        if selection == "per_class":
            m.roi_outputs.selection, m.roi_outputs.nms_thresh, m.roi_outputs.score_thresh = "per_class", [0.3], 0.05
        return m

    calls = [dict(images=x[:n], image_shapes=shapes[:n]) for x, n in zip(xs, (1, 1, 2, 2))]
    ref, _ = serial(fresh(), calls)
    m = fresh()
    a = m.forward_async(**calls[0])
    b = m.forward_async(**calls[1])
    assert m.get_option("working_sets") == 2
    got = [block(a)]
    c = m.forward_async(**calls[2])                 # set 0 grows, B still open
    got.append(block(b))
    d = m.forward_async(**calls[3])                 # set 1 grows, C still open
    assert m.get_option("lane_forwards") == 3       # A ran on the caller's stream (nothing was open), B, C and D on the lanes
    got.append(block(c))
    got.append(block(d))
    for i, (o, r) in enumerate(zip(got, ref)):
        same(o, r, (selection, i))
    assert not torch.equal(ref[2]["roi_features"][:1], ref[0]["roi_features"])


def test_other_entry_points_overlapped(setup, models):
    """Given boxes, ignorey and per-class selection: one overlapped pair each against the pair run serially; a given-boxes
    forward with no box at all (nothing to launch) between two ordinary forwards."""
    _, _, xs, shapes = setup
    m = models["fp16"]
    sc = torch.tensor([[1.25, 1.5], [2.0, 1.75]])
    props = [[np.array([[10.0, 12.0, 90.0, 100.0], [30.0, 5.0, 200.0, 150.0], [0.0, 0.0, 50.0, 40.0]], np.float32),
              np.array([[5.0, 5.0, 60.0, 70.0]], np.float32)],
             [np.array([[100.0, 20.0, 180.0, 120.0]], np.float32),
              np.array([[15.0, 25.0, 120.0, 130.0], [40.0, 40.0, 80.0, 90.0]], np.float32)]]
    bands = [[[[40.5, 60.0]], []], [[], [[20.0, 80.0], [10.0, 11.0]]]]
    pairs = {
        "given": [dict(images=xs[i], image_shapes=shapes, proposals=props[i]) for i in range(2)],
        "ignorey": [dict(images=xs[i], image_shapes=shapes, scales_yx=sc, ignorey=bands[i]) for i in range(2)],
        "plain": [dict(images=xs[i], image_shapes=shapes) for i in range(2)],
    }
    for name, calls in pairs.items():
        ref, _ = serial(m, calls)
        pend = [m.forward_async(**kw) for kw in calls]
        for i, (p, r) in enumerate(zip(pend, ref)):
            same(block(p), r, (name, i))

    ro = m.roi_outputs
    saved = (ro.selection, ro.nms_thresh, ro.score_thresh)
    try:
        ro.selection, ro.nms_thresh, ro.score_thresh = "per_class", [0.3], 0.05
        ref, _ = serial(m, pairs["plain"])
        pend = [m.forward_async(**kw) for kw in pairs["plain"]]
        for i, (p, r) in enumerate(zip(pend, ref)):
            same(block(p), r, ("per_class", i))
    finally:
        ro.selection, ro.nms_thresh, ro.score_thresh = saved

    empty = dict(images=xs[2], image_shapes=shapes, proposals=[np.zeros((0, 4), np.float32)] * 2)
    calls = [pairs["plain"][0], empty, pairs["plain"][1]]
    ref, _ = serial(m, calls)
    pend = [m.forward_async(**kw) for kw in calls]
    for i, (p, r) in enumerate(zip(pend, ref)):
        same(block(p), r, ("empty", i))
    assert ref[1]["preds_per_image"].tolist() == [0, 0]


def test_timers_force_one_lane(setup):
    """With the per-launch timers on, two overlapped forwards run on one lane: the launch counts are twice one forward's,
    no forward is enqueued on a lane's stream and no second working set is taken ("lane_forwards", "working_sets" of
    vk_get_option; the counts alone would not tell, the timer counts launches on any stream).  Timers off again, the
    same pair does use a lane."""
    cfg, sd, xs, shapes = setup
    m = FRCNN(cfg, precision="fp16").load_state_dict(sd).eval()
    m.enable_kernel_timing(True)
    m.kernel_timing(reset=True)
    m(xs[0], shapes)
    one = {k: v["launches"] for k, v in m.kernel_timing(reset=True).items()}
    assert sum(one.values()) > 0
    pend = [m.forward_async(xs[0], shapes), m.forward_async(xs[1], shapes)]
    for p in pend:
        p.wait_raw()
    two = {k: v["launches"] for k, v in m.kernel_timing(reset=True).items()}
    assert two == {k: 2 * n for k, n in one.items()}
    assert m.get_option("lane_forwards") == 0 and m.get_option("working_sets") == 1
    m.enable_kernel_timing(False)
    for p in [m.forward_async(xs[0], shapes), m.forward_async(xs[1], shapes)]:
        p.wait_raw()
    assert m.get_option("lane_forwards") == 1       # the second of the pair: the first began with nothing open


def test_callers_stream_orders_input_and_output(setup, models):
    """Forward inside a non-default stream, the input produced on that stream just before and an output consumed on it just
    after, with no synchronize in between: the bits of the synchronized run.  The input side is real: each input is the
    end of a chain of large matrix products on that stream (tens of milliseconds), so a lane that did not wait for the
    caller's stream at _begin would read a buffer not yet written.  The output side is a smoke test only: vk_forward_end
    waits on the host for the ticket before it returns, so the stream-side wait it also enqueues cannot fail here."""
    _, _, xs, shapes = setup
    m = models["fp16"]
    ref, _ = serial(m, [dict(images=xs[0] * 0.5, image_shapes=shapes), dict(images=xs[1] * 0.5, image_shapes=shapes)])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pend, sums = [], []
        for x in xs[:2]:
            big = torch.full((4096, 4096), 1e-4, device=x.device)
            for _ in range(12):
                big = big @ big                                     # (entries shrink towards 0: finite)
            late = x * 0.5 + big.sum() * 0.0                        # bit-equal to x * 0.5, ready only after the chain
            pend.append(m.forward_async(late, shapes))              # enqueued on s; the forward reads it
        for p in pend:
            blk = p.wait_raw()
            sums.append((blk, blk["roi_features"] * 2.0))           # consumed on s behind the lane's completion event
    torch.cuda.synchronize()
    for i, ((blk, twice), r) in enumerate(zip(sums, ref)):
        same({k: v for k, v in blk.items()}, r, i)
        assert torch.equal(twice, r["roi_features"] * 2.0), i
