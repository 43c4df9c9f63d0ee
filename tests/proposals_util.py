"""Inputs, call helpers and a second reference for the proposal stage (csrc/rpn.hip): used by test_proposals_host.py (CPU),
test_gpu_proposals_edge.py, and by the older stage tests (test_gpu_stages.py, test_gpu_fpn.py) for their calls.

What makes the selection visible: with nms_thresh = 2.0 (an IoU never exceeds 1) and post_nms_topk = pre_nms_topk the entry
points return every selected candidate that passed the size filter, in rank order -- every slot of the radix select, the
compaction, the sort, the merge and the valid flags, through the public C ABI.

What makes it exact: deltas with dw = dh = 0 (exp(0) == 1 everywhere) and dx, dy = k/64, bbox weights that are powers of two,
cell anchors with integer or half-integer corners and sides <= 512, a power-of-two stride, offset 0 or 0.5, integer image
sizes.  Every intermediate of the decode then carries at most 7 fractional bits at magnitudes below 2^16, so boxes are
BIT-equal to the oracle's, and a bit-equal box says which anchor was taken where equal logits of a tie class cannot.

The second reference (`select_restatement`, `greedy_nms`) is plain numpy / Python written from the description of the
reference (sort descending, stable; first K; decode; clip; strict size filter; greedy suppression), and shares no code with
the oracle nor shape with the kernels."""
import ctypes as C
import zlib

import numpy as np
import torch

from oracle import frcnn_oracle as orc
from oracle.frcnn_oracle import FRCNNOracle
from vltk_amd import _lib as L
from vltk_amd.config import Config, vg_c4_config_dict

import gpu_util as G

SCALE_CLAMP = np.float32(np.log(1000.0 / 16.0))
NO_SUPPRESSION = 2.0                                # nms_thresh above every IoU
NOOP_BAND = [[-1e9, -9e8]]                          # an ignorey band above every box: drops nothing, trims nothing


def rng_for(*parts):
    """A generator keyed by the case's own description (stable from run to run and across parametrisations)."""
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(parts).encode())))


# ---- logit regimes: (rng, HWA) -> f32 [HWA] in flat (y, x, a) order; none holds a NaN -----------------------------------------
def _all_equal(g, n):
    return np.full(n, 0.75, np.float32)


def _two_values(g, n):
    v = np.full(n, -1.5, np.float32)
    v[g.permutation(n)[: min(n // 3, 40)]] = 2.25         # the higher value on few anchors: K > 40 cuts the lower class
    return v


def _quantised(g, n):
    return (np.round(g.standard_normal(n) * 2) / 2).astype(np.float32)


def _low_byte(g, n):
    return (1.0 + g.integers(0, 256, n) * 2.0 ** -23).astype(np.float32)     # keys differ in the last radix byte only


def _second_byte(g, n):
    return (1.0 + g.integers(0, 256, n) * 2.0 ** -15).astype(np.float32)


def _signs_specials(g, n):
    pool = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, 1.0, -1.0, 0.5, -0.5, 3.0e38, -3.0e38], np.float32)
    v = pool[g.integers(0, len(pool), n)]
    plain = g.random(n) < 0.3
    v[plain] = g.standard_normal(int(plain.sum())).astype(np.float32)
    return v


def _all_negative(g, n):
    return (-0.5 - np.round(np.abs(g.standard_normal(n)) * 8) / 8).astype(np.float32)


def _continuous(g, n):
    return g.standard_normal(n).astype(np.float32)


REGIMES = {"all_equal": _all_equal, "two_values": _two_values, "quantised": _quantised, "low_byte": _low_byte,
           "second_byte": _second_byte, "signs_specials": _signs_specials, "all_negative": _all_negative,
           "continuous": _continuous}
TIE_REGIMES = ("all_equal", "two_values", "quantised", "low_byte")      # a threshold tie class is what they are for


def regime_logits(name, n, *key):
    v = REGIMES[name](rng_for(name, n, *key), n)
    assert v.dtype == np.float32 and v.shape == (n,) and not np.isnan(v).any()
    return v


# ---- exact geometry ---------------------------------------------------------------------------------------------------------
_SIDES_W = [8, 16, 24, 32, 48, 64, 96, 128, 13, 21, 37, 5, 3, 256, 511]
_SIDES_H = [16, 8, 32, 24, 64, 48, 128, 96, 21, 13, 5, 37, 3, 500, 255]


def exact_cells(A, sides=None):
    """[A, 4] cell anchors centred on 0 with integer sides (odd sides give half-integer corners), all <= 512."""
    sides = list(zip(_SIDES_W, _SIDES_H))[:A] if sides is None else sides
    assert len(sides) == A
    return np.array([[-w / 2, -h / 2, w / 2, h / 2] for w, h in sides], np.float32)


def exact_deltas(g, N, Hf, Wf, A):
    """[N, Hf, Wf, A, 4] f32: dx, dy = k/64 with integer |k| <= 8, dw = dh = 0."""
    d = np.zeros((N, Hf, Wf, A, 4), np.float32)
    d[..., :2] = g.integers(-8, 9, (N, Hf, Wf, A, 2)) / 64.0
    return d


def to_oracle_layout(logits, deltas):
    """logits [N, Hf, Wf, A], deltas [N, Hf, Wf, A, 4] (the kernels' order) -> obj [N, A, Hf, Wf], dlt [N, 4A, Hf, Wf] tensors."""
    N, Hf, Wf, A = logits.shape
    obj = torch.from_numpy(np.ascontiguousarray(logits.transpose(0, 3, 1, 2)))
    dlt = torch.from_numpy(np.ascontiguousarray(deltas.reshape(N, Hf, Wf, 4 * A).transpose(0, 3, 1, 2)))
    return obj, dlt


def grid_anchors_np(Hf, Wf, cell, stride, offset=0.0):
    """[Hf*Wf*A, 4] f32 in flat (y, x, a) order: shift (offset + x) * stride plus the cell anchor."""
    sx = ((offset + np.arange(Wf, dtype=np.float64)) * stride).astype(np.float32)
    sy = ((offset + np.arange(Hf, dtype=np.float64)) * stride).astype(np.float32)
    yy, xx = np.meshgrid(sy, sx, indexing="ij")
    sh = np.stack([xx, yy, xx, yy], -1).reshape(-1, 1, 4)
    return (sh + np.asarray(cell, np.float32).reshape(1, -1, 4)).reshape(-1, 4).astype(np.float32)


# ---- the second reference ---------------------------------------------------------------------------------------------------
def stable_desc_order(v):
    """Indices of v by value descending, equal values (-0.0 == +0.0 among them) by index ascending."""
    v = np.asarray(v, np.float32) + np.float32(0.0)           # -0.0 + 0.0 == +0.0
    return np.lexsort((np.arange(len(v)), -v.astype(np.float64)))


def decode_np(anc, d, weights):
    """Box2BoxTransform.apply_deltas in f32, one operation at a time in the reference's order."""
    f = np.float32
    anc, d = anc.astype(f), d.astype(f)
    w = anc[:, 2] - anc[:, 0]
    h = anc[:, 3] - anc[:, 1]
    cx = anc[:, 0] + f(0.5) * w
    cy = anc[:, 1] + f(0.5) * h
    dx, dy = d[:, 0] / f(weights[0]), d[:, 1] / f(weights[1])
    dw = np.minimum(d[:, 2] / f(weights[2]), SCALE_CLAMP)
    dh = np.minimum(d[:, 3] / f(weights[3]), SCALE_CLAMP)
    pcx = dx * w + cx
    pcy = dy * h + cy
    pw = np.exp(dw).astype(f) * w
    ph = np.exp(dh).astype(f) * h
    out = np.stack([pcx - f(0.5) * pw, pcy - f(0.5) * ph, pcx + f(0.5) * pw, pcy + f(0.5) * ph], 1)
    assert out.dtype == f
    return out


def select_restatement(logits, deltas, anchors, K, weights, hw, min_size):
    """One image, one level.  logits [HWA], deltas [HWA, 4], anchors [HWA, 4] in flat order -> the K best candidates in rank
    order: (flat indices, clipped boxes [K, 4], logits [K], valid [K])."""
    idx = stable_desc_order(logits)[:K]
    b = decode_np(anchors[idx], deltas[idx], weights)
    h, w = np.float32(hw[0]), np.float32(hw[1])
    b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], np.float32(0)), w)
    b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], np.float32(0)), h)
    valid = ((b[:, 2] - b[:, 0]) > np.float32(min_size)) & ((b[:, 3] - b[:, 1]) > np.float32(min_size))
    return idx, b, np.asarray(logits, np.float32)[idx], valid


def greedy_nms(boxes, scores, thr):
    """Greedy NMS, O(n^2): boxes in stable descending score order; a box is suppressed by an earlier kept box when their IoU,
    computed in f32 and widened to double, is > thr.  A 0/0 IoU is NaN and suppresses nothing.  Returns kept indices."""
    b = np.asarray(boxes, np.float32)
    order = stable_desc_order(scores)
    b = b[order]
    n = len(b)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(n, bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if dead[i]:
                continue
            keep.append(int(order[i]))
            r = b[i + 1:]
            iw = np.maximum(np.float32(0), np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]))
            ih = np.maximum(np.float32(0), np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]))
            inter = iw * ih
            iou = inter / (area[i] + area[i + 1:] - inter)
            assert iou.dtype == np.float32
            dead[i + 1:] |= iou.astype(np.float64) > float(thr)
    return np.asarray(keep, np.int64)


def iou_f32(a, b):
    """IoU of two boxes, every operation in f32 (0/0 gives NaN)."""
    f = np.float32
    a, b = np.asarray(a, f), np.asarray(b, f)
    iw = max(f(0), min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(f(0), min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    with np.errstate(invalid="ignore"):
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def tie_stats(flat_logits, K):
    """(size of the class of logits equal to the K-th best, how many of it the selection takes), on the oracle's own order."""
    v = np.asarray(flat_logits, np.float32)
    order = orc.argsort_desc(torch.from_numpy(v)).numpy()
    t = v[order[K - 1]]
    return int((v == t).sum()), int(K - (v > t).sum())


# ---- hand-built NMS sets ------------------------------------------------------------------------------------------------------
def chain_boxes(n):
    """b_i = [i, 0, i+3, 1]: neighbours overlap 2 of 4 (IoU exactly 1/2), next-neighbours 1 of 5, the rest not at all."""
    i = np.arange(n, dtype=np.float32)
    return np.stack([i, np.zeros(n, np.float32), i + 3, np.ones(n, np.float32)], 1)


def chain_scores(n):
    return (n - np.arange(n)).astype(np.float32)               # descending with i


THIRD_BOXES = np.array([[0, 0, 2, 1], [1, 0, 3, 1]], np.float32)                 # IoU = f32(1/3)
THIRD_AS_F32 = float(np.float32(1) / np.float32(3))                              # < 1/3 < the next f32
DEGENERATE_BOXES = np.array([[5, 5, 5, 9], [5, 5, 5, 9], [0, 0, 4, 4], [0, 0, 4, 4], [1, 1, 1, 1]], np.float32)
DEGENERATE_SCORES = np.array([5, 4, 3, 2, 1], np.float32)
DEGENERATE_KEPT = [0, 1, 2, 4]                     # zero-area pairs: NaN IoU, not suppressed; the exact duplicate is


def clustered_boxes(g, n, ties=True):
    """The generator of test_nms_bit_exact: boxes scattered around n/20 centres, scores on a 1/4 grid when ties."""
    ctr = g.uniform(0, 1300, (max(n // 20, 1), 2))
    c = ctr[g.integers(0, len(ctr), n)] + g.normal(0, 25, (n, 2))
    wh = g.uniform(8, 220, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    scores = g.standard_normal(n).astype(np.float32)
    if ties:
        scores = np.round(scores * 4) / 4
    return boxes, scores.astype(np.float32)


# ---- the oracle with the stage's parameters -------------------------------------------------------------------------------------
class StageOracle(FRCNNOracle):
    """FRCNNOracle.rpn_proposals with the stage's parameters taken from the arguments (the oracle reads them from its config;
    its anchor grid has the C4 stride built in)."""

    def __init__(self, cell, pre, post, thr, min_size=0.0, stride=16, offset=0.0, weights=(1.0, 1.0, 1.0, 1.0)):
        d = vg_c4_config_dict()
        d["rpn"].update(pre_nms_topk_test=int(pre), post_nms_topk_test=int(post), nms_thresh=float(thr),
                        bbox_reg_weights=[float(w) for w in weights])
        d["proposal_generator"]["min_size"] = float(min_size)
        d["anchor_generator"]["offset"] = float(offset)
        super().__init__(Config(d), {"proposal_generator.anchor_generator.cell_anchors.0":
                                     torch.from_numpy(np.ascontiguousarray(cell, dtype=np.float32))})
        self.stride = int(stride)

    def grid_anchors(self, Hf, Wf, stride=None):
        return super().grid_anchors(Hf, Wf, self.stride)


# ---- device calls through the C ABI ----------------------------------------------------------------------------------------------
def _ignorey_arg(bands, f64, keep):
    """bands [N, J, 2] (already scaled) -> vk_ignorey*; the device tensors are parked in `keep` for the call's duration."""
    if bands is None:
        return None
    bt = torch.as_tensor(np.asarray(bands, np.float64 if f64 else np.float32)).to(G.DEV).contiguous()
    cnt = torch.full((bt.shape[0],), bt.shape[1], dtype=torch.int32, device=G.DEV)
    ig = L.vk_ignorey(bt.data_ptr(), cnt.data_ptr(), bt.shape[1], 1 if f64 else 0)
    keep += [bt, cnt, ig]
    return C.byref(ig)


def _outputs(N, post, nan_fill):
    fill = float("nan") if nan_fill else 0.0
    ob = torch.full((N, post, 4), fill, dtype=torch.float32, device=G.DEV)
    ol = torch.full((N, post), fill, dtype=torch.float32, device=G.DEV)
    oc = torch.full((N,), -7 if nan_fill else 0, dtype=torch.int32, device=G.DEV)
    return ob, ol, oc, torch.zeros((1,), dtype=torch.int32, device=G.DEV)


def rpn_call(obj, dlt, shapes, cell, pre, post, thr, min_size=0.0, stride=16, offset=0.0, weights=(1.0, 1.0, 1.0, 1.0),
             interleaved=False, nan_fill=False, bands=None, bands_f64=False):
    """obj [N,A,H,W], dlt [N,4A,H,W] (oracle layout) -> vk_rpn_proposals (vk_rpn_proposals_ignorey with `bands`) ->
    (boxes [N,post,4], logits [N,post], counts [N], non-finite flag), whole buffers, on the host.  interleaved: logits and
    deltas in one [N,H,W,5A] buffer with one row stride, deltas at +A, the way the model's RPN head writes them."""
    N, A, Hf, Wf = obj.shape
    lg = obj.permute(0, 2, 3, 1).contiguous().to(G.DEV)            # [N,H,W,A]
    dl = dlt.permute(0, 2, 3, 1).contiguous().to(G.DEV)            # [N,H,W,4A]
    ld_l, ld_d = A, 4 * A
    if interleaved:
        both = torch.cat([lg, dl], 3).contiguous()                 # [N,H,W,A | 4A]
        lg, dl, ld_l, ld_d = both, both[..., A:], 5 * A, 5 * A
    ca = torch.from_numpy(np.ascontiguousarray(cell, dtype=np.float32)).to(G.DEV)
    hw = torch.tensor(shapes, dtype=torch.int32, device=G.DEV)
    ob, ol, oc, flag = _outputs(N, post, nan_fill)
    ws = torch.empty(L.load().vk_rpn_workspace_bytes(N, Hf * Wf * A, pre), dtype=torch.uint8, device=G.DEV)
    args = [C.c_void_p(lg.data_ptr()), ld_l, C.c_void_p(dl.data_ptr()), ld_d, N, Hf, Wf, A, G.P(ca), int(stride), float(offset), G.P(hw),
            (C.c_float * 4)(*weights), float(min_size), float(thr), pre, post, G.P(ob), G.P(ol), G.P(oc), G.P(flag), G.P(ws),
            ws.numel(), G.stream()]
    keep = []
    if bands is None:
        L.call("vk_rpn_proposals", *args)
    else:
        L.call("vk_rpn_proposals_ignorey", *args, _ignorey_arg(bands, bands_f64, keep))
    torch.cuda.synchronize()                                       # the flag is read after the stream is done
    return ob.cpu(), ol.cpu(), oc.cpu(), int(flag.item())


def _rpn_gpu(obj, dlt, shapes, cell, pre, post, thr, min_size=0.0, **kw):
    """rpn_call for finite inputs: the flag must be clear; per image (boxes [count,4], logits [count])."""
    ob, ol, oc, flag = rpn_call(obj, dlt, shapes, cell, pre, post, thr, min_size, **kw)
    assert flag == 0
    cnt = oc.tolist()
    return [(ob[i, :cnt[i]], ol[i, :cnt[i]]) for i in range(len(cnt))]


def ml_call(objs, dlts, cells, strides, shapes, pre, post, thr, min_size=0.0, offset=0.0, weights=(1.0, 1.0, 1.0, 1.0),
            nan_fill=False, bands=None, bands_f64=False):
    """Per level obj [N,A,Hl,Wl], dlt [N,4A,Hl,Wl] -> vk_rpn_proposals_multilevel(_ignorey) -> (boxes, logits, counts, flag)."""
    nl, N, A = len(objs), objs[0].shape[0], objs[0].shape[1]
    lg = [o.permute(0, 2, 3, 1).contiguous().to(G.DEV) for o in objs]                      # [N,H,W,A]
    dl = [d.view(N, A, 4, d.shape[2], d.shape[3]).permute(0, 3, 4, 1, 2).reshape(N, d.shape[2], d.shape[3], 4 * A).contiguous().to(G.DEV)
          for d in dlts]                                                                   # [N,H,W,4A] in (a, coord) order
    ce = [torch.from_numpy(np.ascontiguousarray(c, np.float32)).to(G.DEV) for c in cells]
    P_ = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])      # noqa: E731
    I_ = lambda vs: (C.c_int32 * nl)(*[int(v) for v in vs])             # noqa: E731
    hw = torch.tensor(shapes, dtype=torch.int32, device=G.DEV)
    ob, ol, oc, flag = _outputs(N, post, nan_fill)
    nb = L.load().vk_rpn_multilevel_workspace_bytes(N, nl, pre, post)
    ws = torch.empty(nb, dtype=torch.uint8, device=G.DEV)
    args = [P_(lg), I_([A] * nl), P_(dl), I_([4 * A] * nl), nl, N, I_([o.shape[2] for o in objs]), I_([o.shape[3] for o in objs]), A,
            P_(ce), I_(strides), float(offset), G.P(hw), (C.c_float * 4)(*weights), float(min_size), float(thr), pre, post, G.P(ob),
            G.P(ol), G.P(oc), G.P(flag), G.P(ws), nb, G.stream()]
    keep = []
    if bands is None:
        L.call("vk_rpn_proposals_multilevel", *args)
    else:
        L.call("vk_rpn_proposals_multilevel_ignorey", *args, _ignorey_arg(bands, bands_f64, keep))
    torch.cuda.synchronize()
    return ob.cpu(), ol.cpu(), oc.cpu(), int(flag.item())


def _ml_call(objs, dlts, cells, strides, shapes, pre, post, thr, min_size=0.0):
    ob, ol, oc, flag = ml_call(objs, dlts, cells, strides, shapes, pre, post, thr, min_size)
    assert flag == 0
    return ob, ol, oc


def _nms_gpu(boxes, scores, thr):
    """vk_nms -> kept indices (into the input order), int64."""
    n = len(boxes)
    bd = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(G.DEV)
    sd_ = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(G.DEV)
    keep = torch.zeros(max(n, 1), dtype=torch.int64, device=G.DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=G.DEV)
    ws = torch.empty(L.load().vk_nms_workspace_bytes(n), dtype=torch.uint8, device=G.DEV)
    L.call("vk_nms", G.P(bd), G.P(sd_), n, float(thr), G.P(keep), G.P(cnt), G.P(ws), ws.numel(), G.stream())
    torch.cuda.synchronize()
    return keep[: int(cnt.item())].cpu().numpy()


# ---- a single-level selection case, built once for the oracle, the restatement and the device -------------------------------------
class SelCase:
    """One call's inputs on exact data: per image a logit regime and an image size."""

    def __init__(self, name, Hf, Wf, A, pre, regimes, shapes, stride=4, offset=0.0, weights=(1.0, 1.0, 1.0, 1.0), min_size=0.0,
                 cells=None, post=None, thr=NO_SUPPRESSION, seeds=None):
        self.name, self.Hf, self.Wf, self.A, self.pre = name, Hf, Wf, A, pre
        self.regimes, self.shapes, self.stride, self.offset = list(regimes), [list(s) for s in shapes], stride, offset
        self.weights, self.min_size, self.thr = tuple(weights), min_size, thr
        self.post = pre if post is None else post
        self.N, self.HWA = len(self.regimes), Hf * Wf * A
        self.K = min(pre, self.HWA)
        self.cell = exact_cells(A) if cells is None else np.asarray(cells, np.float32)
        self.logits = np.stack([regime_logits(r, self.HWA, name, i, (seeds or {}).get((name, i), 0)).reshape(Hf, Wf, A)
                                for i, r in enumerate(self.regimes)])
        self.deltas = exact_deltas(rng_for("deltas", name), self.N, Hf, Wf, A)

    def oracle_layout(self):
        return to_oracle_layout(self.logits, self.deltas)

    def oracle(self):
        o = StageOracle(self.cell, self.pre, self.post, self.thr, self.min_size, self.stride, self.offset, self.weights)
        return o.rpn_proposals(*self.oracle_layout(), self.shapes)

    def restatement(self, n):
        anc = grid_anchors_np(self.Hf, self.Wf, self.cell, self.stride, self.offset)
        return select_restatement(self.logits[n].reshape(-1), self.deltas[n].reshape(-1, 4), anc, self.K, self.weights,
                                  self.shapes[n], self.min_size)

    def kw(self):
        return dict(shapes=self.shapes, cell=self.cell, pre=self.pre, post=self.post, thr=self.thr, min_size=self.min_size,
                    stride=self.stride, offset=self.offset, weights=self.weights)


def cut_shape(Hf, Wf, stride, cut=(5, 11)):
    """An integer image size a little inside the anchor grid's extent (beyond it for a negative cut): the border anchors are
    clipped, some to nothing."""
    return [max(Hf * stride - cut[0], 9), max(Wf * stride - cut[1], 9)]
