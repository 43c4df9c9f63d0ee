"""Test-local restatement of the reference's ignorey branch (find_top_rpn_proposals frcnn.py:328-366) and of the proposal
pipelines around it, built from the oracle's pieces.  Used by test_ignorey_host.py and test_gpu_ignorey.py."""
import torch

from oracle.frcnn_oracle import FRCNNOracle, argsort_desc, batched_nms


def scaled_bands(ignorey_n, scale_x):
    """frcnn.py:331 for one image: ignorey[n] * 1 / scales_yx[n, 1] with float32 scales (float64 bands stay float64)."""
    t = torch.as_tensor(ignorey_n)
    t = t if t.dtype == torch.float64 else t.to(torch.float32)
    return t.reshape(-1, 2) * 1 / torch.tensor(scale_x, dtype=torch.float32)


def band_restatement(boxes, bands):
    """One image, in candidate slots: boxes [K, 4] f32 (the pre-band top-k, in rank order), bands [J, 2] already scaled
    (their dtype is the comparison dtype).  Returns (boxes with the survivors trimmed, keep mask).  Band j sees the
    survivors of bands < j with their rows as already trimmed; both trim tests use the rows before band j's trims."""
    b = boxes.clone()
    keep = torch.ones(b.shape[0], dtype=torch.bool)
    for g in bands:
        y0, y1 = b[:, 1].to(g.dtype), b[:, 3].to(g.dtype)
        drop = keep & (g[1] <= y1) & (g[0] >= y0)                  # the box spans the whole band
        above = (y0 > g[1]) & (y1 > g[0])                          # box_ignore_above; box_ignore_below is always false
        to_clip = keep & ~drop & ~above
        top = to_clip & ((g[1] - y1).abs() < (g[0] - y0).abs())
        bottom = to_clip & ((g[0] - y0).abs() < (g[1] - y1).abs())
        b[bottom, 1] = int(g[1])
        b[top, 3] = int(g[0])
        keep &= ~drop
    return b, keep


def _finish(boxes, scores, lvl, hw, cfg):
    FRCNNOracle.clip_box(boxes, hw)                                 # frcnn.py:369 (asserts finite survivors)
    ms = cfg.PROPOSAL_GENERATOR.MIN_SIZE
    keep = ((boxes[:, 2] - boxes[:, 0]) > ms) & ((boxes[:, 3] - boxes[:, 1]) > ms)
    boxes, scores, lvl = boxes[keep], scores[keep], lvl[keep]
    k = batched_nms(boxes, scores, lvl, cfg.RPN.NMS_THRESH)[:cfg.RPN.POST_NMS_TOPK_TEST]
    return boxes[k], scores[k]


def c4_proposals(oracle, obj, dlt, shapes, bands):
    """FRCNNOracle.rpn_proposals with the band step; bands: per image a scaled [J_i, 2] tensor.  Each image on its own."""
    cfg = oracle.cfg
    N, A, Hf, Wf = obj.shape
    anchors = oracle.grid_anchors(Hf, Wf)
    d = dlt.view(N, A, 4, Hf, Wf).permute(0, 3, 4, 1, 2).reshape(-1, 4)
    props = FRCNNOracle.apply_deltas(d, anchors.unsqueeze(0).expand(N, -1, -1).reshape(-1, 4), cfg.RPN.BBOX_REG_WEIGHTS).view(N, -1, 4)
    logits = obj.permute(0, 2, 3, 1).reshape(N, -1)
    pre = min(cfg.RPN.PRE_NMS_TOPK_TEST, logits.shape[1])
    res = []
    for n in range(N):
        order = argsort_desc(logits[n])[:pre]
        boxes, keep = band_restatement(props[n][order], bands[n])
        res.append(_finish(boxes[keep], logits[n][order][keep], torch.zeros(int(keep.sum()), dtype=torch.int64), shapes[n], cfg))
    return res


def fpn_proposals(cfg, cells, objs, dlts, shapes, bands):
    """oracle.fpn_oracle.multilevel_proposals with the band step on each image's concatenated candidates."""
    N = objs[0].shape[0]
    strides = [4 * 2 ** i for i in range(len(objs))]
    tk_b, tk_s, lvl = [], [], []
    for li, (obj, dlt, base, stride) in enumerate(zip(objs, dlts, cells, strides)):
        _, A, Hf, Wf = obj.shape
        off = cfg.ANCHOR_GENERATOR.OFFSET
        sx = torch.arange(off * stride, Wf * stride, step=stride, dtype=torch.float32)
        sy = torch.arange(off * stride, Hf * stride, step=stride, dtype=torch.float32)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
        anchors = (shifts.view(-1, 1, 4) + torch.as_tensor(base).float().view(1, -1, 4)).reshape(-1, 4)
        d = dlt.reshape(N, A, 4, Hf, Wf).permute(0, 3, 4, 1, 2).reshape(-1, 4)
        props = FRCNNOracle.apply_deltas(d, anchors.unsqueeze(0).expand(N, -1, -1).reshape(-1, 4),
                                         cfg.RPN.BBOX_REG_WEIGHTS).view(N, -1, 4)
        logits = obj.permute(0, 2, 3, 1).reshape(N, -1)
        k = min(cfg.RPN.PRE_NMS_TOPK_TEST, logits.shape[1])
        orders = [argsort_desc(logits[n])[:k] for n in range(N)]
        tk_b.append(torch.stack([props[n][o] for n, o in enumerate(orders)]))
        tk_s.append(torch.stack([logits[n][o] for n, o in enumerate(orders)]))
        lvl.append(torch.full((k,), li, dtype=torch.int64))
    boxes_all, scores_all, lvl_all = torch.cat(tk_b, 1), torch.cat(tk_s, 1), torch.cat(lvl)
    res = []
    for n in range(N):
        boxes, keep = band_restatement(boxes_all[n], bands[n])
        res.append(_finish(boxes[keep], scores_all[n][keep], lvl_all[keep], shapes[n], cfg))
    return res
