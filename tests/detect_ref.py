"""Test-local float64 oracle for the many-box detection output (lisec_detect, include/lisec_hip.h section 5b) -- TEST ONLY.

Plain numpy / Python, written from the header text: the decode of the anchor grid, the filters, the key order (ordered
float32 bits, then the larger flat index), the top-N cut, and greedy NMS by value with the IoU of tests/detection_ap_ref.py
(every consulted pair whose footprints can touch is clipped there; a pair whose centres are further apart than 1.01 x the sum
of the half-diagonals has IoU exactly 0 by geometry and is not clipped -- a fact about rectangles, not code shared with the
kernel).  Maps: cls (outX, outY, 2), reg (outX, outY, 14) float32; candidate i = a * M + m, m = ix * outY + iy.
"""
import math

import numpy as np

import detection_ap_ref as AP

GRID = dict(outX=100, outY=200, vx=1.0, vy=0.5, anchors=((1.6, 3.9, 1.56, 0.0), (1.6, 3.9, 1.56, math.pi / 2)))


def decode(reg, grid=GRID):
    """(2 M, 7) float64 rows x, y, z, l, w, h, yaw of every candidate, and nothing else."""
    outX, outY, vx, vy = grid["outX"], grid["outY"], grid["vx"], grid["vy"]
    t = np.asarray(reg, dtype=np.float32).reshape(outX * outY, -1).astype(np.float64)
    m = np.arange(outX * outY)
    x = (m // outY) * vx + vx / 2
    y = (m % outY) * vy + vy / 2
    rows = []
    with np.errstate(over="ignore", invalid="ignore"):
        for a, an in enumerate(grid["anchors"]):
            r = t[:, 7 * a:7 * a + 7]
            rows.append(np.stack([r[:, 0] * an[0] + x, r[:, 1] * an[1] + y, r[:, 2] * an[2] + 1.0, np.exp(r[:, 3]) * an[0],
                                  np.exp(r[:, 4]) * an[1], np.exp(r[:, 5]) * an[2], r[:, 6] + an[3]], axis=1))
    return np.concatenate(rows)


def raw_scores(cls, grid=GRID):
    """(2 M,) float32 in candidate order."""
    c = np.asarray(cls, dtype=np.float32).reshape(grid["outX"] * grid["outY"], -1)
    return np.concatenate([c[:, 0], c[:, 1]])


def ordered_bits(s):
    """uint32 whose unsigned order is the numeric order of the float32 values (-0.0 below +0.0)."""
    u = np.asarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def passing(cls, reg, score_threshold=-math.inf, inside_only=True, grid=GRID):
    """(bool (2 M,), boxes (2 M, 7), raw float32 (2 M,))."""
    boxes, raw = decode(reg, grid), raw_scores(cls, grid)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(raw) & (raw.astype(np.float64) > score_threshold)
        ok &= np.isfinite(boxes).all(axis=1) & (boxes[:, 3] > 0) & (boxes[:, 4] > 0) & (boxes[:, 5] > 0)
        if inside_only:
            ok &= (boxes[:, 0] >= 0) & (boxes[:, 0] <= grid["outX"] * grid["vx"])
            ok &= (boxes[:, 1] >= 0) & (boxes[:, 1] <= grid["outY"] * grid["vy"])
    return ok, boxes, raw


def ranking(ok, raw, top_n):
    """Flat indices of the min(top_n, passing) best candidates: descending score bits, equal scores by the LARGER index."""
    idx = np.nonzero(ok)[0]
    keys = (ordered_bits(raw[idx]).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    return idx[np.argsort(keys)[::-1]][:top_n]


def _half_diagonals(b):
    return 0.5 * np.hypot(b[:, 3], b[:, 4])


def greedy_nms(boxes, iou_threshold, mode, max_boxes):
    """boxes (L, 7) in rank order -> (kept ranks, consulted): rank i is kept unless a KEPT earlier rank has IoU > iou_threshold
    with it; stops once max_boxes are kept.  consulted: the IoU of every (kept earlier rank, rank i) pair looked at before the
    stop, as an array (far pairs contribute their exact 0)."""
    kept, consulted = [], []
    half = _half_diagonals(boxes)
    for i in range(len(boxes)):
        if len(kept) >= max_boxes:
            break
        suppressed = False
        if kept:
            k = np.asarray(kept)
            far = np.hypot(boxes[k, 0] - boxes[i, 0], boxes[k, 1] - boxes[i, 1]) > 1.01 * (half[k] + half[i])
            if far.any():
                consulted.append(0.0)
            for j in k[~far]:
                iou = AP.pair_iou(boxes[j], boxes[i], mode)[0]
                consulted.append(iou)
                suppressed = suppressed or iou > iou_threshold
        if not suppressed:
            kept.append(i)
    return kept, np.asarray(consulted, dtype=np.float64)


def detect(cls, reg, score_threshold=-math.inf, sigmoid_scores=False, pre_nms_top_n=1000, max_boxes=100, iou_threshold=0.1,
           iou_mode="bev", inside_only=True, grid=GRID):
    """The whole definition.  score_threshold is the RAW one (what lisec_detect_cfg holds).  Returns dict(index (k,) flat
    candidate indices in output order, count (kept, passing), boxes (k, 7), scores (k,), raw (k,) float32, ranked = the
    indices after the top-N cut, consulted = the IoUs the greedy pass looked at, all_raw, ok)."""
    ok, boxes, raw = passing(cls, reg, score_threshold, inside_only, grid)
    ranked = ranking(ok, raw, pre_nms_top_n)
    kept, consulted = greedy_nms(boxes[ranked], iou_threshold, iou_mode, max_boxes)
    index = ranked[kept] if len(kept) else np.zeros(0, dtype=np.int64)
    s = raw[index].astype(np.float64)
    with np.errstate(over="ignore"):
        scores = 1.0 / (1.0 + np.exp(-s)) if sigmoid_scores else s
    return dict(index=index.astype(np.int64), count=(len(kept), int(ok.sum())), boxes=boxes[index], scores=scores, raw=raw[index],
                ranked=ranked, consulted=consulted, all_raw=raw, ok=ok)


def margins(result, score_threshold, iou_threshold):
    """(smallest |raw score - score_threshold| over every candidate with a number for a score, smallest |consulted IoU -
    iou_threshold|); inf where there is nothing to compare."""
    raw = result["all_raw"].astype(np.float64)
    raw = raw[np.isfinite(raw)]
    to_score = float(np.abs(raw - score_threshold).min()) if len(raw) and math.isfinite(score_threshold) else math.inf
    c = result["consulted"]
    to_iou = float(np.abs(c - iou_threshold).min()) if len(c) else math.inf
    return to_score, to_iou


def tied_scores(result):
    """How many passing candidates share their float32 score with another passing candidate."""
    raw = result["all_raw"][result["ok"]]
    _, counts = np.unique(ordered_bits(raw), return_counts=True)
    return int(counts[counts > 1].sum())
