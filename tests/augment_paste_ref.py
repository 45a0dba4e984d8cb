"""Test-local float64 oracle for ground-truth object sampling (lisec_augment_owner / lisec_augment_sample /
lisec_augment_paste and augment.ObjectDatabase) -- TEST ONLY.

Plain Python / numpy, written from the text of include/lisec_hip.h section 5c; the Philox words, the footprint clipping,
the owner rule and the draw / apply stages behind the sampling are those of tests/augment_ref.py.
"""
import numpy as np

import augment_ref as R

MAX_SAMPLES = 64              # LISEC_AUG_MAX_SAMPLES
PAD = 2.0 * R.PAD_LIMIT       # the pad rows of a recorded step's point buffer: (1e6, 1e6, 1e6)


def owner(points, boxes):
    """R.owner with the pad rows (|x| >= PAD_LIMIT) owned by nobody."""
    points = np.asarray(points, dtype=np.float64)[:, :3]
    own = R.owner(points, boxes)
    own[~(np.abs(points[:, 0]) < R.PAD_LIMIT)] = -1
    return own


def build_database(points_list, boxes_list, min_points=5):
    """dict(boxes (M, 7), points (P, 3), offsets (M + 1,) int32, counts (M,) int32): every box owning >= min_points points
    (at least one), sweep by sweep and box by box, with its points in the sweep's order; float64 if any sweep is."""
    dtype = np.float64 if any(np.asarray(p).dtype == np.float64 for p in points_list) else np.float32
    rows, pts, counts = [], [], []
    for p, b in zip(points_list, boxes_list):
        p, b = np.asarray(p), np.asarray(b, dtype=np.float64).reshape(-1, 7)
        own = owner(p, b)
        for j in range(len(b)):
            sel = np.nonzero(own == j)[0]
            if len(sel) >= max(min_points, 1):
                rows.append(b[j])
                pts.append(p[sel, :3].astype(dtype))
                counts.append(len(sel))
    counts = np.array(counts, dtype=np.int32)
    return dict(boxes=np.array(rows, dtype=np.float64).reshape(-1, 7),
                points=np.concatenate(pts) if pts else np.zeros((0, 3), dtype),
                offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), counts=counts)


def bound(db, K):
    """The most points K sampled objects can add: the sum of the K largest point counts."""
    return int(np.sort(db["counts"].astype(np.int64))[::-1][:max(K, 0)].sum())


def sample_count(B, sample_to):
    K = min(MAX_SAMPLES, max(0, int(sample_to) - B))
    if B + K > R.MAX_BOXES:
        raise ValueError("too many boxes")
    return K


def database_index(w0, M):
    return (int(w0) * int(M)) >> 32


def sample(boxes, db, K, seed=0, item=0, epoch=0, decisions=None):
    """dict(index (K,) int32, n_boxes, boxes_all (B + K, 7), point_offset (K + 1,) int32, draws (4 K,) uint32).  decisions,
    when a list, collects (area, separation or None) of every candidate-against-scene-box and candidate-against-earlier-
    candidate test (accepted or not: the kernel makes them all)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    B, M = len(boxes), len(db["boxes"])
    if K > MAX_SAMPLES or B + K > R.MAX_BOXES:
        raise ValueError("too many samples")
    index = -np.ones(K, dtype=np.int32)
    drawn = -np.ones(K, dtype=np.int64)
    draws = np.zeros(4 * K, dtype=np.uint32)
    point_offset = np.zeros(K + 1, dtype=np.int32)
    boxes_all = np.zeros((B + K, 7))
    boxes_all[:B] = boxes
    n_boxes = B
    for k in range(K):
        w = R.words(seed, 3, item, epoch, k)
        draws[4 * k:4 * k + 4] = w
        point_offset[k + 1] = point_offset[k]
        if M == 0:
            continue
        drawn[k] = database_index(w[0], M)
        cand = db["boxes"][drawn[k]]
        free = True
        others = [(boxes[j], True) for j in range(B)] + [(db["boxes"][drawn[m]], index[m] >= 0) for m in range(k)]
        for other, counts in others:
            if not counts and decisions is None:
                continue
            ar = R.overlap_area(cand, other)
            if decisions is not None:
                decisions.append((ar, R.separation(cand, other) if ar == 0.0 else None))
            if ar != 0.0 and counts:
                free = False
        if free:
            index[k] = drawn[k]
            boxes_all[n_boxes] = cand
            n_boxes += 1
            point_offset[k + 1] += db["counts"][drawn[k]]
    return dict(index=index, n_boxes=n_boxes, boxes_all=boxes_all, point_offset=point_offset, draws=draws)


def paste(points, db, smp, n_scene_boxes, cap=None):
    """(cap, 3) in the points' dtype (cap defaults to n + bound(db, K)): the scene rows -- a live one inside an accepted pasted
    box becomes a pad row --, the accepted objects' points in order of k, pad rows.  Also returns the removed mask (n,)."""
    points = np.asarray(points)
    n, K = len(points), len(smp["index"])
    if cap is None:
        cap = n + bound(db, K)
    out = np.full((cap, 3), PAD, dtype=points.dtype)
    out[:n] = points[:, :3]
    pasted = smp["boxes_all"][n_scene_boxes:smp["n_boxes"]]
    removed = owner(points, pasted) >= 0 if n else np.zeros(0, dtype=bool)
    out[:n][removed] = PAD
    at = n
    for k in range(K):
        m = smp["index"][k]
        if m >= 0:
            assert at == n + smp["point_offset"][k]
            obj = db["points"][db["offsets"][m]:db["offsets"][m + 1]]
            out[at:at + len(obj)] = obj.astype(points.dtype)
            at += len(obj)
    assert at == n + smp["point_offset"][K] <= cap
    return out, removed


def item(points, boxes, db, sample_to, seed=0, item=0, epoch=0, **params):
    """The whole item: sample, paste, then R.draw / R.apply over the first n_boxes rows.  Returns (points' (n + bound, 3)
    float64, boxes' (n_boxes, 7), the sample, the pasted sweep before the noise)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    smp = sample(boxes, db, sample_count(len(boxes), sample_to), seed, item, epoch)
    pasted, _ = paste(points, db, smp, len(boxes))
    live = smp["boxes_all"][:smp["n_boxes"]]
    d = R.draw(live, seed, item, epoch, **params)
    return R.apply(pasted.astype(np.float64), live, d["transforms"], d["scale"], d["alpha"]), d["boxes"], smp, pasted


def label_margins(boxes, nx=200, ny=400, voxelx=0.5, voxely=0.25, iou_lo=0.45, iou_hi=0.6):
    """How far the label maps of `boxes` (ego metres) are from depending on rounding: (the least best-anchor IoU of a box
    minus iou_hi, the least |IoU - threshold| over all anchors x boxes).  A box whose footprint lies inside two neighbouring
    anchors has the same IoU with both, so WHICH anchor a box without a positive one is given (serialize_data.py:297-307)
    rests on rounding; with the first figure positive every box has positive anchors and that rule never fires."""
    import math
    from oracle.boxes_ref import calculate_iou
    outX, outY, vx, vy = nx // 2, ny // 2, voxelx * 2, voxely * 2
    anchors = [[1.6, 3.9, 1.56, 0], [1.6, 3.9, 1.56, math.pi / 2]]
    fixed = np.asarray(boxes, dtype=np.float64).reshape(-1, 7).copy()
    fixed[:, [0, 3]] *= outX / nx
    fixed[:, [1, 4]] *= outY / ny
    least_best, least_gap = math.inf, math.inf
    for fb in fixed:
        best = 0.0
        for a in anchors:
            reach = 0.5 * math.hypot(fb[3], fb[4]) + 0.5 * math.hypot(a[0], a[1])
            for xV in range(max(-outX // 2, int((fb[0] - reach) / vx) - 1), min(outX // 2, int((fb[0] + reach) / vx) + 2)):
                cX = vx * xV + vx / 2
                if cX - a[0] / 2 < -vx * (outX // 2) or cX + a[0] / 2 > vx * (outX // 2):
                    continue
                for yV in range(max(-outY // 2, int((fb[1] - reach) / vy) - 1), min(outY // 2, int((fb[1] + reach) / vy) + 2)):
                    cY = vy * yV + vy / 2
                    if cY - a[1] / 2 < -vy * (outY // 2) or cY + a[1] / 2 > vy * (outY // 2):
                        continue
                    if math.hypot(fb[0] - cX, fb[1] - cY) > reach:
                        continue
                    iou = calculate_iou([cX, cY, 1.0] + a, fb)
                    best = max(best, iou)
                    least_gap = min(least_gap, abs(iou - iou_lo), abs(iou - iou_hi))
        least_best = min(least_best, best - iou_hi)
    return least_best, least_gap
