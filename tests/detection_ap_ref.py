"""Test-local float64 oracle for detection average precision (lisec_boxes_match / lisec_boxes_average_precision) -- TEST ONLY.

Plain Python / numpy, written from the definition: per-pair IoU from the convex clipping of tests/union_overlap_ref.py,
the rank-ordered take-or-miss walk with a taken flag per (threshold, label), and the PASCAL-VOC precision envelope.
Samples are lists: P[s] (k, 7) predictions, S[s] (k,) scores, L[s] (m, 7) labels, rows x, y, z, l, w, h, yaw.
"""
import math

import numpy as np

from union_overlap_ref import area, clip, clustered_scene, footprint      # noqa: F401  (clustered_scene: for the tests)

DEFAULT_THRESHOLDS = np.arange(0.5, 1.0, 0.05)


def _rows(b):
    return np.asarray(b, dtype=np.float64).reshape(-1, 7)


def pair_iou(p, g, mode='3d'):
    """(iou, union) of one prediction and one label."""
    if mode not in ('3d', 'bev'):
        raise ValueError(mode)
    fp, fg = footprint(p), footprint(g)                        # [] for l == 0 or w == 0
    sp, sg = abs(p[3] * p[4]), abs(g[3] * g[4])
    if mode == '3d':
        sp, sg = abs(p[3] * p[4] * p[5]), abs(g[3] * g[4] * g[5])
    if not fp or not fg or (mode == '3d' and (p[5] == 0 or g[5] == 0)):
        return 0.0, sp + sg
    inter = area(clip(fp, fg))                                 # every pair is clipped: no early-out shared with the kernel
    if mode == '3d':
        hp, hg = abs(p[5]) / 2, abs(g[5]) / 2
        inter = inter * max(0.0, min(p[2] + hp, g[2] + hg) - max(p[2] - hp, g[2] - hg))
    union = sp + sg - inter
    return (inter / union if union > 0 else 0.0), union


def iou_matrix(P, L, mode='3d', with_union=False):
    """(n_pred, n_label) float64 IoU of one sample (and the unions beside it, for tolerances)."""
    P, L = _rows(P), _rows(L)
    out, uni = np.zeros((len(P), len(L))), np.zeros((len(P), len(L)))
    for i, p in enumerate(P):
        for j, g in enumerate(L):
            out[i, j], uni[i, j] = pair_iou(p, g, mode)
    return (out, uni) if with_union else out


def ranking(S):
    """[(sample, row)] of all predictions by descending score, ties by sample index, then by row."""
    keys = [(-float(sc), s, i) for s, scores in enumerate(S) for i, sc in enumerate(np.asarray(scores, dtype=np.float64).reshape(-1))]
    return [(s, i) for _, s, i in sorted(keys)]


def match(P, S, L, thresholds=None, mode='3d', ious=None):
    """The matching of the definition.  Returns dict(tp (T, N) bool in input order, tp_count (n_samples, T), best_iou (N,),
    best_label (N,), order = the ranking as flat input rows, n_predictions, n_labels)."""
    thr = DEFAULT_THRESHOLDS if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    n_s = len(P)
    ious = [iou_matrix(P[s], L[s], mode) for s in range(n_s)] if ious is None else ious
    start = np.concatenate([[0], np.cumsum([len(_rows(p)) for p in P])]).astype(int)
    N, G = int(start[-1]), int(sum(len(_rows(g)) for g in L))
    best_iou, best_label = np.zeros(N), np.full(N, -1, dtype=np.int32)
    for s in range(n_s):
        for i in range(ious[s].shape[0]):
            if ious[s].shape[1]:
                j = int(np.argmax(ious[s][i]))                 # the first of equal maxima: the lowest label index
                best_iou[start[s] + i], best_label[start[s] + i] = ious[s][i, j], j
    order = ranking(S)
    tp = np.zeros((len(thr), N), dtype=bool)
    tp_count = np.zeros((n_s, len(thr)), dtype=np.int32)
    for t, th in enumerate(thr):
        taken = [np.zeros(ious[s].shape[1], dtype=bool) for s in range(n_s)]
        for s, i in order:
            row = start[s] + i
            j = best_label[row]
            if j >= 0 and best_iou[row] > th and not taken[s][j]:
                taken[s][j] = True
                tp[t, row] = True
                tp_count[s, t] += 1
    return dict(tp=tp, tp_count=tp_count, best_iou=best_iou, best_label=best_label,
                order=np.array([start[s] + i for s, i in order], dtype=np.int64), n_predictions=N, n_labels=G, thresholds=thr)


def ap_from_hits(hits, G):
    """AP of one threshold from the ranked hit flags (length N) and the label count G."""
    if G == 0:
        raise ValueError("average precision is undefined without labels")
    hits = np.asarray(hits, dtype=bool)
    N = len(hits)
    cum = np.cumsum(hits.astype(np.int64))
    rec = cum / float(G)
    prec = cum / np.arange(1, N + 1, dtype=np.float64) if N else np.zeros(0)
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    total = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            total += (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return total


def average_precision(P, S, L, thresholds=None, mode='3d', ious=None):
    """dict(ap (T,), mAP, and everything match returns)."""
    if sum(len(_rows(g)) for g in L) == 0:
        raise ValueError("average precision is undefined without labels")
    m = match(P, S, L, thresholds, mode, ious)
    ap = np.array([ap_from_hits(m['tp'][t][m['order']], m['n_labels']) for t in range(len(m['thresholds']))])
    return dict(m, ap=ap, mAP=float(ap.mean()))


def margins(P, S, L, thresholds=None, mode='3d', ious=None):
    """How far the inputs are from a decision that rounding could flip: the minimum gaps (candidate IoU, threshold),
    (best, second-best IoU of a prediction with two or more labels above 0), (two distinct scores).  inf where there is no
    such pair."""
    thr = DEFAULT_THRESHOLDS if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    ious = [iou_matrix(P[s], L[s], mode) for s in range(len(P))] if ious is None else ious
    to_thr, to_second = math.inf, math.inf
    for m in ious:
        for row in m:
            if not len(row):
                continue
            to_thr = min(to_thr, float(np.abs(row.max() - thr).min()))
            pos = np.sort(row[row > 0])
            if len(pos) >= 2:
                to_second = min(to_second, float(pos[-1] - pos[-2]))
    scores = np.unique(np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in S] + [np.zeros(0)]))
    score_gap = float(np.diff(scores).min()) if len(scores) >= 2 else math.inf
    return to_thr, to_second, score_gap
