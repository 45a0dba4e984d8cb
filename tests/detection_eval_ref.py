"""Test-local float64 oracle for the detection evaluation (lisec_boxes_evaluate / lisec_boxes_evaluate_integrate) -- TEST ONLY.

Plain Python / numpy, written from the definition in include/lisec_hip.h: the pair IoU and the ranking of
tests/detection_ap_ref.py, a taken flag per (threshold, non-ignored label), a serial walk in rank order, forward running
sums and the envelopes by the textbook loop.  Samples are lists: P[s] (k, 7) predictions, S[s] (k,) scores, L[s] (m, 7)
labels, rows x, y, z, l, w, h, yaw; label_ignore[s] (m,) / pred_ignore[s] (k,) booleans, None: none set.

Also the random cases the CPU and the GPU tests share (case()): the CPU test asserts their margins, the GPU test runs them.
"""
import math

import numpy as np

from detection_ap_ref import DEFAULT_THRESHOLDS, clustered_scene, iou_matrix, pair_iou, ranking      # noqa: F401

MARGIN = 1e-9


def _rows(b):
    return np.asarray(b, dtype=np.float64).reshape(-1, 7)


def _flags(flags, boxes):
    if flags is None:
        return [np.zeros(len(_rows(b)), dtype=bool) for b in boxes]
    return [np.asarray(f, dtype=bool).reshape(-1) for f in flags]


def geom(p, g):
    """(sim, dist, scale, yaw) of a prediction against its candidate."""
    d = p[6] - g[6]
    vp, vg = abs(p[3] * p[4] * p[5]), abs(g[3] * g[4] * g[5])
    v = min(abs(p[3]), abs(g[3])) * min(abs(p[4]), abs(g[4])) * min(abs(p[5]), abs(g[5]))
    den = vp + vg - v
    return [(1.0 + math.cos(d)) / 2.0, math.sqrt((p[0] - g[0]) ** 2 + (p[1] - g[1]) ** 2), 1.0 - v / den if den > 0 else 1.0,
            abs(math.atan2(math.sin(d), math.cos(d)))]


def envelope_sum(rec, val):
    """The recall-weighted sum of the envelope of `val` from the right (the PASCAL-VOC rule of detection_ap_ref.ap_from_hits)."""
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mval = np.concatenate([[0.0], val, [0.0]])
    for i in range(len(mval) - 2, -1, -1):
        mval[i] = max(mval[i], mval[i + 1])
    total = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            total += (mrec[i + 1] - mrec[i]) * mval[i + 1]
    return total


def evaluate(P, S, L, label_ignore=None, pred_ignore=None, thresholds=None, mode='3d', ious=None):
    """The whole definition.  Returns a dict with the fields of boxes.DetectionEval, `order` (the ranking as flat rows),
    `f1` ([per threshold: the F1 of every non-ignored rank, in rank order]) and `best_tol` / `ignored_tol` (N,): the bound
    1e-10 * (summed |l*w|) / union + 1e-12 of the pair that best_iou / ignored_iou comes from (1e-12 without one).
    ious: [iou_matrix(P[s], L[s], mode, with_union=True)] when the caller has them already."""
    thr = DEFAULT_THRESHOLDS if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    P, L = [_rows(p) for p in P], [_rows(g) for g in L]
    S = [np.asarray(s, dtype=np.float64).reshape(-1) for s in S]
    li, pi = _flags(label_ignore, L), _flags(pred_ignore, P)
    n_s, T = len(P), len(thr)
    both = [iou_matrix(P[s], L[s], mode, with_union=True) for s in range(n_s)] if ious is None else ious
    ious = [b[0] for b in both]
    start = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(int)
    N = int(start[-1])
    n_ignored = int(sum(f.sum() for f in li))
    G = int(sum(len(g) for g in L)) - n_ignored
    if G <= 0:
        raise ValueError("the evaluation is undefined without a label that is not ignored")
    best_iou, best_label, ignored_iou = np.zeros(N), np.full(N, -1, dtype=np.int32), np.zeros(N)
    best_tol, ignored_tol = np.full(N, 1e-12), np.full(N, 1e-12)
    gm = np.full((N, 4), np.nan)
    scores, flagged = np.zeros(N), np.zeros(N, dtype=bool)
    for s in range(n_s):
        lw = np.abs(P[s][:, 3] * P[s][:, 4])[:, None] + np.abs(L[s][:, 3] * L[s][:, 4])[None, :]
        uni = both[s][1]
        tol = 1e-10 * np.divide(lw, uni, out=np.zeros_like(lw), where=uni > 0) + 1e-12
        for i in range(len(P[s])):
            row = start[s] + i
            scores[row], flagged[row] = S[s][i], pi[s][i]
            for j in range(len(L[s])):
                v = ious[s][i, j]
                if li[s][j]:
                    if v > ignored_iou[row]:
                        ignored_iou[row], ignored_tol[row] = v, tol[i, j]
                elif best_label[row] < 0 or v > best_iou[row]:
                    best_iou[row], best_label[row], best_tol[row] = v, j, tol[i, j]
            if best_label[row] >= 0:
                gm[row] = geom(P[s][i], L[s][best_label[row]])
    order = ranking(S)
    flat = np.array([start[s] + i for s, i in order], dtype=np.int64)
    state = np.zeros((T, N), dtype=np.uint8)
    tp_count = np.zeros((n_s, T), dtype=np.int32)
    out = {k: np.zeros(T) for k in ('ap', 'aos', 'ate', 'ase', 'aoe', 'best_f1', 'best_f1_score')}
    curve = np.full((T, N, 3), np.nan)
    f1_all = []
    for t, th in enumerate(thr):
        taken = [np.zeros(len(L[s]), dtype=bool) for s in range(n_s)]
        for s, i in order:                                      # the serial walk
            row = start[s] + i
            j = best_label[row]
            if j >= 0 and best_iou[row] > th and not taken[s][j]:
                taken[s][j] = True
                state[t, row] = 1
                tp_count[s, t] += 1
            elif ignored_iou[row] > th or flagged[row]:
                state[t, row] = 2
        cum_tp, cum_fp, cum_sim = 0, 0, 0.0
        rec, prec, os_, f1 = [], [], [], []
        best, best_score = 0.0, math.nan
        for k, row in enumerate(flat):
            if state[t, row] == 2:
                continue
            if state[t, row] == 1:
                cum_tp += 1
                cum_sim += gm[row, 0]
            else:
                cum_fp += 1
            rec.append(cum_tp / float(G))
            prec.append(cum_tp / float(cum_tp + cum_fp))
            os_.append(cum_sim / float(cum_tp + cum_fp))
            f1.append(2.0 * cum_tp / float(cum_tp + cum_fp + G))
            curve[t, k] = [rec[-1], prec[-1], os_[-1]]
            if f1[-1] > best:                                   # strictly: the lowest rank among equals
                best, best_score = f1[-1], scores[row]
        out['ap'][t] = envelope_sum(np.array(rec), np.array(prec))
        out['aos'][t] = envelope_sum(np.array(rec), np.array(os_))
        hits = np.flatnonzero(state[t] == 1)                    # flat-row order
        for name, col in (('ate', 1), ('ase', 2), ('aoe', 3)):
            out[name][t] = float(np.sum(gm[hits, col])) / len(hits) if len(hits) else math.nan
        out['best_f1'][t], out['best_f1_score'][t] = best, best_score
        f1_all.append(np.array(f1))
    return dict(out, mAP=float(out['ap'].mean()), mAOS=float(out['aos'].mean()), thresholds=thr, state=state, tp=state == 1,
                tp_count=tp_count, best_iou=best_iou, best_label=best_label, ignored_iou=ignored_iou, geom=gm, order=flat,
                n_predictions=N, n_labels=G, n_ignored_labels=n_ignored, curve=curve, f1=f1_all, best_tol=best_tol,
                ignored_tol=ignored_tol)


def margins(P, S, L, label_ignore=None, pred_ignore=None, thresholds=None, mode='3d', ious=None):
    """How far the inputs are from a decision that rounding could flip: the minimum gaps (best_iou, threshold),
    (ignored_iou, threshold), (best, second-best positive IoU among a prediction's non-ignored labels), (two distinct scores)
    and, per threshold, (largest, second-largest distinct F1).  inf where there is no such pair."""
    r = evaluate(P, S, L, label_ignore, pred_ignore, thresholds, mode, ious)
    thr = r['thresholds']
    L = [_rows(g) for g in L]
    li = _flags(label_ignore, L)
    ious = [iou_matrix(P[s], L[s], mode) for s in range(len(P))] if ious is None else [b[0] for b in ious]
    has = r['best_label'] >= 0
    to_thr = float(np.abs(r['best_iou'][has][:, None] - thr[None, :]).min()) if has.any() else math.inf
    to_ign = float(np.abs(r['ignored_iou'][:, None] - thr[None, :]).min()) if r['n_predictions'] else math.inf
    to_second = math.inf
    for m, f in zip(ious, li):
        for row in m:
            pos = np.sort(row[~f][row[~f] > 0])
            if len(pos) >= 2:
                to_second = min(to_second, float(pos[-1] - pos[-2]))
    scores = np.unique(np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in S] + [np.zeros(0)]))
    score_gap = float(np.diff(scores).min()) if len(scores) >= 2 else math.inf
    f1_gap = math.inf
    for f1 in r['f1']:
        distinct = np.unique(f1)
        if len(distinct) >= 2:
            f1_gap = min(f1_gap, float(distinct[-1] - distinct[-2]))
    return to_thr, to_ign, to_second, score_gap, f1_gap


# ---- the random cases the CPU test (margins) and the GPU test (comparison) share ------------------------------------------
def scene(rng, n_pred, n_label, n_clusters):
    """The scene of tests/test_gpu_detection_ap.py: labels are car-sized boxes in separated clusters, predictions are labels
    drawn with replacement and disturbed a little or a lot, scores uniform.  The same draws for the same generator."""
    _, L = clustered_scene(rng, 0, n_label, n_clusters)
    P = np.zeros((n_pred, 7))
    for i in range(n_pred):
        noise = rng.choice([0.03, 0.1, 0.25, 0.6])
        P[i] = L[rng.integers(n_label)] + rng.normal(0, 1, 7) * noise * [1, 1, 0.3, 0.5, 0.3, 0.3, 0.2]
    return P, rng.uniform(0.01, 0.99, n_pred), L


def _flagged_scene(rng, n_pred, n_label, n_clusters, p_label=0.3, p_pred=0.1):
    P, S, L = scene(rng, n_pred, n_label, n_clusters)
    return P, S, L, rng.uniform(size=n_label) < p_label, rng.uniform(size=n_pred) < p_pred


def _many(rng, sizes):
    """One small flagged scene per (n_pred, n_label) of `sizes`, with globally distinct, interleaved scores."""
    P, S, L, LI, PI = [], [], [], [], []
    total = sum(n for n, _ in sizes)
    scores = (rng.permutation(total) + 1) / (2.0 * total)
    at = 0
    for n_pred, n_label in sizes:
        p, _, g, li, pi = _flagged_scene(rng, n_pred, n_label, max(1, n_label // 3))
        P.append(p); S.append(scores[at:at + n_pred]); L.append(g); LI.append(li); PI.append(pi)
        at += n_pred
    return P, S, L, LI, PI


def _ignore_ranks(P, S, PI, ranks):
    """Makes the predictions at the given ranks ignored ones at every threshold: moved far from every label, flag set."""
    start = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(int)
    order = ranking(S)
    for k in ranks:
        s, i = order[k]
        P[s][i, 0] += 500.0
        PI[s][i] = True
    return [int(start[s] + i) for s, i in (order[k] for k in ranks)]


CASE_NAMES = ("mixed_empty", "seventy", "chunk_edge_1025", "chunk_edge_2049", "one_threshold", "sixteen_thresholds")


def case(name):
    """dict(P, S, L, label_ignore, pred_ignore, thresholds, mode[, ignored_ranks])."""
    none = np.zeros((0, 7))
    if name == "mixed_empty":                                   # no predictions / no labels / only ignored labels, mixed in
        rng = np.random.default_rng(41)
        P1, S1, L1, LI1, PI1 = _flagged_scene(rng, 6, 5, 2)
        P2, S2, L2, LI2, PI2 = _flagged_scene(rng, 4, 6, 2)
        LI1[0], LI1[1] = True, False
        P = [none, P1, P1[:2], none, P2, none, P2[:3]]
        S = [[], S1, [0.405, 0.605], [], S2, [], [0.111, 0.222, 0.333]]
        L = [L1[:2], L1, none, none, L2, none, L2[:3]]
        LI = [[False, True], LI1, [], [], LI2, [], [True, True, True]]
        PI = [[], PI1, [False, True], [], PI2, [], [False, False, True]]
        return dict(P=P, S=S, L=L, label_ignore=LI, pred_ignore=PI, thresholds=None, mode="3d")
    if name == "seventy":                                       # 70 x 70 in one sample: more pairs than a workgroup
        P, S, L, LI, PI = _flagged_scene(np.random.default_rng(42), 70, 70, 12)
        return dict(P=[P], S=[S], L=[L], label_ignore=[LI], pred_ignore=[PI], thresholds=None, mode="bev")
    if name == "chunk_edge_1025":                               # one rank more than one integration chunk
        P, S, L, LI, PI = _many(np.random.default_rng(43), [(5, 3)] * 205)
        rows = _ignore_ranks(P, S, PI, (0, 1023, 1024))
        return dict(P=P, S=S, L=L, label_ignore=LI, pred_ignore=PI, thresholds=[0.5, 0.7], mode="3d", ignored_rows=rows)
    if name == "chunk_edge_2049":                               # one more than two chunks; 1025 samples: two scan chunks
        P, S, L, LI, PI = _many(np.random.default_rng(44), [(2, 2)] * 1024 + [(1, 2)])
        rows = _ignore_ranks(P, S, PI, (0, 1023, 1024, 2047, 2048))
        return dict(P=P, S=S, L=L, label_ignore=LI, pred_ignore=PI, thresholds=[0.5, 0.7], mode="3d", ignored_rows=rows)
    if name == "one_threshold":
        P, S, L, LI, PI = _many(np.random.default_rng(45), [(30, 25), (12, 9)])
        return dict(P=P, S=S, L=L, label_ignore=LI, pred_ignore=PI, thresholds=[0.5], mode="3d")
    if name == "sixteen_thresholds":
        P, S, L, LI, PI = _many(np.random.default_rng(46), [(30, 25), (12, 9)])
        return dict(P=P, S=S, L=L, label_ignore=LI, pred_ignore=PI, thresholds=np.linspace(0.2, 0.95, 16), mode="bev")
    raise KeyError(name)


def run(c):
    """evaluate and margins of a case (the IoU matrices are computed once)."""
    ious = [iou_matrix(p, g, c["mode"], with_union=True) for p, g in zip(c["P"], c["L"])]
    args = (c["P"], c["S"], c["L"], c["label_ignore"], c["pred_ignore"], c["thresholds"], c["mode"], ious)
    return evaluate(*args), margins(*args)
