"""The detection-evaluation oracle (tests/detection_eval_ref.py) against hand cases and against the average-precision oracle
it extends, the margins of every random case the GPU test runs, and the refusals that need no GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import detection_ap_ref as R
import detection_eval_hand as H
import detection_eval_ref as E


def _ev(P, S, L, label_ignore=None, pred_ignore=None, thresholds=None, mode="3d", curve=False):
    return SimpleNamespace(**E.evaluate(P, S, L, label_ignore, pred_ignore, thresholds, mode))


@pytest.mark.parametrize("check", H.ALL, ids=[c.__name__ for c in H.ALL])
def test_hand_cases(check):
    check(_ev)


@pytest.mark.parametrize("seed, sizes, mode", [(21, [(70, 70, 12)], "3d"), (11, [(5, 4, 2), (3, 6, 2), (0, 3, 1), (4, 0, 1)], "bev"),
                                                (25, [(20, 40, 10)] * 3, "3d")])
def test_without_flags_the_oracle_is_the_average_precision_oracle(seed, sizes, mode):
    rng = np.random.default_rng(seed)
    P, S, L = [], [], []
    for n_pred, n_label, n_clusters in sizes:
        p, s, g = E.scene(rng, n_pred, max(n_label, 1), n_clusters)
        P.append(p); S.append(s); L.append(g[:n_label])
    want = R.average_precision(P, S, L, None, mode)
    for flags in (None, [np.zeros(len(g), dtype=bool) for g in L]):
        got = E.evaluate(P, S, L, flags, None, None, mode)
        for name in ("ap", "tp", "tp_count", "best_iou", "best_label", "order"):
            assert np.array_equal(got[name], want[name]), name
        assert got["mAP"] == want["mAP"] and got["n_labels"] == want["n_labels"] and got["n_ignored_labels"] == 0
        assert np.array_equal(got["state"], want["tp"].astype(np.uint8)) and not got["ignored_iou"].any()
        assert np.all(got["aos"] <= got["ap"]) and np.all(got["aos"] > 0)


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_random_cases_sit_away_from_every_rounding_edge(name):
    """The seeds were chosen here, on the CPU, so that every gap is at least the project's MARGIN."""
    c = E.case(name)
    r, gaps = E.run(c)
    print(name, "margins (best IoU to threshold, ignored IoU to threshold, best to second IoU, score to score, best to second F1):", gaps)
    assert min(gaps) >= E.MARGIN, gaps
    # the case is what its name says: every state occurs, flags of both kinds are set, the ignored ranks are where they should be
    assert all((r["state"] == k).any() for k in (0, 1, 2)) and r["n_ignored_labels"] > 0
    assert any(np.asarray(f, dtype=bool).any() for f in c["pred_ignore"])
    assert np.all(r["aos"] <= r["ap"] + 1e-15)
    if "ignored_rows" in c:
        N = r["n_predictions"]
        ranks = sorted(int(np.flatnonzero(r["order"] == row)[0]) for row in c["ignored_rows"])
        assert N % 1024 == 1 and ranks == sorted({0, N - 1} | {k for e in range(1024, N, 1024) for k in (e - 1, e)})
        assert np.all(r["state"][:, c["ignored_rows"]] == 2) and np.isnan(r["curve"][:, ranks]).all()
    if name == "mixed_empty":
        sizes = [(len(p), len(g), int(np.sum(f))) for p, g, f in zip(c["P"], c["L"], c["label_ignore"])]
        assert any(n == 0 and m > 0 for n, m, _ in sizes) and any(n > 0 and m == 0 for n, m, _ in sizes)
        assert any(n > 0 and m > 0 and i == m for n, m, i in sizes) and (0, 0, 0) in sizes
    if name == "chunk_edge_2049":
        assert len(c["P"]) > 1024


def test_oracle_refuses_a_list_without_a_counting_label():
    with pytest.raises(ValueError):
        E.evaluate([[H.A]], [[0.5]], [[H.A]], label_ignore=[[True]])
    with pytest.raises(ValueError):
        E.evaluate([[H.A]], [[0.5]], [[]])


# ---- the Python surface, where no GPU is needed ------------------------------------------------------------------------------
def test_evaluate_detections_refuses_before_it_touches_the_device():
    from lisec_amd import boxes, rpnToRegion
    assert rpnToRegion.evaluate_detections is boxes.evaluate_detections and rpnToRegion.evaluate_by_range is boxes.evaluate_by_range
    assert rpnToRegion.points_in_boxes is boxes.points_in_boxes
    A, B = H.A, H.B
    for kw in (dict(label_ignore=[[True]]),                    # a flag too few
               dict(label_ignore=[[True, False], [False]]),    # a sample too many
               dict(pred_ignore=[[True, False]]),              # a flag too many
               dict(pred_ignore=[]),                           # a sample too few
               dict(label_ignore=[[True, True]]),              # no label left that counts
               dict(iou_thresholds=[0.5] * 17), dict(iou_thresholds=[1.0]), dict(iou_thresholds=[]), dict(mode="2d")):
        with pytest.raises(ValueError):
            boxes.evaluate_detections([[A]], [[0.5]], [[A, B]], **kw)
    with pytest.raises(ValueError):
        boxes.evaluate_detections([[A]], [[0.5]], [np.zeros((0, 7))])          # no label at all
    with pytest.raises(ValueError):
        boxes.evaluate_detections([[A]], [[0.5]], [[A], [B]])                  # a label set too many
    with pytest.raises(ValueError):
        boxes.evaluate_by_range([[A]], [[0.5]], [[A, B]], label_ignore=[[True]])
    with pytest.raises(ValueError):
        boxes.evaluate_by_range([[A]], [[0.5]], [[A, B]], pred_ignore=[[True, True]])
    # a bin without a label that counts maps to None, without a launch
    assert boxes.evaluate_by_range([[A]], [[0.5]], [[A, B]], ranges=((100, math.inf),)) == {(100.0, math.inf): None}


def test_detection_evaluation_refuses_at_construction():
    from lisec_amd import callbacks, model_training
    assert model_training.callbacks.DetectionEvaluation is callbacks.DetectionEvaluation
    pts, bx = np.zeros((5, 3)), np.asarray([H.A])
    for args, kw in ((([pts, pts], [bx]), {}), (([pts], [bx, bx]), {}), (([pts], [np.zeros((0, 7))]), {}), (([], []), {}),
                     (([pts], [bx]), dict(every=0)), (([pts], [bx]), dict(every=-2)), (([pts], [bx]), dict(every=1.5)),
                     (([pts], [bx]), dict(detector=dict(max_boxes=5, as_device=True)))):
        with pytest.raises(ValueError):
            callbacks.DetectionEvaluation(*args, **kw)
    cb = callbacks.DetectionEvaluation([pts], [bx], detector=dict(max_boxes=5), every=2, prefix="test_")
    assert (cb.every, cb.prefix, cb.detector, cb.last) == (2, "test_", dict(max_boxes=5), None)
    logs = {}
    cb.on_epoch_end(0, logs)                                   # a skipped epoch: no key, and nothing that needs a model
    assert logs == {}
