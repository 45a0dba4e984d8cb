"""The detection-AP oracle (tests/detection_ap_ref.py) against answers worked out by hand.  No GPU."""
import math

import numpy as np
import pytest

import detection_ap_ref as R


def _box(x, y, l, w, yaw=0.0, z=1.0, h=1.5):
    """x, y, z, l, w, h, yaw; at yaw 0 the WIDTH lies along x and the length along y."""
    return [x, y, z, l, w, h, yaw]


def test_identical_boxes_have_iou_one():
    b = _box(0.3, -0.2, 4.5, 1.9, 0.4)
    for mode in ("3d", "bev"):
        assert R.iou_matrix([b], [b], mode)[0, 0] == pytest.approx(1.0, abs=1e-12)
    assert R.iou_matrix([_box(0, 0, 4, 2)], [_box(0, 0, 4, 2)])[0, 0] == 1.0


def test_same_footprint_offset_in_z():
    """h = 2, z one apart: the height intervals share 1 of 2, inter = A, union = 2 * 2A - A: exactly 1/3; bird's-eye 1."""
    p, g = _box(0, 0, 4, 2, z=0.0, h=2.0), _box(0, 0, 4, 2, z=1.0, h=2.0)
    assert R.iou_matrix([p], [g], "3d")[0, 0] == 1.0 / 3.0
    assert R.iou_matrix([p], [g], "bev")[0, 0] == 1.0
    far = _box(0, 0, 4, 2, z=5.0, h=2.0)                       # apart in z: the clamp, not a negative volume
    assert R.iou_matrix([p], [far], "3d")[0, 0] == 0.0 and R.iou_matrix([p], [far], "bev")[0, 0] == 1.0


def test_squares_shifted_by_half_a_side():
    assert R.iou_matrix([_box(0, 0, 2, 2)], [_box(1, 0, 2, 2)], "bev")[0, 0] == 1.0 / 3.0    # 2 / (4 + 4 - 2)
    assert R.iou_matrix([_box(0, 0, 2, 2)], [_box(0, 1, 2, 2)], "3d")[0, 0] == 1.0 / 3.0     # same z and h: the same ratio


def test_degenerate_and_mirrored_boxes():
    sq = _box(0, 0, 2, 2)
    for flat in (_box(0, 0, 0, 2), _box(0, 0, 2, 0)):
        for mode in ("3d", "bev"):
            assert R.iou_matrix([flat], [sq], mode)[0, 0] == 0.0 and R.iou_matrix([sq], [flat], mode)[0, 0] == 0.0
    thin = _box(0, 0, 2, 2, h=0.0)
    assert R.iou_matrix([thin], [sq], "3d")[0, 0] == 0.0 and R.iou_matrix([thin], [sq], "bev")[0, 0] == 1.0
    mirrored = _box(0, 0, -2, 2, h=-1.5)                       # negative extents mirror the footprint: the same box
    assert R.iou_matrix([mirrored], [sq], "3d")[0, 0] == 1.0
    with pytest.raises(ValueError):
        R.iou_matrix([sq], [sq], "2d")


A, B = _box(0, 0, 4, 2), _box(20, 0, 4, 2)


def test_three_predictions_two_labels_by_hand():
    """Ranked hits [TP, FP, TP], G = 2: rec .5 .5 1, prec 1 .5 2/3, envelope 1 2/3 2/3: AP = .5 * 1 + .5 * 2/3 = 5/6."""
    P = [[A, _box(40, 0, 4, 2), B]]
    r = R.average_precision(P, [[0.9, 0.8, 0.7]], [[A, B]], thresholds=[0.5])
    assert r["tp"].tolist() == [[True, False, True]] and r["best_label"].tolist() == [0, 0, 1]
    assert r["ap"][0] == pytest.approx(5.0 / 6.0, abs=1e-15) and r["mAP"] == r["ap"][0]
    assert r["tp_count"].tolist() == [[2]] and r["n_predictions"] == 3 and r["n_labels"] == 2
    # the input order does not matter, the scores do
    r2 = R.average_precision([[B, A, _box(40, 0, 4, 2)]], [[0.7, 0.9, 0.8]], [[A, B]], thresholds=[0.5])
    assert r2["tp"].tolist() == [[True, True, False]] and r2["ap"][0] == r["ap"][0]
    assert R.ap_from_hits([1, 0, 1], 2) == pytest.approx(5.0 / 6.0, abs=1e-15)


def test_all_false_positives_duplicates_and_empty_sides():
    miss = _box(40, 0, 4, 2)
    r = R.average_precision([[miss, miss]], [[0.9, 0.8]], [[A, B]], thresholds=[0.5, 0.75])
    assert not r["tp"].any() and r["ap"].tolist() == [0.0, 0.0] and r["mAP"] == 0.0
    # two predictions on one label: the lower-scored one is a false positive
    r = R.average_precision([[A, A]], [[0.3, 0.6]], [[A]], thresholds=[0.5])
    assert r["tp"].tolist() == [[False, True]] and r["ap"][0] == 1.0
    # a sample without labels: its predictions are false positives; one without predictions only adds labels
    r = R.average_precision([[A], [], [A]], [[0.9], [], [0.8]], [[], [B], [A]], thresholds=[0.5])
    assert r["tp"].tolist() == [[False, True]] and r["best_label"].tolist() == [-1, 0] and r["n_labels"] == 2
    assert r["ap"][0] == pytest.approx(0.5 * 0.5, abs=1e-15)   # one hit of two labels at precision 1/2
    r = R.average_precision([[]], [[]], [[A]], thresholds=[0.5])
    assert r["ap"].tolist() == [0.0] and r["n_predictions"] == 0
    with pytest.raises(ValueError):
        R.average_precision([[A]], [[0.5]], [[]])
    with pytest.raises(ValueError):
        R.ap_from_hits([1], 0)


def test_strict_threshold_and_tie_rules():
    # shift 0.47 of 2 m wide boxes: (2 - .47) / (2 + .47) = 0.619..: TP at .5 .55 .6, FP from .65 up
    r = R.average_precision([[_box(0.47, 0, 4, 2)]], [[0.9]], [[A]])
    assert r["best_iou"][0] == pytest.approx(1.53 / 2.47, abs=1e-12)
    assert r["tp"][:, 0].tolist() == [True] * 3 + [False] * 7 and r["mAP"] == pytest.approx(0.3, abs=1e-15)
    # iou > t is strict: an exact 1/3 is no hit at t = 1/3
    r = R.average_precision([[_box(0, 1, 2, 2)]], [[0.9]], [[_box(0, 0, 2, 2)]], thresholds=[1.0 / 3.0, 0.33])
    assert r["tp"][:, 0].tolist() == [False, True]
    # equal scores: the lower sample first, then the lower row; equal IoU: the lower label
    r = R.average_precision([[_box(40, 0, 4, 2)], [A, A]], [[0.5], [0.5, 0.5]], [[A], [A, A]], thresholds=[0.5])
    assert r["order"].tolist() == [0, 1, 2] and r["tp"].tolist() == [[False, True, False]] and r["best_label"].tolist() == [0, 0, 0]
    assert r["ap"][0] == pytest.approx((1.0 / 3.0) * 0.5, abs=1e-15)


def test_margins():
    P, S, L = [[_box(0.47, 0, 4, 2), _box(20.2, 0, 4, 2)]], [[0.9, 0.25]], [[A, B, _box(0.2, 0, 4, 2)]]
    to_thr, to_second, score_gap = R.margins(P, S, L, thresholds=[0.5, 0.85])
    ious = R.iou_matrix(P[0], L[0])
    assert ious[0, 2] > ious[0, 0] > 0 and ious[0, 1] == 0
    assert to_second == pytest.approx(ious[0, 2] - ious[0, 0], abs=1e-15)          # prediction 1 meets one label only
    assert to_thr == pytest.approx(min(abs(ious[0, 2] - 0.85), abs(ious[1, 1] - 0.85)), abs=1e-15)
    assert score_gap == pytest.approx(0.65, abs=1e-15)
    assert R.margins([[A]], [[0.5]], [[A]])[1:] == (math.inf, math.inf)
