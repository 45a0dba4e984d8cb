"""The hand cases of the detection evaluation, written once and run twice: by tests/test_detection_eval_oracle.py through the
oracle (tests/detection_eval_ref.py) and by tests/test_gpu_detection_eval.py through boxes.evaluate_detections -- TEST ONLY.

`ev(P, S, L, label_ignore=None, pred_ignore=None, thresholds=None, mode='3d')` returns an object with the fields of
boxes.DetectionEval as attributes.  Decisions are exact, values are held to abs=1e-15 as the AP hand cases are."""
import math

import numpy as np
import pytest


def box(x, y, l=4.0, w=2.0, yaw=0.0, z=1.0, h=1.5):
    """x, y, z, l, w, h, yaw; at yaw 0 the WIDTH lies along x and the length along y."""
    return [x, y, z, l, w, h, yaw]


A, B, C, FAR = box(0, 0), box(20, 0), box(0, 20), box(40, 0)
EXACT = dict(abs=1e-15)


def ignored_label_is_neither_hit_nor_miss(ev):
    """g0 and g1 (ignored) far apart; ranked: p0 on g1, p1 nowhere, p2 on g0.  Three inputs, three different numbers."""
    P, S = [[B, FAR, A]], [[0.9, 0.8, 0.7]]
    r = ev(P, S, [[A, B]], label_ignore=[[False, True]], thresholds=[0.5])
    assert r.state.tolist() == [[2, 0, 1]] and r.tp.tolist() == [[False, False, True]] and r.tp_count.tolist() == [[1]]
    assert r.ap[0] == pytest.approx(1.0 / 2.0, **EXACT) and (r.n_labels, r.n_ignored_labels, r.n_predictions) == (1, 1, 3)
    assert r.best_label.tolist() == [0, 0, 0] and r.best_iou[:2].tolist() == [0.0, 0.0]      # g1 is never a candidate
    assert r.ignored_iou[0] == pytest.approx(1.0, abs=1e-12) and r.ignored_iou[1:].tolist() == [0.0, 0.0]
    r = ev(P, S, [[A, B]], label_ignore=[[False, False]], thresholds=[0.5])                 # the flag cleared
    assert r.state.tolist() == [[1, 0, 1]] and r.ap[0] == pytest.approx(5.0 / 6.0, **EXACT) and r.n_labels == 2
    r = ev(P, S, [[A]], thresholds=[0.5])                                                   # g1 removed
    assert r.state.tolist() == [[0, 0, 1]] and r.ap[0] == pytest.approx(1.0 / 3.0, **EXACT) and r.n_labels == 1


def ignored_label_absorbs_any_number(ev):
    r = ev([[B, box(20.1, 0), box(19.9, 0), A]], [[0.9, 0.8, 0.7, 0.6]], [[A, B]], label_ignore=[[False, True]], thresholds=[0.5])
    assert r.state.tolist() == [[2, 2, 2, 1]] and r.ap[0] == pytest.approx(1.0, **EXACT) and r.best_f1[0] == 1.0


def heading_flip_costs_orientation_score_only(ev):
    """Copies of two labels, one of them turned by pi: the rectangle IoU cannot see it, sim and AOS can."""
    turned = box(20, 0, yaw=math.pi)
    r = ev([[A, turned]], [[0.9, 0.8]], [[A, B]], thresholds=[0.5])
    assert r.state.tolist() == [[1, 1]] and r.ap[0] == pytest.approx(1.0, **EXACT)
    assert r.geom[:, 0].tolist() == pytest.approx([1.0, 0.0], **EXACT)
    assert r.aos[0] == pytest.approx(3.0 / 4.0, **EXACT) and r.aoe[0] == pytest.approx(math.pi / 2.0, **EXACT)
    assert r.mAP == pytest.approx(1.0, **EXACT) and r.mAOS == pytest.approx(0.75, **EXACT)
    r = ev([[A, turned]], [[0.8, 0.9]], [[A, B]], thresholds=[0.5])                         # the turned one ranked first
    assert r.ap[0] == pytest.approx(1.0, **EXACT) and r.aos[0] == pytest.approx(1.0 / 2.0, **EXACT)
    assert r.aoe[0] == pytest.approx(math.pi / 2.0, **EXACT) and r.aos[0] <= r.ap[0]


def flagged_prediction_can_still_hit(ev):
    r = ev([[A]], [[0.9]], [[A]], pred_ignore=[[True]], thresholds=[0.5])
    assert r.state.tolist() == [[1]] and r.ap[0] == pytest.approx(1.0, **EXACT) and r.tp_count.tolist() == [[1]]
    r = ev([[FAR]], [[0.9]], [[A]], pred_ignore=[[True]], thresholds=[0.5])                 # the same prediction moved away
    assert r.state.tolist() == [[2]] and r.ap[0] == 0.0 and r.best_f1[0] == 0.0 and math.isnan(r.best_f1_score[0])
    assert math.isnan(r.ate[0]) and math.isnan(r.ase[0]) and math.isnan(r.aoe[0])
    r = ev([[FAR]], [[0.9]], [[A]], thresholds=[0.5])                                       # ... and without the flag
    assert r.state.tolist() == [[0]]


def duplicate_on_a_taken_label_over_an_ignored_one(ev):
    """The duplicate overlaps the ignored label with IoU 7.2 / 8.8 > t: it is left out instead of counting as a miss."""
    dup = box(0.1, 0)
    r = ev([[A, dup]], [[0.9, 0.8]], [[A, box(0.3, 0)]], label_ignore=[[False, True]], thresholds=[0.5, 0.9])
    assert r.best_label.tolist() == [0, 0] and r.state.tolist() == [[1, 2], [1, 0]]          # 0.818 clears 0.5, not 0.9
    assert r.ignored_iou[1] == pytest.approx(7.2 / 8.8, abs=1e-12)
    assert r.ap.tolist() == pytest.approx([1.0, 1.0], **EXACT)                              # a miss BEHIND the only hit costs nothing
    r = ev([[A, dup]], [[0.9, 0.8]], [[A, box(0.3, 0)]], thresholds=[0.5])                  # not ignored: dup's best is A, taken
    assert r.state.tolist() == [[1, 0]]


def geometry_words(ev):
    r = ev([[box(3, 4)], [box(0, 0, l=8.0)]], [[0.9], [0.8]], [[A], [A]], thresholds=[0.25])
    assert r.geom[0].tolist() == pytest.approx([1.0, 5.0, 0.0, 0.0], **EXACT)
    assert r.geom[1].tolist() == pytest.approx([1.0, 0.0, 0.5, 0.0], **EXACT)
    assert r.state.tolist() == [[0, 1]] and r.ase[0] == pytest.approx(0.5, **EXACT) and r.ate[0] == 0.0
    r = ev([[A], [A]], [[0.9], [0.8]], [[], [A]], thresholds=[0.5])                         # no label in the sample: NaN
    assert np.isnan(r.geom[0]).all() and r.best_label.tolist() == [-1, 0] and r.best_iou[0] == 0.0


def best_f1_and_its_score(ev):
    """Ranked TP, FP, TP with G = 3: F1 = 1/2, 2/5, 2/3."""
    r = ev([[A, FAR, B]], [[0.9, 0.8, 0.7]], [[A, B, C]], thresholds=[0.5], curve=True)
    assert r.state.tolist() == [[1, 0, 1]] and r.best_f1[0] == pytest.approx(2.0 / 3.0, **EXACT) and r.best_f1_score[0] == 0.7
    assert r.curve[0, :, 0].tolist() == pytest.approx([1 / 3, 1 / 3, 2 / 3], **EXACT)
    assert r.curve[0, :, 1].tolist() == pytest.approx([1.0, 1 / 2, 2 / 3], **EXACT)
    r = ev([[A, FAR, FAR]], [[0.9, 0.8, 0.7]], [[A, B, C]], thresholds=[0.5])               # the first of the maxima's rank
    assert r.best_f1[0] == pytest.approx(1.0 / 2.0, **EXACT) and r.best_f1_score[0] == 0.9


ALL = (ignored_label_is_neither_hit_nor_miss, ignored_label_absorbs_any_number, heading_flip_costs_orientation_score_only,
       flagged_prediction_can_still_hit, duplicate_on_a_taken_label_over_an_ignored_one, geometry_words, best_f1_and_its_score)
