"""Every case of tests/box_edge_cases.py still takes the path it was written for, judged on oracle/boxes_ref.py alone: building
a case asserts the margins and the exactness its comparison relies on and the path it is named for (the case file's header),
so this file builds them all without a GPU, and shows on altered cases that those assertions do fail when a case stops
exercising its path.  tests/test_gpu_box_edges.py runs the same cases on the GPU; this file keeps them honest."""
import numpy as np
import pytest

import box_edge_cases as E


@pytest.mark.parametrize("name", list(E.LABEL_CASES))
def test_label_case_meets_its_conditions(name):
    c = E.label_case(name)
    cfg = c["cfg"]
    assert c["cls"].shape == (cfg["outX"], cfg["outY"], 2) and c["reg"].shape == (cfg["outX"], cfg["outY"], 14)
    assert np.array_equal(c["valid"] + c["overlap"], c["cls"]) and np.all(c["overlap"] <= c["valid"])
    assert np.isfinite(c["reg"]).all()


@pytest.mark.parametrize("name", list(E.NMS_CASES))
def test_nms_case_meets_its_conditions(name):
    c = E.nms_case(name)
    assert c["cls"].dtype == np.float32 and c["reg"].dtype == np.float32
    assert len(c["probs"]) == E.candidates(c["cfg"]) and 1 <= len(c["picks"]) <= c["max_boxes"] + 1
    assert len(set(c["picks"])) == len(c["picks"])


def test_every_case_has_its_path_check():
    assert set(E.LABEL_PATHS) == set(E.LABEL_CASES) and set(E.PICKS) == set(E.NMS_CASES)


def test_launch_geometry():
    """Candidate counts that are no multiple of the 128-thread label and the 256-thread decode / suppress workgroups, and one
    beyond the 1024 threads of the pick; 65 boxes are more than one wave."""
    assert E.candidates(E.EXACT) == E.candidates(E.REF12) == 576 and 576 % 128 == 64 and 576 % 256 == 64
    assert E.candidates(E.REF16) == 1280 and 1024 < 1280 < 2048 and 1280 % 1024 == 256
    assert {E.NMS_CASES[n][0]["name"] for n in E.NMS_CASES} == {"ref12", "ref16"}
    assert {E.LABEL_CASES[n]()[0]["name"] for n in E.LABEL_CASES} == {"exact", "ref12", "ref16"}
    assert len(E.label_case("many")["fixed"]) == 65


# ---- the assertions of the case file fail when a case leaves its path -----------------------------------------------------------
def test_fixup_tie_that_gains_a_positive_anchor_is_refused():
    shorter = list(E.FIXUP_TIE)
    shorter[2], shorter[3] = 1.0, 4.0                          # inter 24, union 12 + 48 - 24: IoU 2/3 >= iou_hi
    with pytest.raises(AssertionError, match="no anchor at iou_hi"):
        E.build_label_case("fixup_tie", E.EXACT, [shorter])


def test_a_tie_that_is_not_exact_is_refused():
    turned = list(E.FIXUP_TIE)
    turned[6] = 1e-3                                           # the maxima are no longer equal for every implementation
    with pytest.raises(AssertionError):
        E.build_label_case("fixup_tie", E.EXACT, [turned])
    off_grid = list(E.FIXUP_TIE)
    off_grid[0] += 0.1                                         # not a multiple of 2^-2
    with pytest.raises(AssertionError):
        E.build_label_case("fixup_tie", E.EXACT, [off_grid])


def test_maxima_that_do_not_stand_alone_are_refused():
    """A box that holds two anchors of the reference configuration has one IoU with both, up to rounding."""
    with pytest.raises(AssertionError, match="maxima"):
        E.build_label_case("border_wrap", E.REF12, [[0.5, 0.3, 1.0, 2.8, 4.0, 1.5, 0.0]])


def test_untied_probabilities_are_refused_as_a_tie_case():
    cfg, head, thresh, max_boxes = E.NMS_CASES["ties_576"]
    with pytest.raises(AssertionError, match="share one probability"):
        E.build_nms_case("ties_576", cfg, dict(seed=head["seed"]), thresh, max_boxes)


def test_a_list_that_does_not_run_out_is_refused_as_exhausted():
    cfg, head, _, max_boxes = E.NMS_CASES["exhausted"]
    with pytest.raises(AssertionError):
        E.build_nms_case("exhausted", cfg, head, 5.0, max_boxes)
