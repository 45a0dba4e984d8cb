"""The detection-output oracle (tests/detect_ref.py) against answers worked out by hand, and the guard on every case the GPU
file (tests/test_gpu_detect.py) compares exactly: no raw score within 1e-9 of the score threshold, no consulted IoU within 1e-9
of the IoU threshold, no two passing candidates with one score unless the case is about ties.  The seeds in detect_cases were
chosen here, on the CPU, so that this holds; no case leaves anything out of its comparison.  Runs without a GPU."""
import math

import numpy as np
import pytest

import detect_cases as C
import detect_ref as D

MARGIN = 1e-9


def test_key_order_is_the_numeric_order():
    s = np.array([-math.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.5, 0.5000001, 7.0, math.inf], dtype=np.float32)
    bits = D.ordered_bits(s)
    assert np.all(np.diff(bits.astype(np.int64)) > 0) and bits.min() > 0
    ok = np.ones(6, dtype=bool)
    raw = np.array([1.0, 2.0, 1.0, 2.0, 1.0, -5.0], dtype=np.float32)
    assert D.ranking(ok, raw, 10).tolist() == [3, 1, 4, 2, 0, 5]          # equal scores: the larger flat index first
    assert D.ranking(ok, raw, 3).tolist() == [3, 1, 4]
    ok[4] = False
    assert D.ranking(ok, raw, 3).tolist() == [3, 1, 2]


def test_builder_inverts_the_decode():
    maps = C.Maps()
    want = [C.car(30.3, 41.7, 0.4, l=4.4, w=1.9, z=0.8, h=1.6), C.car(2.0, 99.0, -2.0)]
    at = [maps.put(want[0], 1.5), maps.put(want[1], 0.5, at=(1, 7, 190))]
    boxes, raw = D.decode(maps.reg), D.raw_scores(maps.cls)
    assert at[1] == C.M + 7 * 200 + 190 and at[0] == 30 * 200 + 83
    assert np.allclose(boxes[at], want, rtol=0, atol=1e-5) and raw[at].tolist() == [1.5, 0.5]
    other = np.setdiff1d(np.arange(2 * C.M), at)
    assert np.all(raw[other] == C.FILL) and np.array_equal(boxes[other][:, 3:6], np.tile([1.6, 3.9, 1.56], (len(other), 1)))
    assert boxes[1, :3].tolist() == [0.5, 0.75, 1.0] and boxes[C.M + 1, 6] == math.pi / 2


def test_chain_by_hand():
    """A (3.0) suppresses B (2.0): IoU 3.2 / 12.8 = 0.25.  B overlaps C (1.0) just as much, A and C are 0.4 m apart: C stays,
    which a rule that drops whatever overlaps ANYTHING ranked higher would get wrong."""
    maps = C.Maps()
    a, b, c = (maps.put(C.car(40.0 + dx, 50.0), s) for dx, s in ((0.0, 3.0), (1.2, 2.0), (2.4, 1.0)))
    got = D.detect(maps.cls, maps.reg, score_threshold=-10.0, iou_threshold=0.1)
    assert got["index"].tolist() == [a, c] and got["count"] == (2, 3) and got["ranked"].tolist() == [a, b, c]
    assert got["scores"].tolist() == [3.0, 1.0]
    assert sorted(got["consulted"].tolist()) == pytest.approx([0.0, 0.25], abs=1e-6)     # (A, B), then (A, C): B is not kept
    assert D.margins(got, -10.0, 0.1) == (pytest.approx(11.0), pytest.approx(0.1))
    over = D.detect(maps.cls, maps.reg, score_threshold=-10.0, iou_threshold=0.3)        # above 0.25: nothing is suppressed
    assert over["index"].tolist() == [a, b, c]
    capped = D.detect(maps.cls, maps.reg, score_threshold=-10.0, iou_threshold=0.3, max_boxes=2)
    assert capped["index"].tolist() == [a, b] and capped["count"] == (2, 3) and len(capped["consulted"]) == 1
    assert D.detect(maps.cls, maps.reg, score_threshold=2.5)["index"].tolist() == [a]
    sig = D.detect(maps.cls, maps.reg, score_threshold=-10.0, sigmoid_scores=True)
    assert sig["scores"].tolist() == pytest.approx([1 / (1 + math.exp(-3.0)), 1 / (1 + math.exp(-1.0))], rel=1e-15)


def test_tie_by_hand():
    """Three lone candidates with one score: the larger flat index ranks first, and makes the cut."""
    maps = C.Maps()
    lo = maps.put(C.car(10.0, 10.0), 0.5, at=(0, 10, 20))
    mid = maps.put(C.car(50.0, 50.0), 0.5, at=(0, 50, 100))
    hi = maps.put(C.car(30.0, 80.0), 0.5, at=(1, 30, 160))
    top = maps.put(C.car(80.0, 20.0), 0.75, at=(0, 80, 40))
    assert lo < mid < top < hi
    got = D.detect(maps.cls, maps.reg, score_threshold=-10.0)
    assert got["index"].tolist() == [top, hi, mid, lo] and D.tied_scores(got) == 3
    cut = D.detect(maps.cls, maps.reg, score_threshold=-10.0, pre_nms_top_n=3, max_boxes=3)
    assert cut["index"].tolist() == [top, hi, mid] and cut["count"] == (3, 4)


def test_filters_by_hand():
    ref, raw = C.case("filters_raw")["ref"], C.case("filters_raw")["ref"]["all_raw"]
    inf_at, out_at = 1 * 200 + 30, 0 * 200 + 150
    assert ref["index"][0] == inf_at and ref["scores"][0] == math.inf and out_at not in ref["ranked"]
    assert ref["count"][1] == 1 + int((raw[np.isfinite(raw)] > 0.5).sum()) - 4     # +inf; less the four bad boxes at 4.0 .. 4.3
    both = C.case("filters_raw_outside_too")["ref"]
    assert both["ranked"][:2].tolist() == [inf_at, out_at] and both["count"][1] == ref["count"][1] + 1
    logits = C.case("filters_logits")["ref"]
    assert logits["scores"][0] == 1.0 and np.all((logits["scores"] > 0.6) & (logits["scores"] <= 1.0))
    assert 0 < logits["count"][1] and np.all(np.diff(logits["scores"]) <= 0)


def test_cases_are_what_their_names_say():
    n = {k: C.case(k)["ref"]["count"] for k in C.CASES}
    assert n["top1"] == (1, 200) and n["top64_exactly"][1] == 64 and n["top1000_fewer"][1] == 700
    assert n["top1000_exactly"][1] == 1000 and n["top4096_of_4500"][1] == 4500 and n["nothing_passes"] == (0, 0)
    for name in ("top63", "top64", "top65"):
        assert n[name][1] == 200 and len(C.case(name)["ref"]["ranked"]) == int(name[3:]) and 20 <= n[name][0] <= int(name[3:])
    assert len(C.case("top4096_of_4500")["ref"]["ranked"]) == 4096 and 300 <= n["top4096_of_4500"][0] <= 1000
    assert n["all_equal_fewer"][1] == 50 and len(C.case("all_equal_cut")["ref"]["ranked"]) == 30
    eq = C.case("all_equal_cut")["ref"]
    assert np.all(np.diff(eq["ranked"]) < 0) and eq["ranked"][-1] > np.sort(np.nonzero(eq["ok"])[0])[19]
    st = C.case("tie_straddles_the_cut")["ref"]
    tied = np.nonzero(st["ok"] & (st["all_raw"] == 1.0))[0]
    assert len(tied) == 10 and st["ranked"][15:].tolist() == np.sort(tied)[::-1][:5].tolist()
    fill = C.case("fill_ties_without_a_threshold")["ref"]
    assert fill["count"][1] == 2 * C.M and fill["ranked"][200:].tolist() == list(range(2 * C.M - 1, 2 * C.M - 101, -1))
    # anchor boxes k cells apart along their 3.9 m side: IoU (3.9 - k/2) / (3.9 + k/2) > 0.1 up to k = 6, so every 7th stays
    assert fill["index"][np.isin(fill["index"], fill["ranked"][200:])].tolist() == list(range(2 * C.M - 1, 2 * C.M - 101, -7))
    assert n["cap"][0] == 50 and n["cap"][1] == 600 and len(C.case("cap")["ref"]["index"]) == 50
    cap_free = D.detect(C.case("cap")["cls"], C.case("cap")["reg"], **dict(C.oracle_arguments(C.case("cap")["kw"]), max_boxes=1000))
    assert cap_free["count"][0] > 100 and cap_free["index"][:50].tolist() == C.case("cap")["ref"]["index"].tolist()
    bev, z3d = C.case("z_pairs_bev")["ref"], C.case("z_pairs_3d")["ref"]
    assert bev["count"] == (2, 4) and z3d["count"] == (3, 4) and z3d["index"][[0, 2]].tolist() == bev["index"].tolist()
    cl = C.case("clustered_scene")["ref"]
    assert cl["count"][1] == 700 and 100 <= cl["count"][0] < 300 and len(cl["consulted"]) > 2000


def test_chains_keep_everything_but_the_victims():
    ref = C.case("chains")["ref"]
    assert ref["count"][1] == 4096 and len(ref["ranked"]) == 4096
    kept_ranks = np.nonzero(np.isin(ref["ranked"], ref["index"]))[0]
    assert kept_ranks.tolist() == [r for r in range(4096) if r not in C.CHAIN_RANKS["B"]] and ref["count"][0] == 4090
    assert np.array_equal(ref["index"], ref["ranked"][kept_ranks])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_no_case_sits_on_a_rounding_edge(name):
    c = C.case(name)
    args = C.oracle_arguments(c["kw"])
    to_score, to_iou = D.margins(c["ref"], args["score_threshold"], args["iou_threshold"])
    print(f"{name}: kept {c['ref']['count'][0]} of {len(c['ref']['ranked'])} ranked, {c['ref']['count'][1]} passing; "
          f"{len(c['ref']['consulted'])} IoUs consulted; margins score {to_score:.3e} IoU {to_iou:.3e}")
    assert to_score >= MARGIN and to_iou >= MARGIN
    assert (D.tied_scores(c["ref"]) > 0) == c["ties"]
