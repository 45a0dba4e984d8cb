"""The numpy oracle of ground-truth object sampling (tests/augment_paste_ref.py) against hand-made known answers, and the
conditions under which the GPU tests' inputs (tests/augment_paste_cases.py) have one right answer: every collision and every
point-in-box decision is taken with room to spare, so no compared row rests on rounding and none is excluded."""
import numpy as np
import pytest

import augment_paste_cases as C
import augment_paste_ref as P
import augment_ref as R


def _row(x, y=0.0):
    return [x, y, 1.0, 4.0, 2.0, 1.6, 0.0]                    # 2 m wide along x, 4 m long along y


def _db(rows, counts):
    rows = np.array(rows, dtype=np.float64).reshape(-1, 7)
    counts = np.array(counts, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pts = np.arange(3 * offsets[-1], dtype=np.float32).reshape(-1, 3)
    return dict(boxes=rows, counts=counts, offsets=offsets, points=pts)


def _seed_for(M, want, item=0, epoch=0):
    return next(s for s in range(100000)
                if [P.database_index(R.words(s, 3, item, epoch, k)[0], M) for k in range(len(want))] == want)


def test_index_formula():
    assert P.database_index(0, 1) == 0 and P.database_index(0xffffffff, 1) == 0
    M = 2 ** 20
    assert P.database_index(0, M) == 0 and P.database_index(0xffffffff, M) == M - 1
    assert P.database_index(0x80000000, M) == M // 2 and P.database_index(0x00000fff, M) == 0
    assert P.database_index(0x00001000, M) == 1
    w = [R.words(9, 3, 1, 2, k)[0] for k in range(200)]
    assert all(0 <= P.database_index(v, 17) < 17 for v in w) and len({P.database_index(v, 17) for v in w}) == 17
    assert P.sample_count(3, 10) == 7 and P.sample_count(12, 10) == 0 and P.sample_count(0, 1000) == 64
    assert P.sample_count(448, 1000) == 64
    with pytest.raises(ValueError):
        P.sample_count(449, 1000)


def test_chain_rejected_accepted_rejected():
    """#0 hits a scene box, #1 hits only #0, #2 hits #1: a collision with a REJECTED candidate does not count."""
    scene, db, sample_to, seed = C.sample_case("chain")
    assert P.sample_count(len(scene), sample_to) == 3
    assert R.overlap_area(db["boxes"][0], scene[0]) > 0.1 and R.overlap_area(db["boxes"][1], scene[0]) == 0.0
    assert R.overlap_area(db["boxes"][1], db["boxes"][0]) > 0.1 and R.overlap_area(db["boxes"][2], db["boxes"][1]) > 0.1
    assert R.overlap_area(db["boxes"][2], db["boxes"][0]) == 0.0 and R.overlap_area(db["boxes"][2], scene[0]) == 0.0
    s, _ = C.sample_expected("chain")
    assert s["index"].tolist() == [-1, 1, -1] and s["n_boxes"] == 2
    assert s["point_offset"].tolist() == [0, 0, 7, 7]
    assert np.array_equal(s["boxes_all"], np.concatenate([scene, db["boxes"][1:2], np.zeros((2, 7))]))
    assert s["draws"].tolist() == sum((R.words(seed, 3, 3, 1, k) for k in range(3)), [])


def test_duplicate_and_own_sweep_reject_themselves():
    db = _db([_row(0.0), _row(10.0)], [5, 9])
    seed = _seed_for(2, [1, 1, 0, 1])
    s = P.sample(np.zeros((0, 7)), db, 4, seed)
    assert s["index"].tolist() == [1, -1, 0, -1] and s["n_boxes"] == 2 and s["point_offset"].tolist() == [0, 9, 9, 14, 14]
    assert np.array_equal(s["boxes_all"][:2], db["boxes"][[1, 0]]) and not s["boxes_all"][2:].any()
    # an object of the item's own sweep collides with its original: no special case
    s = P.sample(db["boxes"][:1], db, 4, seed)
    assert s["index"].tolist() == [1, -1, -1, -1] and s["n_boxes"] == 2
    # an empty database samples nothing, and draws all the same
    s = P.sample(db["boxes"], _db([], []), 3, seed)
    assert s["index"].tolist() == [-1] * 3 and s["n_boxes"] == 2 and not s["point_offset"].any() and s["draws"].all()


def test_paste_row_layout_and_bound():
    db = _db([_row(0.0), _row(10.0), _row(20.0)], [5, 9, 2])
    assert [P.bound(db, k) for k in range(5)] == [0, 9, 14, 16, 16]
    seed = _seed_for(3, [2, 0, 2])
    scene = np.array([_row(30.0)])
    s = P.sample(scene, db, 3, seed)
    assert s["index"].tolist() == [2, 0, -1]
    pts = np.array([[30.0, 0, 1], [0.2, 1.0, 1.2], [20.0, 0.0, 1.79], [20.0, 0.0, 1.81], [1.0e6, 5, 5], [-1.0e6, 0, 1]],
                   dtype=np.float32)
    out, removed = P.paste(pts, db, s, 1, cap=6 + 16 + 2)
    assert removed.tolist() == [False, True, True, False, False, False]          # inside object 0 / 2; z above; pad rows
    assert out.dtype == np.float32 and out.shape == (24, 3)
    assert np.array_equal(out[[0, 3, 4, 5]], pts[[0, 3, 4, 5]]) and np.all(out[[1, 2]] == 1.0e6)
    assert np.array_equal(out[6:8], db["points"][14:16]) and np.array_equal(out[8:13], db["points"][0:5])
    assert np.all(out[13:] == 1.0e6) and P.PAD == 1.0e6


def test_build_database_keeps_the_owned_points_in_order():
    pts, boxes = C.database_sweeps("f32")
    own = P.owner(pts[0], boxes[0])
    counts = [int((own == j).sum()) for j in range(len(boxes[0]))]
    assert counts[0] == 0 and counts[1] == C.MIN_POINTS and counts[2] == C.MIN_POINTS - 1 and counts[3] > 256
    assert [600 <= len(p) <= 2000 for p in pts] == [True] * 3 and [4 <= len(b) <= 9 for b in boxes] == [True] * 3
    db = C.database("f32")
    kept0 = [j for j in range(len(boxes[0])) if counts[j] >= C.MIN_POINTS]
    assert 0 not in kept0 and 2 not in kept0 and 1 in kept0 and 3 in kept0
    assert np.array_equal(db["boxes"][:len(kept0)], boxes[0][kept0])
    assert np.array_equal(db["points"][:C.MIN_POINTS], pts[0][own == 1]) and db["points"].dtype == np.float32
    assert db["offsets"][0] == 0 and np.array_equal(np.diff(db["offsets"]), db["counts"]) and db["counts"].min() >= C.MIN_POINTS
    assert db["counts"].max() > 256 and db["offsets"][-1] == len(db["points"]) and len(db["boxes"]) >= 10
    mixed = C.database("mixed")
    assert mixed["points"].dtype == np.float64 and np.array_equal(mixed["counts"], db["counts"])
    assert np.array_equal(mixed["points"][:db["offsets"][len(kept0)]], db["points"][:db["offsets"][len(kept0)]].astype(np.float64))


# ---- the committed cases have one right answer ----------------------------------------------------------------------------
def _clear(points, boxes):
    points = np.asarray(points)[:, :3].astype(np.float64)
    live = np.abs(points[:, 0]) < R.PAD_LIMIT
    if len(boxes) and live.any():
        assert R.face_margins(points[live], boxes).min() > 1e-6


@pytest.mark.parametrize("name", C.OWNER_CASES)
def test_owner_cases_are_clear_of_every_face(name):
    pts, boxes = C.owner_case(name)
    _clear(pts, boxes)
    own = P.owner(pts, boxes)
    if name in ("b7", "b130", "f32", "strided", "pad"):
        assert (own >= 0).sum() >= 100 and (own < 0).sum() >= 100
    if name == "b130":
        assert own.max() >= 128                               # the second LDS chunk owns points too
    if name == "b7":
        assert ((own == 0) & (R.owner(pts, boxes[1:2]) == 0)).sum() >= 3          # shared points go to the lower index
    if name == "pad":
        assert np.all(own[-100:] == -1)


@pytest.mark.parametrize("name", C.DATABASE_CASES)
def test_database_sweeps_are_clear_of_every_face(name):
    for p, b in zip(*C.database_sweeps(name)):
        _clear(p, b)


@pytest.mark.parametrize("name", C.SAMPLE_CASES)
def test_sample_decisions_are_unambiguous(name):
    seen = []
    for item, epoch in ((3, 1), (3, 2), (4, 1)):
        s, decisions = C.sample_expected(name, item, epoch)
        for ar, sep in decisions:
            assert (ar == 0.0 and sep > 1e-6) or ar > 1e-6, (ar, sep)
        seen.append(s)
    s = seen[0]
    K = len(s["index"])
    assert K == {"k0": 0, "m0": 3, "m1": 3, "b0": 6, "chain": 3, "crowded": 24, "k64": 64}[name]
    if name == "m1":
        assert s["index"].tolist() == [0, -1, -1]
    if name in ("crowded", "k64"):
        assert (s["index"] >= 0).any() and (s["index"] < 0).any()
    if K and name != "m0":
        assert not np.array_equal(seen[0]["draws"], seen[1]["draws"]) and not np.array_equal(seen[0]["draws"], seen[2]["draws"])


@pytest.mark.parametrize("name", C.PASTE_CASES)
def test_paste_cases_are_clear_of_every_pasted_face(name):
    c = C.paste_case(name)
    s = c["sample"]
    _clear(c["points"], s["boxes_all"][len(c["boxes"]):s["n_boxes"]])
    assert s["n_boxes"] > len(c["boxes"]) and c["cap"] >= len(c["points"]) + s["point_offset"][-1]
    if name not in ("n0",):
        assert c["removed"].sum() > 0
    if name == "big":
        assert (c["db"]["counts"][s["index"][s["index"] >= 0]] > 256).any()
    if name == "pad":
        assert not c["removed"][-200:].any()
    assert np.all(c["want"][len(c["points"]) + s["point_offset"][-1]:] == 1.0e6)


def test_item_case_is_unambiguous():
    pts, scene, db = C.item_case()
    for item, epoch in (C.ITEM_AT,):
        out, boxes, smp, pasted = C.item_expected(item, epoch)
        decisions = []
        P.sample(scene, db, len(smp["index"]), C.SEED, item, epoch, decisions=decisions)
        R.draw(smp["boxes_all"][:smp["n_boxes"]], C.SEED, item, epoch, decisions=decisions)
        for ar, sep in decisions:
            assert (ar == 0.0 and sep > 1e-6) or ar > 1e-6, (ar, sep)
        _clear(pts, smp["boxes_all"][:smp["n_boxes"]])         # removal, and the scene points' owners in apply
        _clear(pasted, smp["boxes_all"][:smp["n_boxes"]])      # the pasted points' owners in apply
        assert smp["n_boxes"] > len(scene) and len(boxes) == smp["n_boxes"] and out.shape == pasted.shape
        # the label maps: every box has positive anchors (which anchor a box WITHOUT one is given rests on rounding: a
        # footprint inside two neighbouring anchors has the same IoU with both) and no IoU sits on a threshold
        least_best, least_gap = P.label_margins(boxes)
        assert least_best > 1e-6 and least_gap > 1e-6, (least_best, least_gap)


def test_fit_case_is_unambiguous():
    """The sweeps Model.fit trains on in tests/test_gpu_augment_paste.py: objects are accepted in both epochs, and every
    decision behind the staged points of epoch 1 is clear of rounding."""
    import augment_cases as C0
    pts, bxs = C0.fit_sweeps()
    db = P.build_database(pts, bxs)
    for p, b in zip(pts, bxs):
        _clear(p, b)
    for epoch in (0, 1):
        accepted = 0
        for i in range(3):
            out, boxes, smp, pasted = P.item(pts[i], bxs[i], db, C.FIT_SAMPLE_TO, C.FIT_SEED, i, epoch)
            accepted += smp["n_boxes"] - len(bxs[i])
            decisions = []
            P.sample(bxs[i], db, len(smp["index"]), C.FIT_SEED, i, epoch, decisions=decisions)
            R.draw(smp["boxes_all"][:smp["n_boxes"]], C.FIT_SEED, i, epoch, decisions=decisions)
            for ar, sep in decisions:
                assert (ar == 0.0 and sep > 1e-6) or ar > 1e-6, (ar, sep)
            _clear(pts[i], smp["boxes_all"][:smp["n_boxes"]])
            _clear(pasted, smp["boxes_all"][:smp["n_boxes"]])
        assert accepted >= 1
