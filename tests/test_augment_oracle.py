"""The numpy oracle of the training-time augmentation (tests/augment_ref.py) against known answers and its own
definitions, and the conditions under which the GPU tests' inputs (tests/augment_cases.py) have one right answer."""
import math

import numpy as np
import pytest

import augment_cases as C
import augment_ref as R


def test_philox4x32_10_known_answers():
    """The published vectors of Random123 (kat_vectors: philox4x32 10)."""
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 0xffffffff
    assert R.philox4x32_10((ones,) * 4, (ones,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert 0.0 < R.uniform(0) < R.uniform(ones) < 1.0
    # key = the 64-bit seed, low word first; every counter word matters
    base = R.words(5 << 32 | 9, 1, 2, 3, 4)
    assert base == R.philox4x32_10((1, 2, 3, 4), (9, 5))
    assert all(R.words(5 << 32 | 9, *c) != base for c in ((0, 2, 3, 4), (1, 0, 3, 4), (1, 2, 0, 4), (1, 2, 3, 0)))


def _rotate(xy, alpha, s):
    cs, sn = math.cos(alpha), math.sin(alpha)
    return [(s * (x * cs - y * sn), s * (x * sn + y * cs)) for x, y in xy]


@pytest.mark.parametrize("name", ["b1", "b7", "crowded"])
def test_returned_row_has_the_transformed_corners(name):
    """box_corners of the new row = the old row's corners moved by the box's transform, then rotated counter-clockwise by
    alpha and scaled: with u = (cos yaw, -sin yaw) that is yaw - alpha."""
    d, _ = C.draw_expected(name)
    before = C.draw_case(name)
    for b in range(len(before)):
        per = R.footprint(d["perturbed"][b])
        # the per-box stage: the frame coordinates of the corners are kept
        u, v = R.box_frame(before[b])
        nu, nv = R.box_frame(d["perturbed"][b])
        for old, new in zip(R.footprint(before[b]), per):
            du, dv = np.dot(np.array(old) - before[b, :2], u), np.dot(np.array(old) - before[b, :2], v)
            assert np.allclose(d["perturbed"][b, :2] + du * nu + dv * nv, new, atol=1e-12)
        assert np.allclose(R.footprint(d["boxes"][b]), _rotate(per, d["alpha"], d["scale"]), atol=1e-12)
        assert np.allclose(d["boxes"][b, 3:6], d["scale"] * before[b, 3:6]) and d["boxes"][b, 2] == d["scale"] * d["perturbed"][b, 2]
    # and the points of a box move with its corners: a corner pulled in by 1 % lands at the new corner pulled in by 1 %
    pts = np.array([[*(before[b, :2] + 0.99 * (np.array(c) - before[b, :2])), before[b, 2]] for b in range(len(before))
                    for c in R.footprint(before[b])])
    own = R.owner(pts, before)
    moved = R.apply(pts, before, d["transforms"], d["scale"], d["alpha"])
    for k, b in enumerate(np.repeat(np.arange(len(before)), 4)):
        if own[k] == b:
            want = d["boxes"][b, :2] + 0.99 * (np.array(R.footprint(d["boxes"][b])[k % 4]) - d["boxes"][b, :2])
            assert np.allclose(moved[k, :2], want, atol=1e-9)


@pytest.mark.parametrize("name", C.DRAW_CASES)
def test_accepted_pose_intersects_no_other_box(name):
    d, _ = C.draw_expected(name)
    before, per = C.draw_case(name), d["perturbed"]
    for b in np.nonzero(d["attempt"] >= 0)[0]:
        for j in range(len(per)):
            # later boxes had not moved yet when b was placed, earlier ones had
            other = per[j] if j < b else before[j]
            assert j == b or R.overlap_area(per[b], other) == 0.0
    stayed = d["attempt"] < 0
    assert np.array_equal(per[stayed], before[stayed]) and not d["transforms"][stayed].any()
    if name == "crowded":
        assert stayed.any() and (~stayed).any()              # some boxes exhaust their attempts, some find room
    elif len(before):
        assert (~stayed).any()


def test_identity_parameters_return_the_inputs():
    boxes = C.draw_case("b7")
    pts = C.apply_case("b7")["points"]
    for params in (R.IDENTITY, dict(R.IDENTITY, attempts=10)):
        d = R.draw(boxes, 5, 1, 2, **params)
        assert np.array_equal(d["boxes"], boxes) and d["scale"] == 1.0 and d["alpha"] == 0.0
        assert np.array_equal(R.apply(pts, boxes, d["transforms"], d["scale"], d["alpha"]), pts)
    # one stage at a time
    d = R.draw(boxes, 5, 1, 2, **dict(R.IDENTITY, scale=(0.9, 1.1)))
    assert np.array_equal(d["boxes"][:, 6], boxes[:, 6]) and np.allclose(d["boxes"][:, :6], d["scale"] * boxes[:, :6], rtol=1e-15)
    d = R.draw(boxes, 5, 1, 2, **dict(R.IDENTITY, rot_global=0.5))
    assert np.array_equal(d["boxes"][:, 2:6], boxes[:, 2:6]) and d["alpha"] != 0.0


@pytest.mark.parametrize("name", C.DRAW_CASES)
def test_collision_decisions_of_the_gpu_cases_are_unambiguous(name):
    """Every test the walk makes is decided with room to spare: area 0 with the footprints >= 1e-6 m apart, or an area
    above 1e-6 m^2 -- so rounding in the kernel's own clipping cannot flip one."""
    for item, epoch in ((3, 1), (3, 2), (4, 1)):
        _, decisions = C.draw_expected(name, item, epoch)
        assert name == "b0" or name == "b1" or decisions
        for ar, sep in decisions:
            assert (ar == 0.0 and sep >= 1e-6) or ar > 1e-6, (ar, sep)


@pytest.mark.parametrize("name", C.APPLY_CASES)
def test_points_of_the_gpu_cases_are_clear_of_every_face(name):
    c = C.apply_case(name)
    pts = c["points"][:, :3].astype(np.float64)
    live = np.abs(pts[:, 0]) < R.PAD_LIMIT
    if len(c["boxes"]) and live.any():
        assert R.face_margins(pts[live], c["boxes"]).min() >= 1e-6
    own = R.owner(pts[live], c["boxes"])
    if name == "b7":
        shared = (R.owner(pts, c["boxes"][1:2]) == 0) & (own == 0)
        assert shared.sum() >= 5                              # points inside both overlapping boxes: index 0 owns them
    if len(c["boxes"]) and len(pts):
        assert (own >= 0).sum() >= 100 and (own < 0).sum() >= 100
    want = C.apply_expected(name)
    assert np.array_equal(want[~live], pts[~live]) and want.shape == pts.shape


def test_balance_keeps_the_smallest_keys():
    rng = np.random.default_rng(3)
    valid = (rng.uniform(size=(8, 16, 2)) < 0.8).astype(np.float64)
    overlap = ((rng.uniform(size=(8, 16, 2)) < 0.2) & (valid == 1)).astype(np.float64)
    pos, neg = int(((valid == 1) & (overlap == 1)).sum()), int(((valid == 1) & (overlap == 0)).sum())
    out = R.balance_keep(valid, overlap, 16, seed=1, item=2, epoch=3)
    assert pos > 8 and neg > 8
    assert int(((out == 1) & (overlap == 1)).sum()) == 8 and int(((out == 1) & (overlap == 0)).sum()) == 8
    assert np.all(out <= valid) and np.array_equal(out, R.balance_keep(valid, overlap, 16, seed=1, item=2, epoch=3))
    assert not np.array_equal(out, R.balance_keep(valid, overlap, 16, seed=1, item=2, epoch=4))
    assert np.array_equal(R.balance_keep(valid, overlap, 1024), valid)          # nothing to drop
    # no positives: the reference keeps as many negatives as positives -- none
    assert not R.balance_keep(valid, np.zeros_like(valid), 16).any()
