"""The test-local oracle of the union / overlap areas (tests/union_overlap_ref.py: inclusion-exclusion over the convex
pieces P_i n L_j) against hand-computed answers and an independent Monte-Carlo estimate.  shapely, which the reference's
calcIntersectAll delegates to (rpnToRegion.py:202-213), is absent: these pin the yardstick the GPU tests use."""
import math

import numpy as np
import pytest

import union_overlap_ref as R


def _box(x, y, l, w, yaw=0.0, z=1.0, h=1.5):
    """Rows are x, y, z, l, w, h, yaw; at yaw 0 the WIDTH lies along x and the length along y (serialize_data.py:151-163)."""
    return [x, y, z, l, w, h, yaw]


def test_two_offset_unit_squares_against_a_2x2_square():
    # P: [-0.5,0.5]^2 and the same moved by (0.5, 0): union = [-0.5,1] x [-0.5,0.5], area 1.5.  L: [0,2]^2.
    P = [_box(0, 0, 1, 1), _box(0.5, 0, 1, 1)]
    L = [_box(1, 1, 2, 2)]
    got = R.union_overlap(P, L)
    assert got[0] == pytest.approx(1.0 * 0.5, rel=1e-14)       # [0,1] x [0,0.5]
    assert got[1] == pytest.approx(1.5, rel=1e-14)
    assert got[2] == pytest.approx(4.0, rel=1e-14)
    assert got[3] == pytest.approx(2 * 1.5, rel=1e-14) and got[4] == pytest.approx(4 * 1.5, rel=1e-14)


def test_rotated_square_inside_a_square():
    # a square of side sqrt(2) turned by 45 degrees has its corners at (+-1, 0), (0, +-1): inside [-1.5,1.5]^2, area 2
    P = [_box(0, 0, math.sqrt(2), math.sqrt(2), math.pi / 4)]
    L = [_box(0, 0, 3, 3)]
    got = R.union_overlap(P, L)
    assert got[0] == pytest.approx(2.0, rel=1e-14) and got[1] == pytest.approx(2.0, rel=1e-14)
    assert got[2] == pytest.approx(9.0, rel=1e-14)
    assert R.union_overlap(L, P)[0] == pytest.approx(2.0, rel=1e-14)


def test_plus_sign_under_a_covering_square():
    # two 3 x 1 bars crossing at right angles: 2 * 3 * 1 - 1 = 5, all of it under the 4 x 4 square
    P = [_box(0, 0, 1, 3), _box(0, 0, 3, 1)]
    L = [_box(0, 0, 4, 4)]
    got = R.union_overlap(P, L)
    assert got[0] == pytest.approx(5.0, rel=1e-14) and got[1] == pytest.approx(5.0, rel=1e-14)
    # the same plus drawn with one bar turned by pi/2 instead of swapped sides
    P2 = [_box(0, 0, 1, 3), _box(0, 0, 1, 3, math.pi / 2)]
    assert R.union_overlap(P2, L)[0] == pytest.approx(5.0, rel=1e-13)


def test_degenerate_inputs():
    sq = _box(0, 0, 2, 2)
    assert R.union_overlap([sq, sq], [sq])[:3] == pytest.approx([4.0, 4.0, 4.0], rel=1e-14)      # a duplicate counts once
    assert R.union_overlap([_box(0, 0, 0, 2)], [sq])[0] == 0.0                                  # zero length: no footprint
    assert R.union_overlap([_box(0, 0, -2, 2)], [sq])[0] == pytest.approx(4.0, rel=1e-14)       # mirrored, same area
    assert list(R.union_overlap([], [sq])[:3]) == [0.0, 0.0, 4.0]
    assert R.union_overlap([_box(2, 2, 2, 2)], [sq])[0] == 0.0                                  # corner touch
    with pytest.raises(ValueError):
        R.union_overlap([_box(0.01 * i, 0, 2, 2) for i in range(13)], [])                       # beyond the cluster limit


def _inside(pts, box):
    th = box[6]
    u = np.array([math.cos(th), -math.sin(th)])                # width axis; v = length axis
    v = np.array([math.sin(th), math.cos(th)])
    d = pts - np.array(box[:2])
    return (np.abs(d @ u) <= abs(box[4]) / 2) & (np.abs(d @ v) <= abs(box[3]) / 2)


def test_random_scenes_vs_monte_carlo():
    """3 + 3 rotated boxes in a 10 x 10 window against N uniform points; each area within 4 sigma of the binomial
    estimate, sigma = sqrt(p (1 - p) / N) * window area."""
    rng = np.random.default_rng(0)
    N, window = 400000, 100.0
    for _ in range(6):
        def side():
            return [[rng.uniform(-2, 2), rng.uniform(-2, 2), 1.0, rng.uniform(1, 4), rng.uniform(1, 4), 1.5,
                     rng.uniform(-3.2, 3.2)] for _ in range(3)]
        P, L = side(), side()
        got = R.union_overlap(P, L)
        pts = rng.uniform(-5, 5, (N, 2))
        in_p = np.any([_inside(pts, b) for b in P], axis=0)
        in_l = np.any([_inside(pts, b) for b in L], axis=0)
        for value, hit in ((got[0], in_p & in_l), (got[1], in_p), (got[2], in_l)):
            p = hit.mean()
            assert abs(value - p * window) <= 4 * math.sqrt(p * (1 - p) / N) * window, (value, p * window)


def test_clusters_add_up():
    """The cluster split changes nothing: a clustered scene equals the sum of its clusters scored one by one."""
    rng = np.random.default_rng(1)
    P, L = R.clustered_scene(rng, 6, 6, 3)
    whole = R.union_overlap(P, L)
    parts = sum(R.union_overlap(P[c::3], L[c::3]) for c in range(3))
    assert whole == pytest.approx(parts, rel=1e-13)
