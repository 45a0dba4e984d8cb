"""Edge cases of the label and NMS kernels of csrc/boxes.hip (lisec_rpn_labels, lisec_rpn_to_region) -- TEST ONLY.
tests/test_box_edge_cases.py checks on the CPU that every case still takes the path it was written for;
tests/test_gpu_box_edges.py runs the same cases through the C ABI.  label_case(name) / nms_case(name) build a case once per
process, run oracle/boxes_ref.py on it once and assert, on the oracle alone, the conditions under which a comparison with the
kernels can neither hide nor invent a failure:

  * exact cases (EXACT: dyadic anchors at yaw 0, box rows multiples of 2^-2 at yaw 0): every IoU of the oracle equals the
    correctly rounded value of the IoU in rational arithmetic, so a tie there is a tie of the exact values;
  * other cases: each box's largest anchor IoU, and each positive anchor's largest box IoU, lies MARGIN (relative) above the
    runner-up; no IoU lies within MARGIN of iou_lo, iou_hi or the overlap threshold;
  * all cases: no IoU other than an exact 0 is smaller than MARGIN in magnitude, and no NMS candidate's x -+ ax, y -+ ay
    lies within MARGIN of the range bounds 0 and 100;
  * the path the case is named for is the one the oracle takes (LABEL_PATHS, _check_nms_path).
"""
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import boxes_ref as B

IOU_LO, IOU_HI = 0.45, 0.6                                     # Constants.iouLowerBound / iouUpperBound
MARGIN = 1e-9
REF_ANCHORS = [[1.6, 3.9, 1.56, 0.0], [1.6, 3.9, 1.56, math.pi / 2]]
# vx = 1.0, vy = 0.5 as in the reference (2 * voxelx, 2 * voxely)
EXACT = dict(name="exact", outX=12, outY=24, vx=1.0, vy=0.5, anchors=[[2.0, 4.0, 1.5, 0.0], [4.0, 2.0, 1.5, 0.0]], exact=True)
REF12 = dict(name="ref12", outX=12, outY=24, vx=1.0, vy=0.5, anchors=REF_ANCHORS, exact=False)      # 576 = 4.5 x 128 = 2.25 x 256
REF16 = dict(name="ref16", outX=16, outY=40, vx=1.0, vy=0.5, anchors=REF_ANCHORS, exact=False)      # 1280 > 1024


def oracle_grid(cfg):
    """The grid of a configuration as oracle/boxes_ref.py takes it (it halves nx, ny and doubles the voxel sizes)."""
    return dict(nx=2 * cfg["outX"], ny=2 * cfg["outY"], voxelx=cfg["vx"] / 2, voxely=cfg["vy"] / 2, anchors=cfg["anchors"])


def candidates(cfg):
    return 2 * cfg["outX"] * cfg["outY"]


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def anchor_box(cfg, order):
    """(in_range, [cX, cY, 1, l, w, h, yaw], (xV, yV, a)) of the anchor at position `order` of the reference's loop nest
    (anchor, xVoxel, yVoxel; serialize_data.py:219-232), with its expressions."""
    outX, outY, vx, vy = cfg["outX"], cfg["outY"], cfg["vx"], cfg["vy"]
    a, m = divmod(order, outX * outY)
    xV, yV = m // outY + int(-outX / 2), m % outY + int(-outY / 2)
    an = cfg["anchors"][a]
    cX, cY = vx * xV + vx / 2, vy * yV + vy / 2
    out = (cX - an[0] / 2 < vx * int(-outX / 2) or cX + an[0] / 2 > vx * int(outX / 2) or
           cY - an[1] / 2 < vy * int(-outY / 2) or cY + an[1] / 2 > vy * int(outY / 2))
    return (not out), [cX, cY, 1.0] + list(an), (xV, yV, a)


def iou_table(cfg, fixed):
    """(2 * outX * outY, B) float64: calculate_iou of every in-range anchor with every box, rows in loop order, NaN rows for
    the anchors the reference skips.  The far shortcut is preprocess_labels' own."""
    T = np.full((candidates(cfg), len(fixed)), np.nan)
    rad = [0.5 * math.hypot(b[3], b[4]) for b in fixed]
    with np.errstate(divide="ignore"):
        for order in range(candidates(cfg)):
            ok, ab, _ = anchor_box(cfg, order)
            if not ok:
                continue
            arad = 0.5 * math.hypot(ab[3], ab[4])
            for b, fb in enumerate(fixed):
                far = math.hypot(fb[0] - ab[0], fb[1] - ab[1]) > rad[b] + arad
                T[order, b] = 0.0 if far else B.calculate_iou(ab, fb)
    return T


def rational_iou(ab, fb):
    """calculateIoU of two yaw-0 boxes in rational arithmetic (the footprint is w along x and l along y), as a float: inf
    where the union is 0."""
    ab, fb = [Fraction(v) for v in ab], [Fraction(v) for v in fb]
    ox = min(ab[0] + ab[4] / 2, fb[0] + fb[4] / 2) - max(ab[0] - ab[4] / 2, fb[0] - fb[4] / 2)
    oy = min(ab[1] + ab[3] / 2, fb[1] + fb[3] / 2) - max(ab[1] - ab[3] / 2, fb[1] - fb[3] / 2)
    area = max(ox, 0) * max(oy, 0)
    inter = (min(ab[2] + ab[5], fb[2] + fb[5]) - max(ab[2] - ab[5], fb[2] - fb[5])) * area
    uni = ab[3] * ab[4] * ab[5] + fb[3] * fb[4] * fb[5] - inter
    if uni == 0:
        return math.copysign(math.inf, inter)
    return float(inter / uni)


def _dyadic(v, q=4):
    return float(v) * q == math.floor(float(v) * q)


FIXUP_TIE = [0.5, 0.25, 1.25, 4.5, 8.0, 1.5, 0.0]


def _lattice65():
    """65 boxes on a jittered 5 x 13 lattice inside the 16 x 40 grid (x in -8 .. 8, y in -10 .. 10).  Each is longer and
    narrower than the anchors (1.6, 3.9): a box that holds an anchor, or lies inside one, has the same IoU with every anchor
    it holds or lies in up to rounding, and its maximum would not stand alone.  Every eighth box floats about 2 m above the
    anchors: its IoUs stay below iou_hi, so it takes the fixup path among 64 others."""
    rng = np.random.default_rng(14)                            # chosen on the oracle: the conditions of the header hold
    rows = []
    for i in range(5):
        for j in range(13):
            rows.append([-6.0 + 3.0 * i + rng.uniform(-0.4, 0.4), -8.4 + 1.4 * j + rng.uniform(-0.3, 0.3),
                         (3.0 + rng.uniform(0, 0.3)) if (i * 13 + j) % 8 == 3 else rng.uniform(0.5, 1.5),
                         rng.uniform(1.7, 2.0), rng.uniform(3.5, 3.8), rng.uniform(1.3, 1.8),
                         float(rng.choice([0.0, math.pi / 2, 0.1, -0.2, 1.4]))])
    return rows


def _first_best(cfg, box):
    """The anchor box of the first anchor in loop order that attains `box`'s largest IoU."""
    T = iou_table(cfg, [box])[:, 0]
    return anchor_box(cfg, int(np.flatnonzero(T == np.nanmax(T))[0]))[1]


LABEL_CASES = {
    # name: (configuration, fixed boxes: rows x, y, z, l, w, h, yaw ALREADY scaled by fixBoxScaling, as lisec_rpn_labels takes them)
    "coincident": lambda: (EXACT, [[0.5, 0.25, 1.0, 2.0, 4.0, 1.5, 0.0]]),
    "z_apart": lambda: (EXACT, [[0.5, 0.25, 9.0, 2.0, 4.0, 1.5, 0.0]]),
    "outside": lambda: (EXACT, [[40.0, 40.0, 1.0, 2.0, 4.0, 1.5, 0.0]]),
    "fixup_tie": lambda: (EXACT, [FIXUP_TIE]),
    "shared_fixup": lambda: (EXACT, [FIXUP_TIE, [0.5, 0.25, 1.0, 4.5, 8.0, 1.75, 0.0]]),
    "fixup_over_neutral": lambda: (EXACT, [FIXUP_TIE, _first_best(EXACT, FIXUP_TIE)]),
    "border_wrap": lambda: (REF12, [[-5.0, -4.0, 1.1, 1.7, 3.8, 1.5, 0.1], [5.0, 4.0, 0.9, 1.8, 4.0, 1.6, -0.2]]),
    "many": lambda: (REF16, _lattice65()),
    "empty": lambda: (EXACT, []),
}


def _check_label_conditions(c):
    cfg, fixed, T = c["cfg"], c["fixed"], c["table"]
    live = ~np.isnan(T[:, 0]) if len(fixed) else np.zeros(candidates(cfg), dtype=bool)
    if not len(fixed):
        return
    V = T[live]
    if cfg["exact"]:
        assert all(_dyadic(v) for an in cfg["anchors"] for v in an) and all(an[3] == 0 for an in cfg["anchors"])
        assert all(_dyadic(v) for row in fixed for v in row) and all(row[6] == 0 for row in fixed)
        for order in np.flatnonzero(live):
            ab = anchor_box(cfg, int(order))[1]
            for b, fb in enumerate(fixed):
                want = rational_iou(ab, fb)
                assert T[order, b] == want, f"{c['name']}: anchor {order} box {b}: oracle {T[order, b]!r}, exact {want!r}"
    else:
        for b in range(len(fixed)):                            # the largest anchor IoU of a box stands alone
            col = np.sort(V[:, b])
            if col[-1] > 0:
                assert col[-1] - col[-2] >= MARGIN * col[-1], f"{c['name']}: box {b}: maxima {col[-1]!r}, {col[-2]!r}"
        if len(fixed) > 1:                                     # and so does the largest box IoU of a positive anchor
            top = np.sort(V, axis=1)
            pos = top[:, -1] >= IOU_HI
            assert np.all(top[pos, -1] - top[pos, -2] >= MARGIN * top[pos, -1]), c["name"]
        for t in (IOU_LO, IOU_HI):
            assert np.abs(V - t).min() >= MARGIN, f"{c['name']}: an IoU within {MARGIN} of {t}"
    assert np.all((V == 0) | (np.abs(V) >= MARGIN)), f"{c['name']}: an IoU below {MARGIN} in magnitude that is not 0"


def fixup_facts(c):
    """Per box: count of anchors at iou >= IOU_HI, the largest IoU, the loop orders that attain it bit for bit."""
    T = c["table"]
    out = []
    for b in range(len(c["fixed"])):
        col = T[:, b]
        mx = np.nanmax(col)
        out.append(dict(count=int(np.nansum(col >= IOU_HI)), best=float(mx), ties=[int(o) for o in np.flatnonzero(col == mx)]))
    return out


def cell_of(cfg, order):
    """(ix, iy, a) of the output element an anchor writes: negative voxel indices wrap (serialize_data.py:284-294)."""
    xV, yV, a = anchor_box(cfg, order)[2]
    return xV % cfg["outX"], yV % cfg["outY"], a


def positive_cells(c):
    return {tuple(int(v) for v in i) for i in np.argwhere(c["cls"] == 2)}


def _row(c, cell):
    return c["reg"][cell[0], cell[1], 7 * cell[2]:7 * cell[2] + 7]


def _live(cfg):
    return np.array([anchor_box(cfg, o)[0] for o in range(candidates(cfg))])


def _path_empty(c):
    live = _live(c["cfg"])
    want = np.zeros_like(c["cls"])
    for o in np.flatnonzero(live):
        want[cell_of(c["cfg"], int(o))] = 1.0
    assert len(c["fixed"]) == 0 and 0 < live.sum() < len(live) and np.array_equal(c["cls"], want) and not c["reg"].any()


def _path_no_overlap(c):
    """No positive, no neutral, no fixup: the maps of the empty scene."""
    V = c["table"][_live(c["cfg"]), 0]
    if c["name"] == "z_apart":
        assert (V < 0).any() and not (V > 0).any(), "z_apart: the IoUs are to be negative, or 0 far away"
    else:
        assert np.all(V == 0.0), "outside: every IoU is to be exactly 0"
    assert np.array_equal(c["cls"], label_case("empty")["cls"]) and not c["reg"].any()


def _path_coincident(c):
    (f,) = fixup_facts(c)
    assert f["best"] == math.inf and len(f["ties"]) == 1 and f["count"] > 1
    cell = cell_of(c["cfg"], f["ties"][0])
    assert c["cls"][cell] == 2 and np.array_equal(_row(c, cell), np.ones(7))         # regression 0 + overlap 1


def _path_fixup_tie(c):
    (f,) = fixup_facts(c)
    M = candidates(c["cfg"]) // 2
    assert f["count"] == 0, "fixup_tie: the box is to have no anchor at iou_hi or above"
    assert f["best"] == 0.5 and len(f["ties"]) == 32
    assert f["ties"][0] < M <= f["ties"][-1], "the maxima are to span both anchors"
    assert f["ties"][0] // 128 != f["ties"][-1] // 128, "and more than one workgroup"
    first = cell_of(c["cfg"], f["ties"][0])
    assert positive_cells(c) == {first}
    assert all(c["cls"][cell_of(c["cfg"], o)] == 0 for o in f["ties"][1:]), "the other maxima stay neutral (0.45 < 0.5 <= 0.6)"
    ab, fb = anchor_box(c["cfg"], f["ties"][0])[1], c["fixed"][0]
    want = [(fb[0] - ab[0]) / ab[3], (fb[1] - ab[1]) / ab[4], (fb[2] - ab[2]) / ab[5], math.log(fb[3] / ab[3]),
            math.log(fb[4] / ab[4]), math.log(fb[5] / ab[5]), fb[6] - ab[6]]
    assert np.array_equal(_row(c, first), np.asarray(want) + 1.0)


def _path_shared_fixup(c):
    f0, f1 = fixup_facts(c)
    assert f0["count"] == f1["count"] == 0 and f0["best"] > 0 and f1["best"] > 0 and f0["best"] != f1["best"]
    assert f0["ties"][0] == f1["ties"][0] and len(f1["ties"]) > 1, "both boxes are to fix up to one anchor"
    cell = cell_of(c["cfg"], f0["ties"][0])
    assert positive_cells(c) == {cell}
    row, single = _row(c, cell), _row(label_case("fixup_tie"), cell)
    assert row[2] == 1.0 and row[5] == 1.0 + math.log(1.75 / 1.5), "box 1 (z = 1, h = 1.75) is the one whose regression stays"
    assert single[2] != row[2] and single[5] != row[5]


def _path_fixup_over_neutral(c):
    f0, f1 = fixup_facts(c)
    assert f0["count"] == 0 and f0["best"] == 0.5 and f1["count"] > 0
    target = f0["ties"][0]
    assert c["table"][target, 1] == math.inf and f1["ties"] == [target], "box 1 coincides with box 0's fixup anchor"
    cell = cell_of(c["cfg"], target)
    assert c["cls"][cell] == 2 and len(positive_cells(c)) == f1["count"]
    row = _row(c, cell)
    assert row[2] == 1.0 + 0.25 / 1.5 and row[3] == 1.0 + math.log(4.5 / 2.0), "box 0's fixup overwrites box 1's zero regression"


def _path_border_wrap(c):
    cfg, pos = c["cfg"], positive_cells(c)
    assert any(ix >= cfg["outX"] // 2 and iy >= cfg["outY"] // 2 for ix, iy, _ in pos), "a positive at negative xVoxel AND yVoxel"
    assert any(ix < cfg["outX"] // 2 and iy < cfg["outY"] // 2 for ix, iy, _ in pos)
    assert all(f["count"] > 0 for f in fixup_facts(c))


def _path_many(c):
    facts = fixup_facts(c)
    assert len(facts) == 65 and c["cfg"]["name"] == "ref16"
    fix = [f for f in facts if f["count"] == 0 and f["best"] > 0]
    assert len(fix) >= 4 and len(facts) - len(fix) >= 32 and facts[64]["best"] > 0
    assert all(len(f["ties"]) == 1 for f in facts)
    assert len({round(float(y), 6) for y in c["fixed"][:, 6]}) == 5, "mixed yaws"
    assert all(c["cls"][cell_of(c["cfg"], f["ties"][0])] == 2 for f in fix)


LABEL_PATHS = dict(coincident=_path_coincident, z_apart=_path_no_overlap, outside=_path_no_overlap, fixup_tie=_path_fixup_tie,
                   shared_fixup=_path_shared_fixup, fixup_over_neutral=_path_fixup_over_neutral, border_wrap=_path_border_wrap,
                   many=_path_many, empty=_path_empty)


def build_label_case(name, cfg, rows):
    """The case `name` on the given boxes: the oracle's maps, with the conditions of the header and the path of `name`
    asserted."""
    fixed = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    data = fixed.copy()                                        # undo fixBoxScaling: a factor 2, exact
    data[:, [0, 1, 3, 4]] *= 2.0
    with np.errstate(divide="ignore"):
        cls, reg = B.preprocess_labels(data, iou_lo=IOU_LO, iou_hi=IOU_HI, balance=False, **oracle_grid(cfg))
    c = dict(name=name, cfg=cfg, fixed=fixed, table=iou_table(cfg, fixed), cls=cls, reg=reg,
             valid=(cls >= 1).astype(np.float64), overlap=(cls == 2).astype(np.float64))
    assert set(np.unique(cls)) <= {0.0, 1.0, 2.0}
    _check_label_conditions(c)
    LABEL_PATHS[name](c)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def label_case(name):
    """dict(name, cfg, fixed (B, 7), table = iou_table, cls = valid + overlap (outX, outY, 2), reg = regress + overlap
    (outX, outY, 14), valid, overlap): preprocess_labels(balance=False) on the case, arrays read-only."""
    return build_label_case(name, *LABEL_CASES[name]())


# ---- decode + NMS ----------------------------------------------------------------------------------------------------------------
def _head(cfg, seed, quantum=None, constant=None):
    rng = np.random.default_rng(seed)
    reg = rng.normal(0, 0.05, (cfg["outX"], cfg["outY"], 14)).astype(np.float32)
    prob = rng.uniform(0, 1, (cfg["outX"], cfg["outY"], 2)).astype(np.float32)
    if quantum is not None:
        prob = (np.floor(prob / np.float32(quantum)) * np.float32(quantum)).astype(np.float32)
    if constant is not None:
        prob[:] = np.float32(constant)
    return prob, reg


NMS_CASES = {
    # name: (configuration, head arguments, overlap threshold, maxBoxes)
    "exhausted": (REF12, dict(seed=3), 0.0, 20),
    "one": (REF12, dict(seed=3), 0.0, 0),
    "many_picks": (REF12, dict(seed=7), 5.0, 260),
    "more_than_exist": (REF12, dict(seed=7), 1e9, 600),
    "ties_576": (REF12, dict(seed=3, quantum=0.25), 1.0, 20),
    "ties_1280": (REF16, dict(seed=5, quantum=0.25), 1.0, 20),     # seed: the first pick ties with the candidate 1024 below it
    "all_equal": (REF16, dict(seed=5, constant=0.5), 1.0, 20),
}


def replay_nms(boxes, probs, thresh, max_boxes, anchor):
    """nonMaxSuppressionFast as oracle/boxes_ref.nms restates it, written out again so that every comparison it makes is seen:
    returns (picks, the smallest |IoU - thresh| over the IoUs compared that are not an exact 0 beside a threshold of 0, the
    smallest magnitude of an IoU that is not 0, whether the first pick is out of range)."""
    def out_of_range(j):
        x, y = boxes[j, 0], boxes[j, 1]
        return x - anchor[0] < 0 or x + anchor[0] > 100 or y - anchor[1] < 0 or y + anchor[1] > 100

    alive = np.ones(len(probs), dtype=bool)
    picks, gap, small = [], math.inf, math.inf
    while alive.any():
        cand = np.flatnonzero(alive)
        top = cand[probs[cand] == probs[cand].max()]
        best = int(top.max())                                  # ties: the larger flat index
        picks.append(best)
        alive[best] = False
        last = boxes[best]
        for j in np.flatnonzero(alive):
            if out_of_range(j):
                alive[j] = False
                continue
            far = math.hypot(boxes[j, 0] - last[0], boxes[j, 1] - last[1]) > 0.5 * (math.hypot(last[3], last[4]) +
                                                                                    math.hypot(boxes[j, 3], boxes[j, 4]))
            iou = 0.0 if far else B.calculate_iou(list(last), list(boxes[j]))
            if iou != 0.0:
                small = min(small, abs(iou))
            if iou != 0.0 or thresh != 0.0:
                gap = min(gap, abs(iou - thresh))
            if iou > thresh:
                alive[j] = False
        if len(picks) > max_boxes:
            break
    return picks, gap, small, out_of_range(picks[0])


PICKS = dict(exhausted=10, one=1, many_picks=261, more_than_exist=325, ties_576=21, ties_1280=21, all_equal=21)


def _check_nms_path(c):
    name, p, picks, cap = c["name"], c["probs"], c["picks"], c["max_boxes"]
    assert len(picks) == PICKS[name], f"{name}: {len(picks)} picks, listed {PICKS[name]}"
    if name == "exhausted":
        assert len(picks) < cap + 1, "the candidates are to run out before maxBoxes + 1 picks"
    if name == "one":
        assert cap == 0
    if name == "many_picks":
        assert 256 < len(picks) == cap + 1
    if name == "more_than_exist":
        assert 256 < len(picks) < cap + 1
    if name in ("exhausted", "one", "many_picks", "more_than_exist"):
        assert c["first_out_of_range"], f"{name}: the first pick is to lie out of range (the reference never checks it)"
    if name in ("ties_576", "ties_1280", "all_equal"):
        assert len(np.unique(p[picks])) == 1 and p[picks[0]] == p.max(), f"{name}: the picks are to share one probability"
        tied = np.flatnonzero(p == p.max())
        assert len(tied) > 2 * len(picks) and picks[0] == tied.max(), "the larger flat index wins"
        assert all(a > b for a, b in zip(picks, picks[1:])), "so the picks descend"
        assert tied.min() < picks[-1], "a rule that took the smaller index would pick others"
        if len(p) > 1024:                                      # the strided scan of one thread sees a tie at j and j + 1024
            assert picks[0] >= 1024 and p[picks[0] - 1024] == p[picks[0]]
    if name == "all_equal":
        assert len(np.unique(p)) == 1 and picks[0] == len(p) - 1


def build_nms_case(name, cfg, head, thresh, max_boxes):
    """The case `name` on the given head and arguments: the oracle's decode and picks, with the conditions of the header and
    the path of `name` asserted."""
    cls, reg = _head(cfg, **head)
    boxes = B.decode_boxes(reg.astype(np.float64), **oracle_grid(cfg))
    probs = cls.astype(np.float64).transpose(2, 0, 1).reshape(-1)
    anchor = (cfg["anchors"][0][0], cfg["anchors"][0][1])
    picks = B.nms(boxes, probs, overlapThresh=thresh, maxBoxes=max_boxes, anchor=anchor)
    again, gap, small, first_out = replay_nms(boxes, probs, thresh, max_boxes, anchor)
    assert again == picks, f"{name}: the replay picks differ from the oracle's"
    assert gap >= MARGIN, f"{name}: an IoU within {gap} of the overlap threshold"
    assert small >= MARGIN, f"{name}: an IoU of magnitude {small}"
    edges = np.concatenate([boxes[:, 0] - anchor[0], boxes[:, 0] + anchor[0] - 100, boxes[:, 1] - anchor[1], boxes[:, 1] + anchor[1] - 100])
    assert np.abs(edges).min() >= MARGIN, f"{name}: a candidate on a range bound"
    assert np.all(boxes[:, 3:6] > 0) and np.all(np.isfinite(boxes))       # the "illegal boxes" filter removes nothing
    c = dict(name=name, cfg=cfg, cls=cls, reg=reg, thresh=thresh, max_boxes=max_boxes, boxes=boxes, probs=probs, picks=picks,
             first_out_of_range=bool(first_out))
    _check_nms_path(c)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """dict(name, cfg, cls (outX, outY, 2) float32, reg (outX, outY, 14) float32, thresh, max_boxes, boxes (N, 7) and probs
    (N,) = the oracle's decode in anchor-major order, picks = the oracle's nms, first_out_of_range), arrays read-only."""
    return build_nms_case(name, *NMS_CASES[name])
