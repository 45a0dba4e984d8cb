"""Head maps for the detection-output tests (tests/test_detect_oracle.py on the CPU, tests/test_gpu_detect.py on the GPU) -- TEST
ONLY.  A builder turns wanted boxes and scores into cls (100, 200, 2) / reg (100, 200, 14) float32 maps by inverting the
decode of detect_ref; every other candidate keeps the anchor box and a very low score.  case(name) builds a case once per
process and runs the oracle on it once; both test files read that one result.
"""
import functools
import math

import numpy as np

import detect_ref as D

G = D.GRID
M = G["outX"] * G["outY"]
FILL = -30.0                                                   # the score of every candidate a case does not place


class Maps:
    def __init__(self, fill=FILL):
        self.cls = np.full((G["outX"], G["outY"], 2), fill, dtype=np.float32)
        self.reg = np.zeros((G["outX"], G["outY"], 14), dtype=np.float32)
        self.used = set()

    def _free_cell(self, x, y):
        ix0 = min(max(int(math.floor(x / G["vx"])), 0), G["outX"] - 1)
        iy0 = min(max(int(math.floor(y / G["vy"])), 0), G["outY"] - 1)
        for r in range(0, 40):
            for dx in range(-r, r + 1):
                for dy in range(-r, r + 1):
                    if max(abs(dx), abs(dy)) != r:
                        continue
                    ix, iy = ix0 + dx, iy0 + dy
                    if 0 <= ix < G["outX"] and 0 <= iy < G["outY"]:
                        for a in (0, 1):
                            if (a, ix, iy) not in self.used:
                                return a, ix, iy
        raise RuntimeError("no free cell near the box")

    def put(self, box, score, at=None):
        """The candidate at = (anchor, ix, iy) (default: the free one nearest to the centre) decodes to `box` (up to the
        float32 rounding of the seven regression values) and scores `score`.  Returns its flat index."""
        a, ix, iy = at if at is not None else self._free_cell(box[0], box[1])
        assert (a, ix, iy) not in self.used
        self.used.add((a, ix, iy))
        an = G["anchors"][a]
        xc, yc = ix * G["vx"] + G["vx"] / 2, iy * G["vy"] + G["vy"] / 2
        t = [(box[0] - xc) / an[0], (box[1] - yc) / an[1], (box[2] - 1.0) / an[2], math.log(box[3] / an[0]),
             math.log(box[4] / an[1]), math.log(box[5] / an[2]), box[6] - an[3]]
        self.reg[ix, iy, 7 * a:7 * a + 7] = np.asarray(t, dtype=np.float32)
        self.cls[ix, iy, a] = np.float32(score)
        return a * M + ix * G["outY"] + iy

    def raw(self, at, score, regress=None):
        """Sets a candidate's score and, when given, its seven regression values as they are."""
        a, ix, iy = at
        assert at not in self.used
        self.used.add(at)
        self.cls[ix, iy, a] = np.float32(score)
        if regress is not None:
            self.reg[ix, iy, 7 * a:7 * a + 7] = np.asarray(regress, dtype=np.float32)
        return a * M + ix * G["outY"] + iy


def car(x, y, yaw=0.0, l=4.0, w=2.0, z=1.0, h=1.5):
    """x, y, z, l, w, h, yaw; at yaw 0 the WIDTH lies along x and the length along y."""
    return [x, y, z, l, w, h, yaw]


def descending(n, hi=6.0, lo=-6.0):
    """n distinct float32 scores, largest first."""
    s = np.linspace(hi, lo, n).astype(np.float32)
    assert len(np.unique(s)) == n
    return s


def scattered(maps, rng, count, scores):
    """count candidates on random distinct cells away from the border, each the anchor box disturbed a little."""
    flat = rng.choice(2 * 92 * 186, size=count, replace=False)
    for f, s in zip(flat, scores):
        a, rest = divmod(int(f), 92 * 186)
        ix, iy = rest // 186 + 4, rest % 186 + 7
        t = rng.normal(0, 0.1, 7)
        maps.raw((a, ix, iy), s, t)


def clustered(maps, rng, count, n_clusters, scores, spread=2.5):
    """count car-sized boxes in n_clusters groups spread over the whole grid."""
    cols = int(math.ceil(math.sqrt(n_clusters)))
    pitch = 90.0 / cols
    for i, s in enumerate(scores[:count]):
        c = i % n_clusters
        cx, cy = 5.0 + pitch * (c % cols + 0.5), 5.0 + pitch * (c // cols + 0.5)
        maps.put([cx + rng.uniform(-spread, spread), cy + rng.uniform(-spread, spread), rng.uniform(0.5, 1.5),
                  rng.uniform(3.5, 5.2), rng.uniform(1.6, 2.2), rng.uniform(1.3, 1.8), rng.uniform(-math.pi, math.pi)], s)


# ---- the cases: name -> (maps, keyword arguments of boxes.detect, ties meant) -------------------------------------------------
def _scatter_case(seed, count, top_n, max_boxes, **kw):
    def build():
        rng = np.random.default_rng(seed)
        maps = Maps()
        scattered(maps, rng, count, rng.permutation(descending(count)))
        return maps, dict(dict(score_threshold=-10.0, pre_nms_top_n=top_n, max_boxes=max_boxes), **kw), False
    return build


def _all_equal(top_n):
    def build():
        rng = np.random.default_rng(40)
        maps = Maps()
        scattered(maps, rng, 50, np.full(50, 0.5, dtype=np.float32))
        return maps, dict(score_threshold=-10.0, pre_nms_top_n=top_n, max_boxes=top_n), True
    return build


def _straddle():
    """15 distinct scores above, ten equal ones around the 20th place, 20 distinct below: five of the ten make the cut."""
    rng = np.random.default_rng(41)
    maps = Maps()
    scores = np.concatenate([descending(15, 6.0, 2.0), np.full(10, 1.0, dtype=np.float32), descending(20, 0.5, -3.0)])
    scattered(maps, rng, 45, rng.permutation(scores))
    return maps, dict(score_threshold=-10.0, pre_nms_top_n=20, max_boxes=20), True


def _fill_ties():
    """No threshold: all 40 000 candidates pass, 39 800 of them with the one score of the fill.  The 100 places left after
    the 200 placed ones go to the fill's largest flat indices, anchor boxes half a metre apart that suppress their neighbours;
    the cut sits in a bin of 39 800 equal scores, which only the index digits of the key take apart."""
    rng = np.random.default_rng(44)
    maps = Maps()
    scattered(maps, rng, 200, rng.permutation(descending(200)))
    return maps, dict(score_threshold=None, pre_nms_top_n=300, max_boxes=300), True


CHAIN_RANKS = dict(A=(8, 3, 5, 10, 65, 127), B=(20, 70, 4095, 64, 100, 128), C=(21, 72, None, 66, 101, 130))


def _chains():
    """4096 candidates, all of them ranked: six chains A, B, C of cars 1.2 m apart along x (IoU(A, B) = IoU(B, C) = 0.25, A and
    C 0.4 m apart) at the ranks of CHAIN_RANKS, every other rank a 0.5 m box of its own on a 1 m lattice.  A suppresses B, so C
    stays: the kept ranks are all but the six B.  Suppressor and victim share a mask word (8, 20), sit in different words
    (3, 70), in the first and the last (5, 4095), the victim is bit 0 of a word (10, 64), both lie in one tile on the diagonal
    whose first row is the suppressor's neighbour (65, 100), and they are neighbours across a tile edge (127, 128)."""
    maps = Maps()
    scores = descending(4096)
    placed = {}
    for c in range(6):
        x0 = 10.0 + 15.0 * c
        for name, dx in (("A", 0.0), ("B", 1.2), ("C", 2.4)):
            r = CHAIN_RANKS[name][c]
            if r is not None:
                placed[r] = car(x0 + dx, 8.0)
    lattice = ((2.5 + i, 20.5 + j) for j in range(70) for i in range(96))
    for r in range(4096):
        if r in placed:
            maps.put(placed[r], scores[r])
        else:
            x, y = next(lattice)
            maps.put(car(x, y, l=0.5, w=0.5), scores[r])
    return maps, dict(score_threshold=-10.0, pre_nms_top_n=4096, max_boxes=4096), False


def _filters(**kw):
    def build():
        rng = np.random.default_rng(42)
        maps = Maps()
        scattered(maps, rng, 30, rng.permutation(descending(30, 3.0, -1.0)))
        zero = [0.0] * 7
        maps.raw((0, 1, 3), math.nan, zero)                    # scores that are no numbers or no finite ones
        maps.raw((0, 1, 30), math.inf, zero)
        maps.raw((0, 1, 60), -math.inf, zero)
        maps.raw((1, 2, 90), 4.0, [0, 0, 0, 800.0, 0, 0, 0])   # exp overflows: the length is not finite
        maps.raw((1, 2, 120), 4.1, [0, 0, 0, 0, -800.0, 0, 0])  # exp underflows: the width is 0
        maps.raw((0, 0, 150), 4.2, [-1.0, 0, 0, 0, 0, 0, 0])   # x = 0.5 - 1.6: a good box centred outside the grid
        maps.raw((1, 3, 180), 4.3, [0, 0, 0, 0, 0, 0, math.nan])
        return maps, dict(dict(pre_nms_top_n=64, max_boxes=64), **kw), False
    return build


def _z_pairs(mode):
    """Two cars on one footprint 3 m apart in z, and two that overlap in both senses."""
    def build():
        maps = Maps()
        s = descending(4, 3.0, 0.0)
        maps.put(car(30.0, 30.0, 0.3, z=1.0), s[0])
        maps.put(car(30.2, 30.1, 0.3, z=4.0), s[1])
        maps.put(car(60.0, 60.0, -0.4, z=1.0), s[2])
        maps.put(car(60.3, 60.2, -0.4, z=1.2), s[3])
        return maps, dict(score_threshold=-10.0, pre_nms_top_n=64, max_boxes=64, iou_mode=mode), False
    return build


def _clustered_scene():
    rng = np.random.default_rng(43)
    maps = Maps()
    clustered(maps, rng, 700, 49, rng.permutation(descending(700)))
    return maps, dict(score_threshold=-10.0, pre_nms_top_n=1000, max_boxes=300), False


CASES = {
    "top1": _scatter_case(30, 200, 1, 1),
    "top63": _scatter_case(31, 200, 63, 63),
    "top64": _scatter_case(32, 200, 64, 64),
    "top65": _scatter_case(33, 200, 65, 65),
    "top64_exactly": _scatter_case(34, 64, 64, 64),
    "top1000_fewer": _scatter_case(35, 700, 1000, 300),
    "top1000_exactly": _scatter_case(36, 1000, 1000, 300),
    "top4096_of_4500": _scatter_case(37, 4500, 4096, 1000),
    "nothing_passes": _scatter_case(38, 200, 64, 64, score_threshold=7.0),
    "all_equal_fewer": _all_equal(64),
    "all_equal_cut": _all_equal(30),
    "tie_straddles_the_cut": _straddle,
    "fill_ties_without_a_threshold": _fill_ties,
    "chains": _chains,
    "cap": _scatter_case(39, 600, 1000, 50),
    "filters_raw": _filters(score_threshold=0.5),
    "filters_raw_outside_too": _filters(score_threshold=0.5, inside_only=False),
    "filters_logits": _filters(score_threshold=0.6, from_logits=True),
    "z_pairs_bev": _z_pairs("bev"),
    "z_pairs_3d": _z_pairs("3d"),
    "clustered_scene": _clustered_scene,
}


def oracle_arguments(kw):
    """The keyword arguments of boxes.detect as detect_ref.detect takes them: the raw threshold and the sigmoid flag."""
    t = kw.get("score_threshold")
    logits = kw.get("from_logits", False)
    raw = -math.inf if t is None else (math.log(t / (1.0 - t)) if logits else float(t))
    return dict(score_threshold=raw, sigmoid_scores=logits, pre_nms_top_n=kw.get("pre_nms_top_n", 1000),
                max_boxes=kw.get("max_boxes", 100), iou_threshold=kw.get("iou_threshold", 0.1), iou_mode=kw.get("iou_mode", "bev"),
                inside_only=kw.get("inside_only", True))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(cls, reg, kw = boxes.detect's keyword arguments, ref = detect_ref.detect's result, ties)."""
    maps, kw, ties = CASES[name]()
    maps.cls.setflags(write=False)
    maps.reg.setflags(write=False)
    return dict(cls=maps.cls, reg=maps.reg, kw=kw, ref=D.detect(maps.cls, maps.reg, **oracle_arguments(kw)), ties=ties)
