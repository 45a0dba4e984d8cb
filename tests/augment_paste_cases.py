"""The inputs the ground-truth sampling tests share (tests/test_augment_paste_oracle.py asserts that they are unambiguous,
tests/test_gpu_augment_paste.py runs the kernels on them) and the oracle's answers, each computed once -- TEST ONLY."""
import functools

import numpy as np

import augment_paste_ref as P
import augment_ref as R

SEED = 4711
MIN_POINTS = 5
OWNER_CASES = ("n0", "n1", "b0", "b1", "b7", "b130", "f32", "strided", "pad")
DATABASE_CASES = ("f32", "mixed")
SAMPLE_CASES = ("k0", "m0", "m1", "b0", "chain", "crowded", "k64")
PASTE_CASES = ("f32", "f64", "strided", "n0", "pad", "big", "cap")


# ---- owner ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def owner_case(name):
    """(points (n, 3 or 5), boxes (B, 7))."""
    rng = np.random.default_rng(sorted(OWNER_CASES).index(name) + 301)
    nb = {"b0": 0, "b1": 1, "b130": 130}.get(name, 7)
    boxes = R.scene(rng, nb, pitch=6.5, jitter=0.5) if nb == 130 else R.scene(rng, nb)
    if nb == 7:
        boxes[1] = boxes[0]              # two overlapping boxes: the lower index owns the shared points
        boxes[1, 0] += 0.9
        boxes[1, 6] += 0.3
    pts = R.points_around(rng, boxes, {"n0": 0, "n1": 1}.get(name, 1000))
    if name == "f32":
        pts = pts.astype(np.float32)
    if name == "strided":
        pts = np.concatenate([pts, rng.normal(0, 1, (len(pts), 2))], 1)
    if name == "pad":
        pts[-100:] = 1.0e6
        pts[-3:, 0] = -1.0e6
    return pts, boxes


# ---- database -------------------------------------------------------------------------------------------------------------
def _interior(rng, row, k):
    """k points well inside the box `row`."""
    u, v = R.box_frame(row)
    a, c = rng.uniform(-0.4, 0.4, k) * row[4], rng.uniform(-0.4, 0.4, k) * row[3]
    xy = row[:2] + a[:, None] * u + c[:, None] * v
    return np.concatenate([xy, (row[2] + rng.uniform(-0.4, 0.4, k) * row[5])[:, None]], 1)


@functools.lru_cache(maxsize=None)
def database_sweeps(name="f32"):
    """(points_list, boxes_list): 3 sweeps of 600 to 2000 points with 4 to 9 boxes.  In sweep 0, box 0 owns no point, box 1
    exactly MIN_POINTS, box 2 MIN_POINTS - 1 and box 3 more than 256.  "mixed": sweep 2 is float64, the others float32."""
    rng = np.random.default_rng(911)
    pts, boxes = [], []
    for s, (n, nb) in enumerate(((1500, 9), (600, 4), (2000, 6))):
        b = R.scene(rng, nb)
        p = R.points_around(rng, b, n, inside=0.3)
        if s == 0:
            own = R.owner(p, b)
            p = p[~np.isin(own, (0, 1, 2, 3))]
            p = np.concatenate([p, _interior(rng, b[1], MIN_POINTS), _interior(rng, b[2], MIN_POINTS - 1),
                                _interior(rng, b[3], 300)])
            p = p[rng.permutation(len(p))]
        pts.append(p.astype(np.float64 if (name == "mixed" and s == 2) else np.float32))
        boxes.append(b)
    return pts, boxes


@functools.lru_cache(maxsize=None)
def database(name="f32"):
    return P.build_database(*database_sweeps(name), min_points=MIN_POINTS)


def as_dtype(db, dtype):
    return dict(db, points=db["points"].astype(dtype))


# ---- sample ---------------------------------------------------------------------------------------------------------------
def _chain():
    """Scene box S; object 0 overlaps S, object 1 overlaps object 0 only, object 2 overlaps object 1 only."""
    row = lambda x: [x, 0.0, 1.0, 4.0, 2.0, 1.6, 0.0]            # footprints 2 m wide along x, 4 m long along y
    scene = np.array([row(0.0)])
    db = dict(boxes=np.array([row(1.5), row(3.0), row(4.5)]), counts=np.array([6, 7, 8], dtype=np.int32),
              offsets=np.array([0, 6, 13, 21], dtype=np.int32))
    rng = np.random.default_rng(5)
    db["points"] = np.concatenate([_interior(rng, r, c) for r, c in zip(db["boxes"], db["counts"])]).astype(np.float32)
    return scene, db


@functools.lru_cache(maxsize=None)
def chain_seed():
    """The first seed whose three draws at (item 3, epoch 1) hit the objects 0, 1, 2 in that order."""
    for seed in range(10000):
        if [P.database_index(R.words(seed, 3, 3, 1, k)[0], 3) for k in range(3)] == [0, 1, 2]:
            return seed
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def sample_case(name):
    """(scene boxes (B, 7), database, sample_to, seed)."""
    rng = np.random.default_rng(sorted(SAMPLE_CASES).index(name) + 501)
    db = database("f32")
    if name == "chain":
        scene, db = _chain()
        return scene, db, 4, chain_seed()
    if name == "k0":
        return R.scene(rng, 7), db, 5, SEED
    if name == "m0":
        return R.scene(rng, 4), P.build_database([], []), 7, SEED
    if name == "m1":
        one = dict(boxes=db["boxes"][:1], counts=db["counts"][:1], offsets=db["offsets"][:2],
                   points=db["points"][:db["offsets"][1]])
        scene = R.scene(rng, 3)
        scene[:, 0] += 200.0                  # far from the one object: the first draw of it is accepted
        return scene, one, 6, SEED
    if name == "b0":
        return np.zeros((0, 7)), db, 6, SEED
    if name == "crowded":
        return R.scene(rng, 7), db, 7 + 24, SEED
    return R.scene(rng, 3), db, 100, SEED     # k64


@functools.lru_cache(maxsize=None)
def sample_expected(name, item=3, epoch=1):
    """(the oracle's sample, the (area, separation) of every collision test behind it)."""
    scene, db, sample_to, seed = sample_case(name)
    decisions = []
    return P.sample(scene, db, P.sample_count(len(scene), sample_to), seed, item, epoch, decisions=decisions), decisions


# ---- paste ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def paste_case(name):
    """dict(points (n, 3 or 5), boxes (B, 7), db (points in the case's dtype), sample, cap, want (cap, 3), removed (n,))."""
    rng = np.random.default_rng(sorted(PASTE_CASES).index(name) + 701)
    dtype = np.float64 if name == "f64" else np.float32
    db = as_dtype(database("f32"), dtype)
    scene = R.scene(rng, 3)
    seed = SEED
    if name == "big":                    # the first seed at which the object of more than 256 points is accepted
        big = int(np.argmax(db["counts"]))
        seed = next(s for s in range(SEED, SEED + 1000) if big in P.sample(scene, db, 12, s, 3, 1)["index"])
    smp = P.sample(scene, db, 12, seed, 3, 1)
    n = 0 if name == "n0" else 1500
    pts = R.points_around(rng, np.concatenate([scene, db["boxes"]]), n, inside=0.6).astype(dtype)
    if name == "strided":
        pts = np.concatenate([pts, rng.normal(0, 1, (n, 2)).astype(dtype)], 1)
    if name == "pad":
        pts[-200:] = 1.0e6
        pts[-3:, 0] = -1.0e6
    cap = n + P.bound(db, 12) + (777 if name == "cap" else 0)
    want, removed = P.paste(pts, db, smp, len(scene), cap)
    return dict(points=pts, boxes=scene, db=db, sample=smp, cap=cap, want=want, removed=removed)


# ---- the whole item -------------------------------------------------------------------------------------------------------
ITEM_SAMPLE_TO = 14
ITEM_AT = (1, 3)                         # the (item, epoch) whose label maps do not rest on rounding either (label_margins)


@functools.lru_cache(maxsize=None)
def item_case():
    """(points (n, 3) float32, boxes (B, 7), database) of the full-item test; the database is database("f32")."""
    rng = np.random.default_rng(1234)
    db = database("f32")
    scene = R.scene(rng, 4)
    pts = R.points_around(rng, np.concatenate([scene, db["boxes"]]), 1200, inside=0.6).astype(np.float32)
    return pts, scene, db


@functools.lru_cache(maxsize=None)
def item_expected(item=ITEM_AT[0], epoch=ITEM_AT[1]):
    pts, scene, db = item_case()
    return P.item(pts, scene, db, ITEM_SAMPLE_TO, SEED, item, epoch)


FIT_SAMPLE_TO = 6
FIT_SEED = 4                             # objects are accepted in both epochs (tests/test_augment_paste_oracle.py)
