"""The inputs the augmentation tests share (tests/test_augment_oracle.py asserts that they are unambiguous,
tests/test_gpu_augment.py runs the kernels on them) and the oracle's answers, each computed once -- TEST ONLY."""
import functools
import math

import numpy as np

import augment_ref as R

GLOBAL = (1.03, 0.4)                    # the (scale, alpha) of the apply cases
DRAW_SEED = 20260
APPLY_CASES = ("b0", "b1", "b7", "b130", "n0", "f32", "strided", "pad")
DRAW_CASES = ("b0", "b1", "b7", "b130", "crowded")
DRAW_PARAMS = {"crowded": dict(sigma=(0.6, 0.6, 0.0))}


def _boxes(name, rng):
    if name == "b0":
        return np.zeros((0, 7))
    if name == "b1":
        return R.scene(rng, 1)
    if name == "b130":
        return R.scene(rng, 130, pitch=6.5, jitter=0.5)
    b = R.scene(rng, 7)
    b[1] = b[0]                          # two overlapping boxes: the lower index owns the shared points
    b[1, 0] += 0.9
    b[1, 6] += 0.3
    return b


@functools.lru_cache(maxsize=None)
def apply_case(name):
    """dict(points (n, 3 or 5) float64 / float32, boxes (B, 7), transforms (B, 4), scale, alpha)."""
    rng = np.random.default_rng(sorted(APPLY_CASES).index(name) + 13)
    boxes = _boxes({"n0": "b7", "f32": "b7", "strided": "b7", "pad": "b7"}.get(name, name), rng)
    n = 0 if name == "n0" else 4096 + 37
    pts = R.points_around(rng, boxes, n)
    B = len(boxes)
    t = np.stack([rng.normal(0, 1, B), rng.normal(0, 1, B), rng.normal(0, 0.1, B), rng.uniform(-0.3, 0.3, B)], 1).reshape(B, 4)
    t[2::5] = 0.0                        # some boxes stay where they are
    if name == "f32":
        pts = pts.astype(np.float32)
    if name == "strided":
        pts = np.concatenate([pts, rng.normal(0, 1, (n, 2))], 1)
    if name == "pad":
        pts[-300:] = 1.0e6
        pts[-5:, 0] = -1.0e6
    return dict(points=pts, boxes=boxes, transforms=t, scale=GLOBAL[0], alpha=GLOBAL[1])


@functools.lru_cache(maxsize=None)
def apply_expected(name):
    c = apply_case(name)
    return R.apply(c["points"][:, :3].astype(np.float64), c["boxes"], c["transforms"], c["scale"], c["alpha"])


@functools.lru_cache(maxsize=None)
def draw_case(name):
    rng = np.random.default_rng(sorted(DRAW_CASES).index(name) + 101)
    if name != "crowded":
        return _boxes(name, rng) if name != "b7" else R.scene(rng, 7)
    b = np.zeros((12, 7))                # a row of parked cars, doors almost touching: most candidates collide
    for k in range(12):
        b[k] = [-14.0 + 2.35 * k + rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2), 0.9, rng.uniform(4.2, 4.8),
                rng.uniform(1.8, 2.0), 1.6, rng.uniform(-0.03, 0.03)]
    return b


@functools.lru_cache(maxsize=None)
def draw_expected(name, item=3, epoch=1):
    """(the oracle's draw, the (area, separation) of every collision test it made)."""
    decisions = []
    d = R.draw(draw_case(name), DRAW_SEED, item, epoch, decisions=decisions, **DRAW_PARAMS.get(name, {}))
    return d, decisions


def fit_sweeps():
    """The end-to-end case: three sweeps on the (16, 32, 8) grid of tests/test_gpu_api.py (x, y in +-4 m, z in 0..2 m) with
    2-3 car-sized boxes each; float32 points."""
    rng = np.random.default_rng(77)
    pts, boxes = [], []
    for s in range(3):
        nb = 2 + s % 2
        b = np.zeros((nb, 7))
        for k in range(nb):
            b[k] = [-2.4 + 2.4 * k + rng.uniform(-0.1, 0.1), rng.uniform(-1.2, 1.2), 1.0, rng.uniform(3.4, 3.9),
                    rng.uniform(1.5, 1.7), 1.5, rng.uniform(-0.1, 0.1)]
        n = 1100 + 170 * s
        p = np.stack([rng.uniform(-4.2, 4.2, n), rng.uniform(-4.2, 4.2, n), rng.uniform(0.0, 2.1, n)], 1)
        pts.append(p.astype(np.float32))
        boxes.append(b)
    return pts, boxes
