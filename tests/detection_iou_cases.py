"""The inputs of tests/test_gpu_detection_iou_loss.py, built without a GPU so that tests/test_detection_iou_loss_oracle.py
can check on the reference alone the condition the GPU tolerance rests on -- TEST ONLY.

A case is (pattern, M, combo): the label pattern and the number of cells of tests/test_gpu_detection_loss.py, and a combo
(iou_mode, residual deviation, iou_weight, gamma).  Targets t ~ N(0, 0.3) carry the reference's +1; the residuals r - t are
normal with the combo's deviation: 0.15 (nearly every positive overlaps its target), 0.5 and 1.5 (most do not).  The IoU is
piecewise smooth: where a corner of one footprint crosses an edge of the other, or two tops or bottoms are level, it has a
kink and central differences of two steps disagree.  A random anchor lies within a few 1e-6 of one with a probability of
about 1e-4, so the seed of a case is the first of base, base + 1, ... for which NO positive does (SEED_SHIFT, found with
seed_shift() on the reference alone); the oracle test asserts the condition for every positive of every case."""
import functools

import numpy as np

import detection_iou_loss_ref as R

# one workgroup of the anchor pass holds 128 cells (256 threads, two anchors a cell); 1024 workgroups hold 131072 cells
SIZES = [1, 3, 17, 255, 257, 16385]
PATTERNS = ["positives", "mix"]
STRIDE_M = 131072 + 37
WEIGHTS = (2.0, 0.5)
GRAD_SCALE = 0.75
# (iou_mode, deviation of r - t, iou_weight, gamma)
COMBOS = [("bev", 0.15, 1.0, 0.0), ("bev", 0.5, 2.0, 2.0), ("bev", 1.5, 1.0, 2.0),
          ("3d", 0.15, 2.0, 0.0), ("3d", 0.5, 1.0, 2.0), ("3d", 1.5, 2.0, 0.0)]
FD_AGREE = 1e-6                                  # fd(1e-6) against fd(3e-6), of the anchor's largest component

# (pattern, M, combo index) -> how far the seed moved on from its base; absent: 0
SEED_SHIFT = {("positives", 257, 0): 1}


def combos(pattern, M):
    """Indices into COMBOS.  Every positive costs 14 clipped areas in the reference: the all-positive map of 16385 cells
    (32770 positives) takes one combo, every other case all six."""
    return [4] if (pattern, M) == ("positives", 16385) else list(range(len(COMBOS)))


def params(combo):
    mode, _, iou_weight, gamma = COMBOS[combo]
    det = dict(alpha=1.5 if gamma == 0 else 0.5, beta=1.0 if gamma == 0 else 1.5, gamma=gamma, smooth_l1_beta=1.0)
    return det, dict(iou_weight=iou_weight, iou_mode=mode)


def _labels(pattern, M, rng):
    if pattern == "positives":
        return np.full((M, 2), 2.0, np.float32)
    if pattern == "stride":
        y = np.ones((M, 2), np.float32)
        border = [0, 131071, 131072, 131073, M - 1]
        cells = np.concatenate([border, rng.choice(np.setdiff1d(np.arange(M), border), 59, replace=False)])
        y[cells, rng.integers(0, 2, len(cells))] = 2.0
        return y
    y = rng.choice(np.float32([0, 1, 2]), (M, 2), p=[0.49, 0.5, 0.01])           # about 1 % positives
    y[M // 2, 1] = 2.0                                                          # at least one
    return y


def build(pattern, M, combo, seed):
    """head, y_cls, y_reg (float32)."""
    rng = np.random.default_rng(seed)
    y_cls = _labels(pattern, M, rng)
    t = rng.normal(0, 0.3, (M, 14))
    d = rng.normal(0, COMBOS[combo][1], (M, 14))
    head = np.empty((M, 16), np.float32)
    head[:, :2] = rng.normal(0, 1.5, (M, 2))
    head[:, 2:] = t + d
    y_reg = (t + 1.0).astype(np.float32)
    return head, y_cls, y_reg


def _base_seed(pattern, M, combo):
    return 1000 * combo + 7 * M + len(pattern)


def fd_disagreement(head, y_cls, y_reg, mode):
    """Per positive: |fd(1e-6) - fd(3e-6)| of the IoU term's gradient over the anchor's largest |fd(1e-6)| component (0
    where the gradient is zero in both), and fd(1e-6) itself."""
    _, _, r, t, an = R.positives(head, y_cls, y_reg)
    g1, g3 = R.iou_term_grad(r, t, an, mode, 1e-6), R.iou_term_grad(r, t, an, mode, 3e-6)
    top = np.abs(g1).max(axis=1)
    dev = np.abs(g3 - g1).max(axis=1)
    return np.where(dev > 0, dev / np.where(top > 0, top, 1.0), 0.0), g1


def seed_shift(pattern, M, combo, tries=50):
    """The first shift for which every positive meets FD_AGREE: how SEED_SHIFT was filled."""
    for k in range(tries):
        head, y_cls, y_reg = build(pattern, M, combo, _base_seed(pattern, M, combo) + k)
        if fd_disagreement(head, y_cls, y_reg, COMBOS[combo][0])[0].max(initial=0.0) <= FD_AGREE:
            return k
    raise RuntimeError("no seed found")


@functools.lru_cache(maxsize=4)
def case(pattern, M, combo):
    return build(pattern, M, combo, _base_seed(pattern, M, combo) + SEED_SHIFT.get((pattern, M, combo), 0))


def all_cases():
    out = [(p, M, c) for p in PATTERNS for M in SIZES for c in combos(p, M)]
    return out + [("stride", STRIDE_M, c) for c in (1, 3)]
