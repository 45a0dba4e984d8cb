"""Test-local float64 oracle for the training-time augmentation (lisec_augment_draw / lisec_augment_apply) and the device
label balancing (lisec_rpn_targets) -- TEST ONLY.

Plain Python / numpy, written from the definitions of include/lisec_hip.h section 5c: Philox4x32-10 (Salmon et al., SC'11)
with key = seed and counter = (stream, item, epoch, index), uniform = (u32 + 0.5) * 2^-32, Box-Muller normals, the per-box
perturbation with its collision test (the convex clipping of tests/union_overlap_ref.py), the global scale / rotation and
the point move.  Box rows are (x, y, z, l, w, h, yaw), z the box centre.
"""
import math

import numpy as np

from oracle.boxes_ref import box_corners
from union_overlap_ref import area, clip

MAX_ATTEMPTS = 32             # LISEC_AUG_MAX_ATTEMPTS: the stride of the per-box counter index
MAX_BOXES = 512               # LISEC_AUG_MAX_BOXES
PAD_LIMIT = 0.5e6
DEFAULTS = dict(rot_box=math.pi / 10, sigma=(1.0, 1.0, 0.0), scale=(0.95, 1.05), rot_global=math.pi / 4, attempts=10)
IDENTITY = dict(rot_box=0.0, sigma=(0.0, 0.0, 0.0), scale=(1.0, 1.0), rot_global=0.0, attempts=0)
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two -> four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return [c0, c1, c2, c3]


def words(seed, stream, item, epoch, index):
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((stream, item, epoch, index), (seed & _M32, seed >> 32))


def uniform(w):
    return (w + 0.5) * 2.0 ** -32


def box_muller(w1, w2):
    r, t = math.sqrt(-2.0 * math.log(uniform(w1))), 2.0 * math.pi * uniform(w2)
    return r * math.cos(t), r * math.sin(t)


def footprint(row):
    return box_corners([float(v) for v in row])


def overlap_area(a, b):
    return area(clip(footprint(a), footprint(b)))


def _seg_dist(p, a, b):
    ax, ay, bx, by = a[0], a[1], b[0], b[1]
    dx, dy = bx - ax, by - ay
    t = max(0.0, min(1.0, ((p[0] - ax) * dx + (p[1] - ay) * dy) / (dx * dx + dy * dy)))
    return math.hypot(p[0] - ax - t * dx, p[1] - ay - t * dy)


def separation(a, b):
    """The distance between two DISJOINT footprints (vertex to edge, both ways)."""
    fa, fb = footprint(a), footprint(b)
    d = math.inf
    for p, q in ((fa, fb), (fb, fa)):
        for v in p:
            for k in range(4):
                d = min(d, _seg_dist(v, q[k], q[(k + 1) % 4]))
    return d


def draw(boxes, seed=0, item=0, epoch=0, decisions=None, **params):
    """dict(transforms (B, 4) = dx, dy, dz, dyaw; scale; alpha; boxes (B, 7) after both stages; perturbed (B, 7) after the
    per-box stage; attempt (B,), -1 = stayed; draws (4 + 8 B,) uint32).  decisions, when a list, collects (area,
    separation or None) of every candidate-against-box test the walk makes."""
    P = dict(DEFAULTS, **params)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    B = len(boxes)
    if B > MAX_BOXES:
        raise ValueError("too many boxes")
    g = words(seed, 0, item, epoch, 0)
    s = P["scale"][0] + (P["scale"][1] - P["scale"][0]) * uniform(g[0])
    alpha = P["rot_global"] * (2.0 * uniform(g[1]) - 1.0)
    cur = boxes.copy()
    transforms, attempt = np.zeros((B, 4)), -np.ones(B, dtype=np.int32)
    out_words = np.zeros(4 + 8 * B, dtype=np.uint32)
    out_words[:4] = g
    for b in range(B):
        for a in range(P["attempts"]):
            idx = (b * MAX_ATTEMPTS + a) * 2
            w0, w1 = words(seed, 1, item, epoch, idx), words(seed, 1, item, epoch, idx + 1)
            n0, n1 = box_muller(w0[1], w0[2])
            n2, _ = box_muller(w1[0], w1[1])
            t = [P["sigma"][0] * n0, P["sigma"][1] * n1, P["sigma"][2] * n2, P["rot_box"] * (2.0 * uniform(w0[0]) - 1.0)]
            cand = boxes[b].copy()
            cand[0] += t[0]; cand[1] += t[1]; cand[6] += t[3]
            free = True
            for j in range(B):
                if j == b:
                    continue
                ar = overlap_area(cand, cur[j])
                if decisions is not None:
                    decisions.append((ar, separation(cand, cur[j]) if ar == 0.0 else None))
                if ar != 0.0:
                    free = False
                    if decisions is None:
                        break
            if free:
                transforms[b], attempt[b] = t, a
                out_words[4 + 8 * b:12 + 8 * b] = w0 + w1
                cur[b] = cand
                cur[b, 2] += t[2]
                break
    perturbed = boxes.copy()
    perturbed[:, :3] += transforms[:, :3]
    perturbed[:, 6] += transforms[:, 3]
    cs, sn = math.cos(alpha), math.sin(alpha)
    out = perturbed.copy()
    out[:, 0] = s * (perturbed[:, 0] * cs - perturbed[:, 1] * sn)
    out[:, 1] = s * (perturbed[:, 0] * sn + perturbed[:, 1] * cs)
    out[:, 2] = s * perturbed[:, 2]
    out[:, 3:6] = s * perturbed[:, 3:6]
    out[:, 6] = perturbed[:, 6] - alpha
    return dict(transforms=transforms, scale=s, alpha=alpha, boxes=out, perturbed=perturbed, attempt=attempt, draws=out_words)


def box_frame(row):
    """(u, v): the footprint's axes, half extents w/2 along u and l/2 along v."""
    cs, sn = math.cos(row[6]), math.sin(row[6])
    return np.array([cs, -sn]), np.array([sn, cs])


def face_margins(points, boxes):
    """(n, B) how far every point is from changing sides of every box's closed slab test: with e_k = |coordinate_k| - half
    extent_k along u, v and z, the point is inside iff max_k e_k <= 0, so the margin is |max_k e_k| -- the distance to the
    nearest face from inside, the largest violation from outside."""
    points = np.asarray(points, dtype=np.float64)[:, :3]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    out = np.full((len(points), len(boxes)), np.inf)
    for j, r in enumerate(boxes):
        u, v = box_frame(r)
        d = points[:, :2] - r[:2]
        e = np.stack([np.abs(d @ u) - r[4] / 2, np.abs(d @ v) - r[3] / 2, np.abs(points[:, 2] - r[2]) - r[5] / 2])
        out[:, j] = np.abs(e.max(0))
    return out


def owner(points, boxes):
    """(n,) the lowest box index holding each point, -1 for none."""
    points = np.asarray(points, dtype=np.float64)[:, :3]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    own = -np.ones(len(points), dtype=np.int64)
    for j in range(len(boxes) - 1, -1, -1):
        r = boxes[j]
        u, v = box_frame(r)
        d = points[:, :2] - r[:2]
        inside = ((np.abs(d @ u) <= r[4] / 2) & (np.abs(d @ v) <= r[3] / 2) & (points[:, 2] >= r[2] - r[5] / 2)
                  & (points[:, 2] <= r[2] + r[5] / 2))
        own[inside] = j
    return own


def apply(points, boxes, transforms, scale, alpha):
    """(n, 3) float64: the points after the per-box move and the global transform; rows with |x| >= PAD_LIMIT untouched."""
    pts = np.asarray(points, dtype=np.float64)[:, :3].copy()
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    transforms = np.asarray(transforms, dtype=np.float64).reshape(-1, 4)
    pad = ~(np.abs(pts[:, 0]) < PAD_LIMIT)
    own = owner(pts, boxes)
    own[pad] = -1
    for j in range(len(boxes)):
        sel = own == j
        if not sel.any() or not transforms[j].any():
            continue                                            # a box that stays leaves its points bit for bit
        r, t = boxes[j], transforms[j]
        u, v = box_frame(r)
        moved = r.copy()
        moved[6] += t[3]
        nu, nv = box_frame(moved)
        d = pts[sel, :2] - r[:2]
        du, dv = d @ u, d @ v
        pts[sel, :2] = (r[:2] + t[:2]) + du[:, None] * nu + dv[:, None] * nv
        pts[sel, 2] += t[2]
    cs, sn = math.cos(alpha), math.sin(alpha)
    out = pts.copy()
    live = ~pad
    out[live, 0] = scale * (pts[live, 0] * cs - pts[live, 1] * sn)
    out[live, 1] = scale * (pts[live, 0] * sn + pts[live, 1] * cs)
    out[live, 2] = scale * pts[live, 2]
    return out


def augment(points, boxes, seed=0, item=0, epoch=0, **params):
    d = draw(boxes, seed, item, epoch, **params)
    return apply(points, boxes, d["transforms"], d["scale"], d["alpha"]), d["boxes"]


def balance_keep(valid, overlap, max_regions, seed=0, item=0, epoch=0):
    """`valid` after the balancing of serialize_data.py:310-325 with Philox keys: per class (positive = valid & overlap,
    negative = valid & ~overlap) the `keep` smallest keys (Philox(2, item, epoch, flat)[0] << 32 | flat) survive."""
    valid = np.array(valid, dtype=np.float64)
    flat_v, flat_o = valid.reshape(-1), np.asarray(overlap, dtype=np.float64).reshape(-1)
    pos = np.nonzero((flat_v == 1) & (flat_o == 1))[0]
    neg = np.nonzero((flat_v == 1) & (flat_o == 0))[0]
    keep_pos = min(len(pos), max_regions // 2)
    keep_neg = keep_pos if len(neg) + keep_pos > max_regions else len(neg)
    for members, keep in ((pos, keep_pos), (neg, keep_neg)):
        keys = sorted((words(seed, 2, item, epoch, int(i))[0] << 32) | int(i) for i in members)
        for k in keys[keep:]:
            flat_v[k & _M32] = 0.0
    return valid


def scene(rng, n_boxes, extent=40.0, pitch=9.0, jitter=1.0):
    """n_boxes car-sized boxes on a jittered lattice of `pitch` metres inside +-extent (no two overlap for pitch >= 8)."""
    side = int(2 * extent // pitch)
    if n_boxes > side * side:
        raise ValueError("the lattice is too small")
    cells = rng.permutation(side * side)[:n_boxes]
    b = np.zeros((n_boxes, 7))
    for k, c in enumerate(cells):
        b[k] = [-extent + pitch * (c % side + 0.5) + rng.uniform(-jitter, jitter),
                -extent + pitch * (c // side + 0.5) + rng.uniform(-jitter, jitter), rng.uniform(0.6, 1.2),
                rng.uniform(3.6, 5.0), rng.uniform(1.6, 2.1), rng.uniform(1.4, 1.8), rng.uniform(-math.pi, math.pi)]
    return b


def points_around(rng, boxes, n, extent=45.0, inside=0.5):
    """n points: a share `inside` of them scattered over the boxes' frames (in and just around them), the rest uniform."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    pts = np.stack([rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n), rng.uniform(-0.5, 2.5, n)], 1)
    if len(boxes):
        k = int(n * inside)
        which = rng.integers(0, len(boxes), k)
        for i, j in enumerate(which):
            r = boxes[j]
            u, v = box_frame(r)
            a, c = rng.uniform(-0.6, 0.6) * r[4], rng.uniform(-0.6, 0.6) * r[3]
            pts[i, :2] = r[:2] + a * u + c * v
            pts[i, 2] = r[2] + rng.uniform(-0.6, 0.6) * r[5]
    return pts
