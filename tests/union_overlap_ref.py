"""Test-local float64 oracle for the union / overlap areas of calcIntersectAll (rpnToRegion.py:202-213) -- TEST ONLY.

The reference unions each side with shapely's cascaded_union and intersects the two unions; shapely is absent here.  This
restates the same quantity without any polygon union: with the convex pieces C_ij = P_i n L_j,

    area((U P) n (U L)) = area(U C_ij) = sum over non-empty subsets S of the pieces of (-1)^(|S|+1) area(n S)

which is exact because an intersection of convex sets is convex (Sutherland-Hodgman clipping returns it).  The subsets are
walked depth-first and a branch ends as soon as its intersection is empty, and the pieces are first split into connected
clusters (overlap graph), each limited to MAX_PIECES pieces.  area(U P) and area(U L) are the same sum over the boxes.
"""
import numpy as np

from oracle.boxes_ref import box_corners

MAX_PIECES = 12


def _signed_area(poly):
    a = 0.0
    for i in range(len(poly)):
        x0, y0 = poly[i]
        x1, y1 = poly[(i + 1) % len(poly)]
        a += x0 * y1 - x1 * y0
    return 0.5 * a


def _ccw(poly):
    return list(poly) if _signed_area(poly) >= 0 else list(poly)[::-1]


def clip(p, q):
    """Sutherland-Hodgman: the convex polygon p n q as a vertex list ([] when empty).  Any orientation."""
    out = _ccw(p)
    q = _ccw(q)
    for i in range(len(q)):
        ax, ay = q[i]
        bx, by = q[(i + 1) % len(q)]
        ex, ey = bx - ax, by - ay
        inp, out = out, []
        if not inp:
            break
        for j in range(len(inp)):
            cx, cy = inp[j]
            dx, dy = inp[(j + 1) % len(inp)]
            sc = ex * (cy - ay) - ey * (cx - ax)
            sd = ex * (dy - ay) - ey * (dx - ax)
            if sc >= 0:
                out.append((cx, cy))
            if (sc >= 0) != (sd >= 0):
                t = sc / (sc - sd)
                out.append((cx + t * (dx - cx), cy + t * (dy - cy)))
    return out if len(out) >= 3 else []


def area(poly):
    return abs(_signed_area(poly)) if len(poly) >= 3 else 0.0


def footprint(box):
    """boxToShapely's quadrilateral (serialize_data.py:151-163); [] for a box with l == 0 or w == 0."""
    if box[3] == 0 or box[4] == 0:
        return []
    return box_corners(list(box))


def union_area(polys):
    """Area of the union of convex polygons by inclusion-exclusion, cluster by cluster."""
    polys = [p for p in polys if area(p) > 0.0]
    n = len(polys)
    touch = [[j for j in range(n) if j != i and area(clip(polys[i], polys[j])) > 0.0] for i in range(n)]
    seen, total = [False] * n, 0.0
    for s in range(n):
        if seen[s]:
            continue
        cluster, stack = [], [s]
        seen[s] = True
        while stack:
            i = stack.pop()
            cluster.append(i)
            for j in touch[i]:
                if not seen[j]:
                    seen[j] = True
                    stack.append(j)
        if len(cluster) > MAX_PIECES:
            raise ValueError(f"a cluster of {len(cluster)} pieces is beyond the oracle's limit of {MAX_PIECES}")
        cluster.sort()
        total += _incl_excl([polys[i] for i in cluster])
    return total


def _incl_excl(polys):
    total = 0.0

    def walk(start, inter, sign):
        nonlocal total
        for i in range(start, len(polys)):
            cur = polys[i] if inter is None else clip(inter, polys[i])
            a = area(cur)
            if a <= 0.0:
                continue
            total += sign * a
            walk(i + 1, cur, -sign)

    walk(0, None, 1.0)
    return total


def union_overlap(pred, label):
    """The five numbers lisec_boxes_union_overlap reports for one sample: area((U P) n (U L)), area(U P), area(U L),
    sum of l*w*h over P, over L."""
    pred = np.asarray(pred, dtype=np.float64).reshape(-1, 7)
    label = np.asarray(label, dtype=np.float64).reshape(-1, 7)
    P = [footprint(b) for b in pred]
    L = [footprint(b) for b in label]
    pieces = [clip(p, q) for p in P if p for q in L if q]
    vol = lambda bs: float(sum(b[3] * b[4] * b[5] for b in bs))          # noqa: E731
    return np.array([union_area(pieces), union_area([p for p in P if p]), union_area([q for q in L if q]),
                     vol(pred), vol(label)])


def clustered_scene(rng, n_pred, n_label, n_clusters, spread=2.5, pitch=14.0):
    """n_pred + n_label car-sized boxes in n_clusters groups `pitch` metres apart (so that no two groups touch and the
    inclusion-exclusion stays small), dealt round-robin to the groups."""
    cols = int(np.ceil(np.sqrt(n_clusters)))
    centres = [((c % cols - (cols - 1) / 2) * pitch, (c // cols - (cols - 1) / 2) * pitch) for c in range(n_clusters)]

    def side(n):
        b = np.zeros((n, 7))
        for i in range(n):
            cx, cy = centres[i % n_clusters]
            b[i] = [cx + rng.uniform(-spread, spread), cy + rng.uniform(-spread, spread), rng.uniform(0.5, 1.5),
                    rng.uniform(3.5, 5.2), rng.uniform(1.6, 2.2), rng.uniform(1.3, 1.8), rng.uniform(-np.pi, np.pi)]
        return b
    return side(n_pred), side(n_label)
