"""The fp64 definition of the VoxelNet detection loss with the rotated-box IoU term (include/lisec_hip.h,
lisec_detection_iou_loss) -- TEST ONLY, numpy, nothing of the kernels and not their method:

    L_reg = 1/N_pos sum_pos [ sum_k S(r_k - t_k) + iou_weight (1 - IoU(decode(r), decode(t))) ],  t = y_reg - target_offset

The IoU is the clipped area (Sutherland-Hodgman on boxToShapely's corners, shoelace) over the union, with the rules of
pair_iou (csrc/box_geom.h): 0 for a zero extent, 0 beyond the sum of the circumradii, 0 for anything that is not finite.
Everything is vectorised over the pairs.  The gradient of the IoU term is taken by CENTRAL DIFFERENCES in r (h = 1e-6),
not by the closed form the kernel uses; the rest of the loss and of the gradient is tests/detection_loss_ref.py's."""
import math

import numpy as np

from detection_loss_ref import DEFAULTS, detection_loss, masks

ANCHORS = ((1.6, 3.9, 1.56, 0.0), (1.6, 3.9, 1.56, math.pi / 2))        # Constants.anchors: l, w, h, yaw
FD_STEP = 1e-6


def decode(v, anchors):
    """v (N,7) residuals, anchors (N,4) = (l, w, h, yaw) -> boxes (N,7) = (x, y, z, l, w, h, yaw): k_rpn_decode's
    arithmetic without the anchor centre that prediction and target share."""
    v, an = np.asarray(v, np.float64), np.asarray(anchors, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([v[:, :3] * an[:, :3], np.exp(v[:, 3:6]) * an[:, :3], v[:, 6:7] + an[:, 3:4]], axis=1)


def corners(b):
    """boxToShapely's vertices [topRight, botRight, botLeft, topLeft] of boxes (N,7) -> (N,4,2)."""
    th, l, w = b[:, 6], b[:, 3], b[:, 4]
    cs, sn = np.cos(th), np.sin(th)
    rx, ry = b[:, 0] + cs * (w / 2), b[:, 1] - sn * (w / 2)
    lx, ly = b[:, 0] - cs * (w / 2), b[:, 1] + sn * (w / 2)
    sx, sy = sn * (l / 2), cs * (l / 2)
    return np.stack([np.stack([rx + sx, ry + sy], 1), np.stack([rx - sx, ry - sy], 1),
                     np.stack([lx - sx, ly - sy], 1), np.stack([lx + sx, ly + sy], 1)], axis=1)


def shoelace(poly):
    """Signed area of polygons (N,K,2)."""
    nxt = np.roll(poly, -1, axis=1)
    return 0.5 * (poly[:, :, 0] * nxt[:, :, 1] - nxt[:, :, 0] * poly[:, :, 1]).sum(axis=1)


def _ccw(poly):
    flip = shoelace(poly) < 0
    out = poly.copy()
    out[flip] = poly[flip][:, ::-1]
    return out


def clipped_area(pa, qa):
    """Area of the intersection of convex quadrilaterals pa, qa (N,4,2): pa clipped by the four half-planes of qa.  A
    polygon of n vertices lives in the first n of K columns; the columns behind repeat vertex 0, which adds degenerate
    edges and no area."""
    p, q = _ccw(pa), _ccw(qa)
    N = p.shape[0]
    poly, n = p, np.full(N, 4)
    for e in range(4):
        a, b = q[:, e], q[:, (e + 1) % 4]
        ex, ey = (b[:, 0] - a[:, 0])[:, None], (b[:, 1] - a[:, 1])[:, None]
        K = poly.shape[1]
        c, d = poly, np.roll(poly, -1, axis=1)
        valid = np.arange(K)[None, :] < n[:, None]
        sc = ex * (c[:, :, 1] - a[:, None, 1]) - ey * (c[:, :, 0] - a[:, None, 0])
        sd = ex * (d[:, :, 1] - a[:, None, 1]) - ey * (d[:, :, 0] - a[:, None, 0])
        keep = valid & (sc >= 0)
        cross = valid & ((sc >= 0) != (sd >= 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(cross, sc / (sc - sd), 0.0)
        x = c + t[:, :, None] * (d - c)
        pts = np.stack([c, x], axis=2).reshape(N, 2 * K, 2)                # c_0, x_0, c_1, x_1, ...
        mask = np.stack([keep, cross], axis=2).reshape(N, 2 * K)
        order = np.argsort(~mask, axis=1, kind="stable")                   # the kept points first, in their order
        n = mask.sum(axis=1)
        K2 = max(int(n.max()), 1) if N else 1
        pts = np.take_along_axis(pts, order[:, :K2, None], axis=1)
        pad = np.arange(K2)[None, :] >= n[:, None]
        poly = np.where(pad[:, :, None], pts[:, :1], pts)
    area = np.abs(shoelace(poly))
    return np.where(n >= 3, area, 0.0)


def iou(p, g, mode="bev"):
    """IoU of boxes p, g (N,7) under '3d' / 'bev', pair_iou's rules; 0 where either box or the value is not finite."""
    p, g = np.asarray(p, np.float64).reshape(-1, 7), np.asarray(g, np.float64).reshape(-1, 7)
    ok = np.isfinite(p).all(axis=1) & np.isfinite(g).all(axis=1)
    ok &= (p[:, 3] != 0) & (p[:, 4] != 0) & (g[:, 3] != 0) & (g[:, 4] != 0)
    if mode == "3d":
        ok &= (p[:, 5] != 0) & (g[:, 5] != 0)
    with np.errstate(over="ignore", invalid="ignore"):
        rad = 0.5 * (np.hypot(p[:, 3], p[:, 4]) + np.hypot(g[:, 3], g[:, 4]))
        ok &= ~((p[:, 0] - g[:, 0]) ** 2 + (p[:, 1] - g[:, 1]) ** 2 > rad * rad * 1.0000001)
    out = np.zeros(p.shape[0])
    if not ok.any():
        return out
    P, G = p[ok], g[ok]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inter = clipped_area(corners(P), corners(G))
        sp, sg = np.abs(P[:, 3] * P[:, 4]), np.abs(G[:, 3] * G[:, 4])
        if mode == "3d":
            hp, hg = 0.5 * np.abs(P[:, 5]), 0.5 * np.abs(G[:, 5])
            inter = inter * np.maximum(0.0, np.minimum(P[:, 2] + hp, G[:, 2] + hg) - np.maximum(P[:, 2] - hp, G[:, 2] - hg))
            sp, sg = sp * np.abs(P[:, 5]), sg * np.abs(G[:, 5])
        uni = sp + sg - inter
        val = np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)
    out[ok] = np.where(np.isfinite(val), val, 0.0)
    return out


def decoded_iou(r, t, anchors, mode="bev"):
    """IoU of the decoded residual pairs r, t (N,7) against anchors (N,4)."""
    return iou(decode(r, anchors), decode(t, anchors), mode)


def iou_term_grad(r, t, anchors, mode="bev", h=FD_STEP):
    """d (1 - IoU) / d r (N,7) by central differences of step h in each of the seven residuals."""
    r = np.asarray(r, np.float64).reshape(-1, 7)
    N = r.shape[0]
    step = np.eye(7)[None, :, :] * h                                       # (1,7,7)
    plus = (r[:, None, :] + step).reshape(-1, 7)
    minus = (r[:, None, :] - step).reshape(-1, 7)
    tt = np.repeat(np.asarray(t, np.float64).reshape(-1, 7), 7, axis=0)
    an = np.repeat(np.asarray(anchors, np.float64).reshape(-1, 4), 7, axis=0)
    d = decoded_iou(plus, tt, an, mode) - decoded_iou(minus, tt, an, mode)
    return -(d / (2.0 * h)).reshape(N, 7)


def positives(head, y_cls, y_reg, target_offset=1.0, anchors=ANCHORS):
    """(cells, anchor index, r, t, anchors) of the positives in (cell, anchor) order."""
    head = np.asarray(head, np.float64).reshape(-1, 16)
    M = head.shape[0]
    pos, _ = masks(np.asarray(y_cls, np.float64).reshape(M, 2))
    m, a = np.nonzero(pos)
    r = head[:, 2:].reshape(M, 2, 7)[m, a]
    t = np.asarray(y_reg, np.float64).reshape(M, 2, 7)[m, a] - float(target_offset)
    return m, a, r, t, np.asarray(anchors, np.float64)[a]


def detection_iou_loss(head, y_cls, y_reg, weights=(1.0, 1.0), grad_scale=1.0, iou_weight=1.0, iou_mode="bev",
                       anchors=ANCHORS, h=FD_STEP, **params):
    """-> (loss [total, L_cls, L_reg], counts, dhead (M,16)), float64: detection_loss plus the IoU term and its
    central-difference gradient on the regression channels of the positives."""
    loss, counts, dhead = detection_loss(head, y_cls, y_reg, weights=weights, grad_scale=grad_scale, **params)
    off = float(dict(DEFAULTS, **params)["target_offset"])
    m, a, r, t, an = positives(head, y_cls, y_reg, off, anchors)
    npos = float(max(len(m), 1))
    wr = float(weights[1])
    term = 1.0 - decoded_iou(r, t, an, iou_mode)
    l_reg = loss[2] + float(iou_weight) * term.sum() / npos
    loss = np.array([float(weights[0]) * loss[1] + wr * l_reg, loss[1], l_reg])
    dhead = dhead.copy()
    if len(m):
        g = iou_term_grad(r, t, an, iou_mode, h) * (float(grad_scale) * wr * float(iou_weight) / npos)
        cols = 2 + 7 * a[:, None] + np.arange(7)[None, :]
        dhead[m[:, None], cols] += g
    return loss, counts, dhead
