"""Test-local float64 definitions of the detection metrics (lisec_detection_metrics, lisec_amd/metrics.py) -- TEST ONLY.

Plain numpy, one expression or loop per metric, written from the table of include/lisec_hip.h.  Each function returns the
pair (num, den) of one sweep; value() pools pairs.  head (M,16): head[:, a] the class logit of anchor a, head[:, 2+7a+k] its
regression output; y_cls (M,2) the 0 / 1 / 2 code; y_reg (M,14) the targets carrying target_offset.  The IoU of a pair is
tests/detection_ap_ref.pair_iou on the two boxes decoded against the anchor of their channel block.
"""
import math

import numpy as np

from detection_ap_ref import pair_iou
from detection_loss_ref import masks

ANCHORS = ((1.6, 3.9, 1.56, 0.0), (1.6, 3.9, 1.56, math.pi / 2))        # Constants.anchors: l, w, h, yaw


def _head(head):
    return np.asarray(head, np.float64).reshape(-1, 16)


def sigmoid(z):
    """In the overflow-free form of k_det_loss: exp(-|z|) lies in (0, 1]; a NaN stays a NaN."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def predicted(head, threshold):
    """(M,2) bool: p > threshold; a NaN logit compares false."""
    with np.errstate(invalid="ignore"):
        return sigmoid(_head(head)[:, :2]) > threshold


def anchor_precision(head, y_cls, threshold=0.5):
    pos, neg = masks(np.asarray(y_cls).reshape(-1, 2))
    pred = predicted(head, threshold)
    return float((pos & pred).sum()), float(((pos | neg) & pred).sum())


def anchor_recall(head, y_cls, threshold=0.5):
    pos, _ = masks(np.asarray(y_cls).reshape(-1, 2))
    return float((pos & predicted(head, threshold)).sum()), float(pos.sum())


def anchor_accuracy(head, y_cls, threshold=0.5):
    pos, neg = masks(np.asarray(y_cls).reshape(-1, 2))
    pred = predicted(head, threshold)
    return float((pos & pred).sum() + (neg & ~pred).sum()), float(pos.sum() + neg.sum())


def _residuals(head, y_reg, target_offset):
    """r, t as (M,2,7) float64."""
    r = _head(head)[:, 2:].reshape(-1, 2, 7)
    t = np.asarray(y_reg, np.float64).reshape(-1, 2, 7) - float(target_offset)
    return r, t


def positive_mae(head, y_cls, y_reg, target_offset=1.0):
    pos, _ = masks(np.asarray(y_cls).reshape(-1, 2))
    r, t = _residuals(head, y_reg, target_offset)
    return float(np.abs(r - t)[pos].sum()), 7.0 * float(pos.sum())


def decode(v, anchor):
    """k_rpn_decode's arithmetic without the anchor centre (and the +1 of z) that prediction and target share."""
    l, w, h, yaw = anchor
    with np.errstate(over="ignore"):
        return np.array([v[0] * l, v[1] * w, v[2] * h, np.exp(v[3]) * l, np.exp(v[4]) * w, np.exp(v[5]) * h, v[6] + yaw])


def decoded_iou(r, t, anchor, mode="bev"):
    """IoU of one positive; 0 when a decoded offset or extent, or the IoU itself, is not finite (a yaw that is not finite
    has no footprint, hence no finite IoU)."""
    p, g = decode(r, anchor), decode(t, anchor)
    if not (np.isfinite(p).all() and np.isfinite(g).all()):
        return 0.0
    iou = pair_iou(p, g, mode)[0]
    return float(iou) if math.isfinite(iou) else 0.0


def positive_ious(head, y_cls, y_reg, mode="bev", target_offset=1.0, anchors=ANCHORS):
    """The IoU of every positive, in (cell, anchor) order."""
    pos, _ = masks(np.asarray(y_cls).reshape(-1, 2))
    r, t = _residuals(head, y_reg, target_offset)
    return np.array([decoded_iou(r[m, a], t[m, a], anchors[a], mode) for m, a in zip(*np.nonzero(pos))], np.float64)


def positive_iou(head, y_cls, y_reg, mode="bev", target_offset=1.0, anchors=ANCHORS):
    ious = positive_ious(head, y_cls, y_reg, mode, target_offset, anchors)
    return float(ious.sum()), float(len(ious))


def pair(name, head, y_cls, y_reg, threshold=0.5, mode="bev", target_offset=1.0):
    """(num, den) of the metric with the given default name."""
    if name == "anchor_precision":
        return anchor_precision(head, y_cls, threshold)
    if name == "anchor_recall":
        return anchor_recall(head, y_cls, threshold)
    if name == "anchor_accuracy":
        return anchor_accuracy(head, y_cls, threshold)
    if name == "positive_mae":
        return positive_mae(head, y_cls, y_reg, target_offset)
    if name == "positive_iou":
        return positive_iou(head, y_cls, y_reg, mode, target_offset)
    raise ValueError(name)


def value(pairs):
    """num/den of (num, den) pairs pooled over sweeps; 0.0 when den == 0."""
    num, den = (float(sum(p[k] for p in pairs)) for k in (0, 1))
    return num / den if den != 0 else 0.0
