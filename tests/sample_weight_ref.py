"""The fp64 definition of the sample-weighted losses (include/lisec_hip.h, lisec_sample_weights) -- TEST ONLY, numpy, from
the formulas of the header and nothing of the kernels.  Our own restatement of tf.keras 2.4's sample_weight at batch 1:

    Keras losses     L_o = 1/(M*C) sum_m w_o[m] sum_c v(m,c);  total = weight[0]*L_cls + weight[1]*L_reg
    weighted metric  {num, den} = {sum w*v, sum w} over the elements of the output (over its cells for the categorical
                     accuracy); an unweighted metric has w = 1, so den is the element (cell) count
    VoxelNet loss    L_cls = alpha/N_pos sum_pos w_cls[m] (...) + beta/N_neg sum_neg w_cls[m] (...)
                     L_reg = 1/N_pos sum_pos w_reg[m] [sum_k S(...) + iou_weight (1 - IoU)];  the counts stay unweighted

A weight is None (1), a number (the sweep's weight) or an array of M numbers (one per cell).  The element values v and
their derivatives are those of tests/test_keras_losses.py (ref_elem); the IoU and its central-difference gradient are those
of tests/detection_iou_loss_ref.py."""
import numpy as np

import detection_iou_loss_ref as IOU
from lisec_amd import losses as K
from test_keras_losses import ref_elem


def cell_weights(w, M):
    """None, a number or M numbers -> float64 (M,)."""
    if w is None:
        return np.ones(M)
    w = np.asarray(w, np.float64).reshape(-1)
    if w.size == 1:
        return np.full(M, w[0])
    assert w.size == M
    return w


def div_no_nan(num, den):
    return float(num / den) if den != 0 else 0.0


def head_loss(spec, head, yc, yr, w=(None, None), weighted=((), ()), grad_scale=1.0):
    """-> (loss [total, L_cls, L_reg], pairs (n_metrics, 2) = {num, den} in metrics_names order, dhead (M,16)), float64.
    weighted[o]: the indices of the metrics of output o that take the weights."""
    head = np.asarray(head, np.float64).reshape(-1, 16)
    M = head.shape[0]
    outs = [(head[:, :2], np.asarray(yc, np.float64).reshape(M, 2)), (head[:, 2:], np.asarray(yr, np.float64).reshape(M, 14))]
    vals, grads, pairs = [], [], []
    for o, (p, t) in enumerate(outs):
        C = p.shape[1]
        wo = cell_weights(w[o], M)
        v, g = ref_elem(spec.losses[o], p, t)
        with np.errstate(invalid="ignore"):
            vals.append((wo[:, None] * v).sum() / (M * C))
            grads.append(grad_scale * spec.weights[o] * wo[:, None] * g / (M * C))
        for j, term in enumerate(spec.metrics[o]):
            mw = wo if j in weighted[o] else np.ones(M)
            if term[0] == K.CATEGORICAL_ACCURACY:
                hit = (np.argmax(p, -1) == np.argmax(t, -1)).astype(np.float64)
                pairs.append(((mw * hit).sum(), mw.sum()))
            else:
                pairs.append(((mw[:, None] * ref_elem(term, p, t)[0]).sum(), mw.sum() * C))
    total = spec.weights[0] * vals[0] + spec.weights[1] * vals[1]
    return np.array([total, vals[0], vals[1]]), np.array(pairs, np.float64).reshape(-1, 2), np.concatenate(grads, 1)


def _sigmoid_parts(z):
    """(sigmoid(z), 1 - sigmoid(z), log(1 + exp(-|z|))), neither sigmoid cancelling."""
    e = np.exp(-np.abs(z))
    lo, hi = e / (1.0 + e), 1.0 / (1.0 + e)
    return np.where(z >= 0, hi, lo), np.where(z >= 0, lo, hi), np.log1p(e)


def detection_loss(head, y_cls, y_reg, w=(None, None), weights=(1.0, 1.0), grad_scale=1.0, alpha=1.5, beta=1.0, gamma=0.0,
                   smooth_l1_beta=1.0, target_offset=1.0, iou=None):
    """-> (loss [total, L_cls, L_reg], counts [N_pos, N_neg], dhead (M,16)), float64.  iou: None, or dict(iou_weight,
    iou_mode, anchors (optional)) for the IoU term of VoxelNetIoULoss."""
    head = np.asarray(head, np.float64).reshape(-1, 16)
    M = head.shape[0]
    code = np.asarray(y_cls, np.float64).reshape(M, 2)
    t = np.asarray(y_reg, np.float64).reshape(M, 2, 7) - float(target_offset)
    pos, neg = code > 1.5, (code > 0.5) & (code <= 1.5)
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    dp, dn = float(max(n_pos, 1)), float(max(n_neg, 1))
    wc, wr = cell_weights(w[0], M)[:, None], cell_weights(w[1], M)[:, None]
    z, r = head[:, :2], head[:, 2:].reshape(M, 2, 7)
    with np.errstate(all="ignore"):
        p, q, l1p = _sigmoid_parts(z)
        sp_neg, sp_pos = np.maximum(z, 0.0) + l1p, np.maximum(-z, 0.0) + l1p           # sp(z), sp(-z)
        # d/dz of (1-p)^g sp(-z) and of p^g sp(z); x^0 = 1 also at x = 0
        fq, fp = (np.ones_like(q), np.ones_like(p)) if gamma == 0 else (np.power(q, gamma), np.power(p, gamma))
        v_pos, v_neg = fq * sp_pos, fp * sp_neg
        g_pos = -fq * (gamma * p * sp_pos + q)
        g_neg = fp * (gamma * q * sp_neg + p)
        d = r - t
        ad = np.abs(d)
        s = np.where(ad < smooth_l1_beta, d * d / (2.0 * smooth_l1_beta), ad - 0.5 * smooth_l1_beta)
        ds = np.where(ad < smooth_l1_beta, d / smooth_l1_beta, np.sign(d))
        l_cls = alpha / dp * (wc * v_pos)[pos].sum() + beta / dn * (wc * v_neg)[neg].sum()
        l_reg = (wr[:, :, None] * s)[pos].sum() / dp
        dz = np.zeros((M, 2))
        dz[pos] = (weights[0] * alpha / dp * wc * g_pos)[pos]
        dz[neg] = (weights[0] * beta / dn * wc * g_neg)[neg]
        dr = np.zeros((M, 2, 7))
        dr[pos] = (weights[1] / dp * wr[:, :, None] * ds)[pos]
        if iou is not None:
            anchors = iou.get("anchors", IOU.ANCHORS)
            m, a, rp, tp, an = IOU.positives(head, y_cls, y_reg, target_offset, anchors)
            if len(m):
                wm = wr[m, 0]
                term = 1.0 - IOU.decoded_iou(rp, tp, an, iou["iou_mode"])
                l_reg = l_reg + float(iou["iou_weight"]) * (wm * term).sum() / dp
                gi = IOU.iou_term_grad(rp, tp, an, iou["iou_mode"])
                dr[m, a] += (weights[1] * float(iou["iou_weight"]) / dp) * wm[:, None] * gi
    loss = np.array([weights[0] * l_cls + weights[1] * l_reg, l_cls, l_reg])
    dhead = np.concatenate([dz, dr.reshape(M, 14)], 1)
    return loss, np.array([n_pos, n_neg], np.int64), float(grad_scale) * dhead
