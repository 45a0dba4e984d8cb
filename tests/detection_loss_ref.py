"""The fp64 definition of the VoxelNet detection loss (include/lisec_hip.h, lisec_detection_loss): loss, counts and
gradient in numpy, from the formulas of the header and nothing of the kernels.

head (M,16): head[:, a] is the class logit z of anchor a (two anchors), head[:, 2+7a+k] its regression output r.
y_cls (M,2): the code 0 ignore / 1 negative / 2 positive (pos = code > 1.5, neg = 0.5 < code <= 1.5).  y_reg (M,14): the
targets, carrying target_offset on positives.  With p = sigmoid(z), sp(x) = max(x,0) + log1p(exp(-|x|)):

    L_cls = alpha/N_pos sum_pos (1-p)^gamma sp(-z) + beta/N_neg sum_neg p^gamma sp(z)
    L_reg = 1/N_pos sum_pos sum_k S(r - (y_reg - target_offset)),   S(d) = |d| < b ? d*d/(2b) : |d| - b/2
    total = w_c*L_cls + w_r*L_reg

A count of 0 divides as 1.  sigmoid and 1 - sigmoid are both formed from exp(-|z|), so neither cancels and no finite
logit overflows."""
import numpy as np

DEFAULTS = dict(alpha=1.5, beta=1.0, gamma=0.0, smooth_l1_beta=1.0, target_offset=1.0)


def masks(y_cls):
    y = np.asarray(y_cls, np.float64)
    return y > 1.5, (y > 0.5) & (y <= 1.5)


def _sigmoids(z):
    """(sigmoid(z), 1 - sigmoid(z), exp(-|z|))"""
    e = np.exp(-np.abs(z))
    lo, hi = e / (1.0 + e), 1.0 / (1.0 + e)
    return np.where(z >= 0, hi, lo), np.where(z >= 0, lo, hi), e


def _softplus(x, e):
    return np.maximum(x, 0.0) + np.log1p(e)


def detection_loss(head, y_cls, y_reg, weights=(1.0, 1.0), grad_scale=1.0, **params):
    """-> (loss [total, L_cls, L_reg], counts [N_pos, N_neg], dhead (M,16) = grad_scale * d total / d head), float64."""
    P = dict(DEFAULTS, **params)
    a_, b_, g, sb, off = (float(P[k]) for k in ("alpha", "beta", "gamma", "smooth_l1_beta", "target_offset"))
    wc, wr = (float(w) for w in weights)
    head = np.asarray(head, np.float64).reshape(-1, 16)
    M = head.shape[0]
    y_cls = np.asarray(y_cls, np.float64).reshape(M, 2)
    y_reg = np.asarray(y_reg, np.float64).reshape(M, 2, 7)
    pos, neg = masks(y_cls)
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    dp, dn = float(max(n_pos, 1)), float(max(n_neg, 1))
    z = head[:, :2]
    r = head[:, 2:].reshape(M, 2, 7)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p, q, e = _sigmoids(z)
        sp_pos, sp_neg = _softplus(-z, e), _softplus(z, e)
        if g == 0.0:
            v_pos, v_neg = sp_pos, sp_neg
            g_pos, g_neg = -q, p
        else:
            fq, fp = np.power(q, g), np.power(p, g)
            v_pos, v_neg = fq * sp_pos, fp * sp_neg
            g_pos = -fq * (g * p * sp_pos + q)
            g_neg = fp * (g * q * sp_neg + p)
        d = r - (y_reg - off)
        ad = np.abs(d)
        s = np.where(ad < sb, d * d / (2.0 * sb), ad - 0.5 * sb)
        ds = np.where(ad < sb, d / sb, np.sign(d))
    l_cls = a_ / dp * v_pos[pos].sum() + b_ / dn * v_neg[neg].sum()
    l_reg = s[pos].sum() / dp
    loss = np.array([wc * l_cls + wr * l_reg, l_cls, l_reg])
    dhead = np.zeros((M, 16))
    dz = np.zeros((M, 2))
    dz[pos] = (wc * a_ / dp) * g_pos[pos]
    dz[neg] = (wc * b_ / dn) * g_neg[neg]
    dr = np.zeros((M, 2, 7))
    dr[pos] = (wr / dp) * ds[pos]
    dhead[:, :2] = dz
    dhead[:, 2:] = dr.reshape(M, 14)
    return loss, np.array([n_pos, n_neg], np.int64), float(grad_scale) * dhead


def loss_only(head, y_cls, y_reg, **kw):
    return detection_loss(head, y_cls, y_reg, **kw)[0]
