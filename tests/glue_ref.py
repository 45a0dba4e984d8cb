"""Test-local float64 restatements of the kernels BETWEEN the contractions (include/lisec_hip.h) -- TEST ONLY.

Plain numpy, one function per operation, written from the formulas of the header: the composite head kernels and their
gradients, the constant-field gradients of the first middle layer with the tap-inside sums they read, the depth fold, the
BatchNormalization finalisers, and the two packed weight layouts.  A function that sums returns (value, magnitude): the
magnitude is the same expression over absolute values, the A of the rounding bound  |got - value| <= (n + 2) u A  that
holds for an fp32 sum of n products in ANY order, with or without fma (sum_bound below).
tests/test_glue_ref.py checks these against torch autograd / torch batch_norm / oracle/conv_ref.py before anything is
measured against them.
"""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
BN_EPS, BN_MOMENTUM = 1e-3, 0.99  # Keras BatchNormalization() of the reference


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def sum_bound(n, mag):
    """Worst case of an fp32 sum of n products, any order, fused or not: gamma_n <= (n + 2) u for the n used here."""
    return (n + 2) * U * mag


def once_bound(ref):
    """A value formed in fp64 and rounded once to fp32 (u |ref|), with a factor two of slack: 2^-23 |ref|."""
    return 2.0 ** -23 * np.abs(ref)


# ---- composite head kernels (lisec_head_compose / lisec_head_compose_backward) ------------------------------------------
def head_compose(up_kernel, head_w):
    """Wc[tap][c][j] = sum_n W_b[tap][n][c] H[n][j].  up_kernel (taps, Cup, Cin) -- the Keras Conv2DTranspose kernel
    (kh, kw, out, in) with the taps flattened; head_w (Cup, 16).  -> (Wc, magnitude), each (taps, Cin, 16); n = Cup."""
    W, H = _f64(up_kernel), _f64(head_w)
    return np.einsum("tnc,nj->tcj", W, H), np.einsum("tnc,nj->tcj", np.abs(W), np.abs(H))


def head_compose_bias(up_bias, head_w, bias_in=None):
    """b'[j] = bias_in[j] + sum_n bias_b[n] H[n][j]  -> (b', magnitude), each (16,); n = Cup + 1."""
    b, H = _f64(up_bias), _f64(head_w)
    b0 = np.zeros(H.shape[1]) if bias_in is None else _f64(bias_in)
    return b0 + b @ H, np.abs(b0) + np.abs(b) @ np.abs(H)


def head_compose_backward(G, up_kernel, up_bias, head_w, S):
    """From G = dL/dWc (taps, Cin, 16) and S[j] = sum_m dhead[m][j]:
         d_up_kernel[tap][n][c] = sum_j G[tap][c][j] H[n][j]                                   n = 16
         d_head_w[n][j]         = sum_{tap, c} W_b[tap][n][c] G[tap][c][j] + bias_b[n] S[j]    n = taps * Cin + 1
         d_up_bias[n]           = sum_j S[j] H[n][j]                                           n = 16
    up_bias None: the branch has no bias term.  -> three (value, magnitude) pairs in that order."""
    G, W, H, S = _f64(G), _f64(up_kernel), _f64(head_w), _f64(S)
    b = np.zeros(W.shape[1]) if up_bias is None else _f64(up_bias)
    dk = np.einsum("tcj,nj->tnc", G, H), np.einsum("tcj,nj->tnc", np.abs(G), np.abs(H))
    dh = (np.einsum("tnc,tcj->nj", W, G) + np.outer(b, S),
          np.einsum("tnc,tcj->nj", np.abs(W), np.abs(G)) + np.outer(np.abs(b), np.abs(S)))
    db = H @ S, np.abs(H) @ np.abs(S)
    return dk, dh, db


def head_shuffle_index(Ho, Wo, ps):
    """(pos, tap) of every head position m = h*Wo + w in a kernel == stride branch: T_b[pos][tap*16 + j]."""
    h, w = np.divmod(np.arange(Ho * Wo), Wo)
    return (h // ps) * (Wo // ps) + w // ps, (h % ps) * ps + w % ps


# ---- first middle layer: tap-inside sums and the constant-field gradients -------------------------------------------------
def tap_inside_sums(dy, in_dims, kernel, stride, pad):
    """S[tap][n] = sum of dy[m][n] over the output positions m of the mode-0 convolution whose tap reads INSIDE the input
    map (src = o*stride - pad + k in [0, n_in) on every axis).  dy (Do, Ho, Wo, C) -> (S, magnitude), each (taps, C)."""
    dy = _f64(dy)
    ok = []
    for axis in range(3):
        o = np.arange(dy.shape[axis])
        ok.append([(o * stride[axis] - pad[axis] + k >= 0) & (o * stride[axis] - pad[axis] + k < in_dims[axis])
                   for k in range(kernel[axis])])
    S, A = [], []
    for kd in range(kernel[0]):
        for kh in range(kernel[1]):
            for kw in range(kernel[2]):
                m = ok[0][kd][:, None, None] & ok[1][kh][None, :, None] & ok[2][kw][None, None, :]
                S.append(dy[m].sum(0))
                A.append(np.abs(dy[m]).sum(0))
    return np.stack(S), np.stack(A)


def const_field_g_all(W, S):
    """g_all[c] = sum_tap sum_n W[tap][c][n] S[tap][n]: the data gradient summed over ALL input positions.
    W (taps, Cin, Cout), S (taps, Cout) -> (g_all, magnitude), each (Cin,)."""
    W, S = _f64(W), _f64(S)
    return np.einsum("tcn,tn->c", W, S), np.einsum("tcn,tn->c", np.abs(W), np.abs(S))


def const_field_dw(cvec, S, dW_old=None):
    """dW[tap][c][n] = dW_old[tap][c][n] + cvec[c] S[tap][n]  (one product, one add)."""
    upd = _f64(cvec)[None, :, None] * _f64(S)[:, None, :]
    return upd if dW_old is None else _f64(dW_old) + upd


# ---- Permute((2,3,4,1)) + Reshape and its way back ------------------------------------------------------------------------
def fold_depth(x):
    """(D, HW, C) -> (HW, C*D), channel c*D + d."""
    x = np.asarray(x)
    D, HW, C = x.shape
    out = np.empty((HW, C * D), dtype=x.dtype)
    for d in range(D):
        out[:, d::D] = x[d]
    return out


def unfold_depth(g, D, mask=None):
    """(HW, C*D) -> (D, HW, C); stored as +0.0 where mask (D, HW, C) is <= 0."""
    g = np.asarray(g)
    out = np.stack([g[:, d::D] for d in range(D)])
    return out if mask is None else np.where(np.asarray(mask) > 0, out, np.zeros((), g.dtype))


# ---- BatchNormalization finalisers ------------------------------------------------------------------------------------------
def bn_state(mean, var, gamma, beta):
    inv = 1.0 / np.sqrt(_f64(var) + BN_EPS)
    scale = _f64(gamma) * inv
    return np.concatenate([scale, _f64(beta) - _f64(mean) * scale, _f64(mean), inv])


def bn_finalize(partials, n_rows, gamma, beta, moving_mean=None, moving_var=None, unbiased=False):
    """partials (nparts, 2, C) = (sum y, sum y^2) per part.  -> bnstate (4C,) {scale, shift, mean, invstd} from the batch
    mean and the BIASED batch variance (clamped at 0), and the moving statistics  m*0.99 + batch*0.01  (None without
    them); the batch variance entering the moving one is multiplied by N/(N-1) when `unbiased` and N > 1."""
    s = _f64(partials).sum(0)
    mean = s[0] / n_rows
    var = np.maximum(s[1] / n_rows - mean * mean, 0.0)
    state = bn_state(mean, var, gamma, beta)
    if moving_mean is None:
        return state, None, None
    v = var * (n_rows / (n_rows - 1.0)) if unbiased and n_rows > 1 else var
    return (state, _f64(moving_mean) * BN_MOMENTUM + mean * (1.0 - BN_MOMENTUM),
            _f64(moving_var) * BN_MOMENTUM + v * (1.0 - BN_MOMENTUM))


def bn_fold(gamma, beta, moving_mean, moving_var):
    """bnstate of inference: the moving statistics in place of the batch's."""
    return bn_state(moving_mean, moving_var, gamma, beta)


# ---- packed weight layouts ----------------------------------------------------------------------------------------------------
def packed_layout(w, group):
    """w (taps, K, N) -> dst[tap][k / group][n][k % group] with K and N zero padded to multiples of 64, flattened.
    group 4: the fp32 kernels (lisec_conv_pack_weights); group 8: the bf16 kernel (lisec_conv_pack_weights_bf16)."""
    w = np.asarray(w)
    taps, K, N = w.shape
    Kp, Np = -(-K // 64) * 64, -(-N // 64) * 64
    full = np.zeros((taps, Kp, Np), dtype=w.dtype)
    full[:, :K, :N] = w
    return np.ascontiguousarray(full.reshape(taps, Kp // group, group, Np).transpose(0, 1, 3, 2)).reshape(-1)
