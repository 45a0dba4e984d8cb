"""LAMB (optimizers.LAMB; the rule of include/lisec_hip.h) in numpy float64, per variable: the definition the GPU tests
hold the kernels of csrc/lamb.hip to.  No import from lisec_amd."""
import numpy as np


def lr_t(lr, decay, iterations):
    return lr / (1.0 + decay * iterations)


def step(theta, m, v, grad, variables, iterations, lr, decay=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-6,
         weight_decay_rate=0.0):
    """One update.  theta, m, v, grad: float64 arrays of one length; variables: [(offset, count, decayed, adapted)].
    Returns (theta, m, v, ratios) -- new arrays, ratios one per variable; floats outside every variable are copied."""
    theta, m, v = (np.array(a, dtype=np.float64) for a in (theta, m, v))
    grad = np.asarray(grad, dtype=np.float64)
    t = iterations + 1
    rate = lr_t(lr, decay, iterations)
    ratios = np.ones(len(variables))
    for j, (off, count, decayed, adapted) in enumerate(variables):
        s = slice(off, off + count)
        g, w = grad[s], theta[s]
        m[s] = beta_1 * m[s] + (1.0 - beta_1) * g
        v[s] = beta_2 * v[s] + (1.0 - beta_2) * g * g
        u = (m[s] / (1.0 - beta_1 ** t)) / (np.sqrt(v[s] / (1.0 - beta_2 ** t)) + epsilon)
        if decayed:
            u = u + weight_decay_rate * w
        nw, nu = np.sqrt(np.sum(w * w)), np.sqrt(np.sum(u * u))
        r = nw / nu if adapted and nw > 0 and nu > 0 else 1.0
        ratios[j] = r
        theta[s] = w - (r * rate) * u
    return theta, m, v, ratios
