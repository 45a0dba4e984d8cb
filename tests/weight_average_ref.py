"""The numpy definition of the weight averaging pass (include/lisec_hip.h, lisec_weight_average): every operation a
separate np.float32 operation, the coefficients from Python floats (doubles), rounded once.  The definition is this
project's restatement of tfa.optimizers.MovingAverage / SWA (parity unpinned)."""
import numpy as np

F = np.float32


def ema_decay(s, average_decay, start_step=0, dynamic_decay=False):
    """decay_s at the iteration count s before the update, a Python float."""
    if s < start_step:
        return 0.0
    if dynamic_decay:
        k = s - start_step
        return min(float(average_decay), (1.0 + k) / (10.0 + k))
    return float(average_decay)


def ema_coefficient(s, average_decay, start_step=0, dynamic_decay=False):
    """c = (float)(1.0 - decay_s): computed in double, rounded once."""
    return F(1.0 - ema_decay(s, average_decay, start_step, dynamic_decay))


def fold_num_updates(average_decay, num_updates):
    """tfa's constructor argument num_updates, folded on the host before the descriptor is built."""
    if num_updates is None:
        return float(average_decay)
    return min(float(average_decay), (1.0 + num_updates) / (10.0 + num_updates))


def ema_step(a, w, s, average_decay, start_step=0, dynamic_decay=False):
    """a after the pass that follows the update made at iteration count s; w: the variables after that update."""
    a, w = np.asarray(a, F), np.asarray(w, F)
    c = ema_coefficient(s, average_decay, start_step, dynamic_decay)
    if c == F(1.0):
        return w.copy()                                  # a store: a - (a - w) is not w in fp32
    d = np.subtract(a, w, dtype=F)
    p = np.multiply(d, c, dtype=F)
    return np.subtract(a, p, dtype=F)


def swa_m(s, start_averaging=0, average_period=10):
    """m of a snapshot step, -1 off a snapshot."""
    m = max(0, (s - start_averaging) // average_period)
    return m if s >= start_averaging and s == start_averaging + m * average_period else -1


def swa_step(a, w, s, start_averaging=0, average_period=10):
    a, w = np.asarray(a, F), np.asarray(w, F)
    m = swa_m(s, start_averaging, average_period)
    if m < 0:
        return a.copy()                                  # keeps its bits
    if m == 0:
        return w.copy()
    t = np.multiply(a, F(m), dtype=F)
    t = np.add(t, w, dtype=F)
    return np.divide(t, F(m + 1), dtype=F)


# ---- the forms the kernel must NOT compute (the GPU test asserts that its inputs tell them apart) ------------------------
def ema_step_fma(a, w, c):
    """a - (a - w)*c with the multiply contracted into the last subtraction (one rounding instead of two)."""
    a, w = np.asarray(a, F), np.asarray(w, F)
    d = np.subtract(a, w, dtype=F).astype(np.float64)
    return (a.astype(np.float64) - d * np.float64(c)).astype(F)      # exact in double, rounded once: the fma


def ema_step_mirrored(a, w, c):
    """a + (w - a)*c.  NOT a different form: round-to-nearest-even is symmetric under negation, so w - a = -(a - w),
    (w - a)*c = -((a - w)*c) and a + (-p) = a - p hold exactly, zeros' signs included -- the same bits for every input."""
    a, w = np.asarray(a, F), np.asarray(w, F)
    return np.add(a, np.multiply(np.subtract(w, a, dtype=F), F(c), dtype=F), dtype=F)


def ema_step_reassociated(a, w, c):
    """a*(1 - c) + w*c: the distributed form, which rounds elsewhere."""
    a, w = np.asarray(a, F), np.asarray(w, F)
    return np.add(np.multiply(a, np.subtract(F(1.0), F(c), dtype=F), dtype=F), np.multiply(w, F(c), dtype=F), dtype=F)


def swa_step_reciprocal(a, w, m):
    """(a*m + w) * (1/(m + 1))"""
    a, w = np.asarray(a, F), np.asarray(w, F)
    t = np.add(np.multiply(a, F(m), dtype=F), w, dtype=F)
    return np.multiply(t, F(1.0) / F(m + 1), dtype=F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def make_inputs(n, seed):
    """(a, w) of n floats: normal values, +-0, denormals, and pairs of very different magnitude."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(F)
    w = (a + rng.standard_normal(n).astype(F) * F(0.01)).astype(F)
    if n >= 16:
        special = rng.permutation(n)[:max(16, n // 8)]
        q = len(special) // 8
        a[special[:q]] = F(0.0)
        w[special[:q]] = F(-0.0)
        a[special[q:2 * q]] = F(-0.0)
        a[special[2 * q:3 * q]] = F(1e-41)                         # denormals
        w[special[2 * q:3 * q]] = F(-3e-42)
        w[special[3 * q:4 * q]] = F(1.4e-45)
        a[special[4 * q:5 * q]] = F(1e8)                           # very different magnitudes
        w[special[4 * q:5 * q]] = F(1.0)
        a[special[5 * q:6 * q]] = F(1e-8)
        w[special[5 * q:6 * q]] = F(3e7)
    return a, w
