"""The numpy definition of the decoupled weight decay pass (include/lisec_hip.h, lisec_weight_decay): a float32 product,
then a float32 subtraction, the coefficient from the float64 schedule of lisec_amd.lr_schedules rounded once.  The rule is
this project's restatement of tfa.optimizers.DecoupledWeightDecayExtension (parity unpinned)."""
import numpy as np

F = np.float32
SEED = 31


def cases():
    """{name: (weight_decay, iteration counts)} of the kernel tests: a constant, a piecewise-constant schedule across a
    boundary, a cosine at s = 0, mid-way and past decay_steps.  Every coefficient is large enough (>= 0.01) for a
    thousand inputs to tell the definition from an fma -- the two differ in roughly wd_t/2 of the elements -- and none
    is a power of two, whose product is exact (tests/test_weight_decay.py checks that they do)."""
    from lisec_amd import lr_schedules as S
    return {"constant": (0.03, (0, 7)),
            "piecewise": (S.PiecewiseConstantDecay([5], [0.3, 0.05]), (5, 6)),
            "cosine": (S.CosineDecay(0.1, 40, alpha=0.1), (0, 20, 55))}


def coefficient(weight_decay, s):
    """wd_t = (float)schedule(s) at the iteration count s before the update: a number as it is, a LearningRateSchedule
    evaluated in double (its __call__), rounded once."""
    return F(weight_decay(s)) if callable(weight_decay) else F(float(weight_decay))


def step(w, wd_t):
    """w after the pass: p = wd_t * w, then w - p, two float32 operations; wd_t == 0 keeps every bit (also of a -0)."""
    w, wd_t = np.asarray(w, F), F(wd_t)
    if wd_t == F(0.0):
        return w.copy()
    with np.errstate(all="ignore"):
        p = np.multiply(wd_t, w, dtype=F)
        return np.subtract(w, p, dtype=F)


def steps(w, weight_decay, counts):
    """step() iterated over the iteration counts `counts`."""
    for s in counts:
        w = step(w, coefficient(weight_decay, s))
    return np.asarray(w, F)


# ---- the forms the kernel must NOT compute (tests/test_weight_decay.py asserts that the inputs tell them apart) ----------
def step_fma(w, wd_t):
    """w - wd_t*w with the multiply contracted into the subtraction: worked out in double, rounded once."""
    w = np.asarray(w, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return (w - np.float64(F(wd_t)) * w).astype(F)


def step_scaled(w, wd_t):
    """w*(1 - wd_t), worked out in double and rounded once."""
    w = np.asarray(w, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return (w * (1.0 - np.float64(F(wd_t)))).astype(F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def same(got, want):
    """Bit for bit, except that a NaN may be any NaN: IEEE 754 leaves the sign and the payload of the NaN an operation
    produces (inf - inf) or passes on to the implementation, and numpy on the host and the GPU choose differently."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def make_inputs(n, seed):
    """n floats: normal values, +-0, denormals, values whose product with a small coefficient is a denormal, large and
    small magnitudes, +-inf and NaN (from 16 floats on)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(F)
    if n >= 16:
        special = rng.permutation(n)[:max(16, n // 8)]
        q = len(special) // 8
        values = ([F(0.0), F(-0.0)], [F(1e-41), F(-3e-42), F(1.4e-45)], [F(1e-36), F(-2.5e-35)], [F(3e38), F(-1e30)],
                  [F(1e-30), F(-7e-25)], [F(np.inf), F(-np.inf)], [F(np.nan)], [F(16777216.0), F(-8388609.0)])
        for k, vals in enumerate(values):
            idx = special[k * q:(k + 1) * q]
            w[idx] = np.resize(np.array(vals, F), len(idx))
    return w
