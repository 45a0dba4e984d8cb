"""The numpy definition of the BatchNormalization recalibration (include/lisec_hip.h, lisec_bn_recalibrate_take /
lisec_bn_recalibrate_finish): every line one IEEE fp64 operation of its own, in the order of the header, the results
rounded once to float32.  A table is a list of rows (mean_off, var_off, C, coef); `state` a float32 array, changed in
place as the kernels change it; acc a float64 array of three planes of N = sum(C) each: S1, S2, Sq.  A float64 `state`
is taken too: the same rule without the two float32 roundings (what the arithmetic alone gives)."""
import numpy as np

COEF_CONV = 1.0 - 0.99                               # lisec_bn_finalize and the conv sinks: 0.99 as a double
COEF_VFE = 1.0 - float(np.float32(0.99))             # the VFE finaliser: 0.99f widened to double


def channels(table):
    return sum(int(r[2]) for r in table)


def new_acc(table):
    return np.zeros(3 * channels(table), dtype=np.float64)


def take(state, table, acc):
    """One sweep: S1 += m, S2 += v, Sq += m*m with m, v = state / coef in fp64; the statistics are zeroed (+0)."""
    assert state.dtype in (np.float32, np.float64) and acc.dtype == np.float64
    n, base = channels(table), 0
    for mean_off, var_off, C, coef in table:
        coef = np.float64(coef)
        m = state[mean_off:mean_off + C].astype(np.float64) / coef
        v = state[var_off:var_off + C].astype(np.float64) / coef
        mm = m * m
        acc[base:base + C] = acc[base:base + C] + m
        acc[n + base:n + base + C] = acc[n + base:n + base + C] + v
        acc[2 * n + base:2 * n + base + C] = acc[2 * n + base:2 * n + base + C] + mm
        state[mean_off:mean_off + C] = 0.0
        state[var_off:var_off + C] = 0.0
        base += C


def finish(state, table, acc, sweeps, statistics="mean"):
    """mean = S1/k; 'mean': var = S2/k; 'pooled': var = max(0, (S2/k + Sq/k) - mean*mean); one rounding to state's type."""
    if statistics not in ("mean", "pooled"):
        raise ValueError(f"statistics must be 'mean' or 'pooled', not {statistics!r}")
    assert state.dtype in (np.float32, np.float64) and acc.dtype == np.float64 and sweeps >= 1
    n, base, k = channels(table), 0, np.float64(sweeps)
    with np.errstate(over="ignore", invalid="ignore"):
        for mean_off, var_off, C, _ in table:
            m = acc[base:base + C] / k
            v = acc[n + base:n + base + C] / k
            if statistics == "pooled":
                q = acc[2 * n + base:2 * n + base + C] / k
                s = v + q
                mm = m * m
                v = s - mm
                v = np.where(v < 0.0, np.float64(0.0), v)
            state[mean_off:mean_off + C] = m.astype(state.dtype)
            state[var_off:var_off + C] = v.astype(state.dtype)
            base += C


def recalibrate(states, table, statistics="mean"):
    """The whole pass over per-sweep states (each what a training forward leaves in a zeroed buffer): the final state
    (pads: those of the first) and the accumulator."""
    acc = new_acc(table)
    for s in states:
        work = s.copy()
        take(work, table, acc)
    out = states[0].copy()
    finish(out, table, acc, len(states), statistics)
    return out, acc


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
