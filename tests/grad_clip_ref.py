"""Gradient clipping in numpy: the three rules of include/lisec_hip.h (lisec_grad_clip_*), written from the definition and
importing nothing of lisec_amd.  g: a flat float32 array; variables: [(offset, count)] in floats, the variables the
norms are taken over; what lies outside every variable is never touched.  The sum of squares is taken in float64 over
the float32 inputs (every product exact), the scale formed in float64 and rounded once."""
import numpy as np

F = np.float32


def clip_by_value(g, c, variables=None):
    """g <- c where g > c, g <- -c where g < -c; every other element (a NaN, a -0, a denormal) keeps its bits."""
    c = F(c)
    out = np.array(g, dtype=F, copy=True)
    for off, n in [(0, out.size)] if variables is None else variables:
        v = out[off:off + n]                      # a view
        src = v.copy()
        with np.errstate(invalid="ignore"):       # (a signalling NaN compares false like any other)
            v[src > c] = c
            v[src < -c] = -c
    return out


def sum_squares(x):
    """sum x*x in float64 over float32 inputs."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(x, dtype=F).astype(np.float64)
        return np.sum(x * x, dtype=np.float64)


def scale_of(S, c):
    """(scale, norm) as float32 of the float64 sum of squares S and the threshold c (taken as a float32): NaN when S is
    not finite; exactly 1 when sqrt(S) <= c; else float32(c / sqrt(S))."""
    c = np.float64(F(c))
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.sqrt(np.float64(S))
        norm = F(n)
        if not np.isfinite(S):
            return F(np.nan), norm
        return (F(c / n) if n > c else F(1.0)), norm


def scaled(x, scale):
    """x*scale, one float32 multiply per element; a scale of exactly 1 leaves x alone (its bits)."""
    x = np.asarray(x, dtype=F)
    if scale == F(1.0):
        return x.copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (x * F(scale)).astype(F)


def clip_by_norm(g, c, variables):
    """Every variable scaled so that its L2 norm is at most c.  Returns (clipped, scales, norms), one scale and norm
    per variable."""
    out = np.array(g, dtype=F, copy=True)
    scales, norms = np.empty(len(variables), F), np.empty(len(variables), F)
    for j, (off, n) in enumerate(variables):
        scales[j], norms[j] = scale_of(sum_squares(out[off:off + n]), c)
        out[off:off + n] = scaled(out[off:off + n], scales[j])
    return out, scales, norms


def clip_by_global_norm(g, c, variables):
    """Everything scaled by ONE factor so that the L2 norm over all variables is at most c.  Returns (clipped, scale,
    norm)."""
    out = np.array(g, dtype=F, copy=True)
    S = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for off, n in variables:
            S = S + sum_squares(out[off:off + n])
    scale, norm = scale_of(S, c)
    for off, n in variables:
        out[off:off + n] = scaled(out[off:off + n], scale)
    return out, scale, norm


def clip(kind, g, c, variables):
    """The clipped gradient alone, by kind: 'value', 'norm' or 'global_norm'."""
    if kind == "value":
        return clip_by_value(g, c, variables)
    return {"norm": clip_by_norm, "global_norm": clip_by_global_norm}[kind](g, c, variables)[0]
