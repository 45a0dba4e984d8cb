"""Synthetic sweeps for the field form of the first Conv3D (lisec_conv_field_forward, csrc/field_conv.hip) and the sparse
backward network.py::first_conv3d composes for the same layer, with their fp64 references -- TEST ONLY, plain numpy.
Shared by tests/test_field_cases.py (CPU: the builder, the bounds, an fp32 emulation of the decomposition and what a wrong
term does to it) and tests/test_gpu_field_conv.py (the kernels).

sweep() writes by hand what the voxeliser and the VFE hand to the layer: voxel ordinals sorted by cell, the cell map with -1
on empty cells AND on the cells of voxels beyond the capacity (voxelize.hip, k_cell_assign), info[NVOX] = the TRUE count,
the constant c, delta and vout of (cap + 1, 64) with vout[min(V_true, cap)] = c.  Every row of delta / vout the kernels must
not read is NaN.

Two operand kinds.  Integer: W in {-2..2}, c and delta in {-3..3}, bias in {-5..5}, stored as fp32 -- every partial sum of
any evaluation order is an integer of magnitude <= 27*64*(2*3 + 2*3) + 5 < 2^24, so the result is exact and the criterion is
BIT EQUALITY with the fp64 reference.  Normal: c, delta ~ N(0,1), W ~ N(0,1)/sqrt(taps*64), bias ~ N(0,0.1); the field form
is some summation tree over the products W*c (taps inside the grid) and W*delta (taps reading a voxel) plus the bias, so
    |got - ref| <= glue_ref.sum_bound(n, A)   elementwise,
    n = 64*(taps inside the grid) + 64*(taps reading a voxel) + 1,   A = |bias| + sum |W||c| + sum |W||delta|,
in any order, with or without fma -- n and A come from the same oracle/conv_ref.py call as the reference, over ones and over
absolute values.  Nothing here is taken from the code under test."""
import types
import zlib

import numpy as np

import glue_ref as R
from oracle import conv_ref

C = 64
NVOX, OVERFLOW = 0, 4                       # LISEC_VI_NVOX, LISEC_VI_OVERFLOW (include/lisec_hip.h)
K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
EXACT = 2.0 ** 24


def _geom(ind, outd, k, s, p):
    return dict(ind=ind, outd=outd, k=k, s=s, p=p)


G1 = _geom((8, 6, 40), (4, 6, 40), K333, (2, 1, 1), (1, 1, 1))         # the production form (model_training.py:236)
G2 = _geom((4, 5, 40), (2, 5, 40), K333, (1, 1, 1), (0, 1, 1))         # valid depth, no depth parity
G3 = _geom((2, 2, 600), (1, 2, 600), K333, (2, 1, 1), (1, 1, 1))       # one segment spans 602 cells under field_seg = 1024
G4 = _geom((8, 20, 1), (4, 20, 1), K333, (2, 1, 1), (1, 1, 1))         # one cell wide: only kw = 1 feeds an output
G_2D = _geom((1, 9, 41), (1, 9, 41), K133, (1, 1, 1), (0, 1, 1))
G_111 = _geom((2, 3, 50), (2, 3, 50), K111, (1, 1, 1), (0, 0, 0))
G_S22 = _geom((1, 9, 41), (1, 5, 21), K133, (1, 2, 2), (0, 1, 1))      # strides along h and w

# field_tpw: taps per workgroup of k_field_taps (1 or KW); field_seg: target segment length of k_field_combine (0: default).
# G1's Wo = 40 under field_seg = 16 is three segments of 14, 14 and 12 positions.
KNOBS_G1 = [dict(field_tpw=1, field_seg=0), dict(field_tpw=3, field_seg=0),
            dict(field_tpw=1, field_seg=16), dict(field_tpw=3, field_seg=16)]
# G3: two segments of 300 by default; one of 600 (staging and mask loops take two trips) under field_seg = 1024
KNOBS_G3 = [dict(field_tpw=1, field_seg=0), dict(field_tpw=3, field_seg=0),
            dict(field_tpw=1, field_seg=1024), dict(field_tpw=3, field_seg=1024)]
KNOBS_TPW = [dict(field_tpw=1, field_seg=0), dict(field_tpw=3, field_seg=0)]
SEGMENT_EDGE_W = (13, 14, 27, 28)           # the cells either side of G1's segment edges under field_seg = 16


def _case(name, geom, layout, V_true, cap, knobs):
    return dict(name=name, geom=geom, layout=layout, V_true=V_true, cap=cap, knobs=knobs)


# V_true None: the layout fixes the count
CASES = [
    _case("G1 random", G1, "random", 300, 400, KNOBS_G1),                       # tiles beyond V (m0 > V) return at once
    _case("G1 V=0", G1, "random", 0, 100, KNOBS_G1),                            # row 0 is the constant, the only row
    _case("G1 V=128", G1, "random", 128, 300, KNOBS_G1),                        # the constant row alone in its tile
    _case("G1 V=256", G1, "random", 256, 300, KNOBS_G1),
    _case("G1 V=cap", G1, "random", 200, 200, KNOBS_G1),                        # row V is the last addressable row
    _case("G1 overflow", G1, "random", 260, 200, KNOBS_G1),                     # info[NVOX] > cap: V is clamped
    _case("G1 odd planes", G1, ("planes", (1, 3)), None, 500, KNOBS_G1),        # whole tiles of one depth parity
    _case("G1 even planes", G1, ("planes", (0, 2)), None, 500, KNOBS_G1),
    _case("G1 full", G1, "full", None, 2000, KNOBS_G1),                         # 27 Z rows at interior positions
    _case("G1 faces", G1, "faces", None, 1100, KNOBS_G1),                       # every boundary class of all three axes
    _case("G2 random", G2, "random", 200, 256, KNOBS_G1),
    _case("G3 line", G3, "line0", 750, 800, KNOBS_G3),                          # tiles 0-3 hold voxels of line (0, 0) only
    _case("G4 one cell wide", G4, "random", 150, 170, KNOBS_TPW),
    _case("2D", G_2D, "random", 120, 150, KNOBS_TPW),
    _case("1x1x1", G_111, "random", 100, 120, KNOBS_TPW[:1]),
    _case("strides h w", G_S22, "random", 120, 150, KNOBS_TPW),
]
BACKWARD_CASES = ("G1 random", "G1 overflow", "G1 V=0")
SINK_CASES = ("G1 random", "G3 line")


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def rng_of(name, integer):
    return np.random.default_rng(zlib.crc32(f"{name}/{'int' if integer else 'normal'}".encode()))


def _cells(ind, V_true, rng, layout):
    """sorted flat indices (d*H + h)*W + w of the occupied cells"""
    D, H, W = ind
    ncell = D * H * W
    d, h, w = np.unravel_index(np.arange(ncell), ind)
    if layout == "full":
        cells = np.arange(ncell)
    elif layout == "faces":
        cells = np.flatnonzero((d == 0) | (d == D - 1) | (h == 0) | (h == H - 1) | (w == 0) | (w == W - 1))
    elif isinstance(layout, tuple) and layout[0] == "planes":
        cells = np.flatnonzero(np.isin(d, layout[1]))
    elif layout == "line0":                                   # line (d = 0, h = 0) full + random cells elsewhere
        rest = rng.choice(np.arange(W, ncell), V_true - W, replace=False)
        cells = np.concatenate([np.arange(W), rest])
    elif layout == "random":                                  # with the cells either side of the segment edges planted
        planted = np.array([], dtype=np.int64)
        if W > max(SEGMENT_EDGE_W) and V_true >= len(SEGMENT_EDGE_W):
            planted = (min(1, D - 1) * H + min(2, H - 1)) * W + np.array(SEGMENT_EDGE_W)
        others = np.setdiff1d(np.arange(ncell), planted)
        cells = np.concatenate([planted, rng.choice(others, V_true - len(planted), replace=False)])
    else:
        raise ValueError(layout)
    cells = np.sort(cells)
    assert V_true is None or len(cells) == V_true
    assert len(np.unique(cells)) == len(cells)
    return cells


def sweep(ind, V_true, cap, rng, layout="random", integer=False):
    """What the voxeliser and the VFE hand to the first Conv3D, as host arrays (a SimpleNamespace):
    cells int32 (cap,) / coords int32 (cap, 3) = (d, h, w) sorted by cell, rows >= V = min(V_true, cap) zero;
    cell_voxel int32 [D*H*W]; info int32[8]; c (64,); delta, vout (cap + 1, 64) with NaN on every row that must not be read;
    grid: the materialised fp64 map (c everywhere, c + delta on the occupied cells)."""
    all_cells = _cells(ind, V_true, rng, layout)
    V_true = len(all_cells)
    V = min(V_true, cap)
    ncell = ind[0] * ind[1] * ind[2]
    cells = np.zeros(cap, np.int32)
    cells[:V] = all_cells[:V]
    coords = np.zeros((cap, 3), np.int32)
    coords[:V] = np.stack(np.unravel_index(all_cells[:V], ind), 1)
    cell_voxel = np.full(ncell, -1, np.int32)
    cell_voxel[all_cells[:V]] = np.arange(V)                  # voxels beyond the capacity leave -1
    info = np.zeros(8, np.int32)
    info[NVOX], info[OVERFLOW] = V_true, int(V_true > cap)
    if integer:
        c = rng.integers(-3, 4, C).astype(np.float32)
        d = rng.integers(-3, 4, (V, C)).astype(np.float32)
    else:
        c = rng.normal(0, 1, C).astype(np.float32)
        d = rng.normal(0, 1, (V, C)).astype(np.float32)
    delta = np.full((cap + 1, C), np.nan, np.float32)
    vout = np.full((cap + 1, C), np.nan, np.float32)
    delta[:V] = d
    vout[:V] = c + d
    vout[V] = c
    grid = np.empty((ncell, C), np.float64)
    grid[:] = c
    grid[all_cells[:V]] += d.astype(np.float64)
    return types.SimpleNamespace(ind=ind, V=V, V_true=V_true, cap=cap, cells=cells, coords=coords, cell_voxel=cell_voxel,
                                 info=info, c=c, delta=delta, vout=vout, grid=grid.reshape(*ind, C))


def weights(k, rng, integer=False):
    """W (taps, 64, 64) in the Keras order (tap, in, out), bias (64,), float32"""
    taps = k[0] * k[1] * k[2]
    if integer:
        return rng.integers(-2, 3, (taps, C, C)).astype(np.float32), rng.integers(-5, 6, C).astype(np.float32)
    return ((rng.normal(0, 1, (taps, C, C)) / np.sqrt(taps * C)).astype(np.float32), rng.normal(0, 0.1, C).astype(np.float32))


def draw(case, integer):
    """(sweep, W, bias) of a case, from a generator seeded by its name and operand kind"""
    rng = rng_of(case["name"], integer)
    sw = sweep(case["geom"]["ind"], case["V_true"], case["cap"], rng, layout=case["layout"], integer=integer)
    W, bias = weights(case["geom"]["k"], rng, integer)
    return sw, W, bias


def _conv_args(geo):
    return geo["outd"], geo["k"], geo["s"], geo["p"]


def reference(sw, geo, W, bias=None, bounds=False):
    """y (Do, Ho, Wo, 64) fp64 = the dense convolution of the materialised grid (+ bias); with bounds also n (.., 1) and A
    (.., 64) of the module docstring, from the same conv_ref call over ones and over absolute values."""
    ref = conv_ref.conv_forward(sw.grid, W, *_conv_args(geo), bias=bias)
    if not bounds:
        return ref
    V = sw.V
    mag = np.empty((sw.cell_voxel.size, C), np.float64)
    mag[:] = np.abs(sw.c)
    mag[sw.cells[:V]] += np.abs(sw.delta[:V]).astype(np.float64)
    A = conv_ref.conv_forward(mag.reshape(*sw.ind, C), np.abs(W), *_conv_args(geo), bias=None if bias is None else np.abs(bias))
    ones = 1.0 + (sw.cell_voxel >= 0).reshape(*sw.ind, 1)     # one term set for the constant, one more where a voxel sits
    taps = W.shape[0]
    n = C * conv_ref.conv_forward(ones, np.ones((taps, 1, 1)), *_conv_args(geo)) + (0 if bias is None else 1)
    return ref, n, A


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


TOL_L2 = 2e-6       # the bound tests/test_gpu_winograd.py and tests/test_gpu_lyft_layers.py hold the direct kernels to


def criteria(got, ref, n, A):
    """(largest err / bound, relative L2) of a normal-operand result; a NaN in `got` gives (inf, nan)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf"), float("nan")
    return float((np.abs(got - ref) / R.sum_bound(n, A)).max()), rel_l2(got, ref)


# ---- the fp32 decomposition on the host -------------------------------------------------------------------------------------
def tap_reads(sw, geo):
    """Per tap and output position: inside (taps, M) bool -- the tap reads inside the grid --, cell (taps, M) the flat cell
    it reads and voxel (taps, M) the ordinal found there (-1: none / outside)."""
    (Do, Ho, Wo), (KD, KH, KW), s, p = _conv_args(geo)
    Di, Hi, Wi = geo["ind"]
    cv = sw.cell_voxel.reshape(Di, Hi, Wi)
    inside, cell, voxel = [], [], []
    axis = lambda n_out, k, a, n_in: np.arange(n_out) * s[a] - p[a] + k
    for kd in range(KD):
        xd = axis(Do, kd, 0, Di)
        for kh in range(KH):
            xh = axis(Ho, kh, 1, Hi)
            for kw in range(KW):
                xw = axis(Wo, kw, 2, Wi)
                ok = (((xd >= 0) & (xd < Di))[:, None, None] & ((xh >= 0) & (xh < Hi))[None, :, None] &
                      ((xw >= 0) & (xw < Wi))[None, None, :])
                d, h, w = np.clip(xd, 0, Di - 1)[:, None, None], np.clip(xh, 0, Hi - 1)[None, :, None], np.clip(xw, 0, Wi - 1)[None, None, :]
                inside.append(ok.ravel())
                cell.append(np.where(ok, (d * Hi + h) * Wi + w, -1).ravel())
                voxel.append(np.where(ok, cv[d, h, w], -1).ravel())
    return np.stack(inside), np.stack(cell), np.stack(voxel)


def emulate(sw, geo, W, bias, voxel=None):
    """The field decomposition in fp32: Z[tap] = delta @ W[tap] and Zc[tap] = c @ W[tap] as fp32 products, then sequential
    fp32 adds per output position: bias, the constant rows of the taps inside the grid, the Z rows of the taps that read a
    voxel, in tap order.  voxel: a replacement for tap_reads()'s ordinals (the mutations of test_field_cases.py)."""
    inside, _, vox = tap_reads(sw, geo)
    if voxel is not None:
        vox = voxel
    W32, V = W.astype(np.float32), sw.V
    M = inside.shape[1]
    val = np.zeros((M, C), np.float32)
    if bias is not None:
        val += bias.astype(np.float32)
    for t in range(W.shape[0]):
        val[inside[t]] += sw.c @ W32[t]
    for t in range(W.shape[0]):
        hit = vox[t] >= 0
        if hit.any():
            val[hit] += (sw.delta[:V] @ W32[t])[vox[t][hit]]
    assert val.dtype == np.float32
    return val.reshape(*geo["outd"], C)


def dropped_term(sw, geo):
    """tap_reads()'s ordinals with ONE (tap, position) term removed, or None when no tap reads a voxel."""
    _, _, vox = tap_reads(sw, geo)
    hits = np.argwhere(vox >= 0)
    if not len(hits):
        return None
    t, m = hits[len(hits) // 2]
    vox = vox.copy()
    vox[t, m] = -1
    return vox


def misplaced_term(sw, geo):
    """tap_reads()'s ordinals with ONE term taken from a neighbouring occupied cell (along w; along h, then d, where the line
    offers none), or None when no term has such a neighbour."""
    _, cell, vox = tap_reads(sw, geo)
    Di, Hi, Wi = geo["ind"]
    hits = np.argwhere(vox >= 0)
    order = np.roll(np.arange(len(hits)), -(len(hits) // 2))
    for t, m in hits[order]:
        c0 = int(cell[t, m])
        for off in (1, -1, Wi, -Wi, Hi * Wi, -Hi * Wi):
            c1 = c0 + off
            if c1 < 0 or c1 >= sw.cell_voxel.size or (abs(off) == 1 and c1 // Wi != c0 // Wi):
                continue
            if abs(off) == Wi and c1 // (Hi * Wi) != c0 // (Hi * Wi):
                continue
            if sw.cell_voxel[c1] >= 0:
                vox = vox.copy()
                vox[t, m] = sw.cell_voxel[c1]
                return vox
    return None


# ---- the sparse backward of the same layer ----------------------------------------------------------------------------------
def draw_dy(case, geo):
    """dy in {-3..3} over the output map, float32"""
    rng = np.random.default_rng(zlib.crc32(f"{case['name']}/dy".encode()))
    return rng.integers(-3, 4, (*geo["outd"], C)).astype(np.float32)


def backward_reference(sw, geo, W, dy):
    """The dense definition in fp64 on the materialised grid: S (taps, 64) the tap-inside sums of dy, dW (taps, grid channel,
    output channel), rows (V, 64) the grid gradient at the occupied cells, g_all (64,) its sum over ALL cells; and `largest`,
    the largest sum of absolute values behind any of them (below 2^24: every partial sum of integer operands is exact)."""
    a = _conv_args(geo)
    V = sw.V
    S, S_mag = R.tap_inside_sums(dy, geo["ind"], geo["k"], geo["s"], geo["p"])
    dW = conv_ref.conv_wgrad(sw.grid, dy, *a)
    Wt = np.transpose(W, (0, 2, 1))
    gg = conv_ref.conv_forward(dy, Wt, geo["ind"], geo["k"], geo["s"], geo["p"], mode=1).reshape(-1, C)
    mag = np.empty((sw.cell_voxel.size, C), np.float64)
    mag[:] = np.abs(sw.c)
    mag[sw.cells[:V]] += np.abs(sw.delta[:V]).astype(np.float64)
    dW_mag = conv_ref.conv_wgrad(mag.reshape(*sw.ind, C), np.abs(dy), *a)
    gg_mag = conv_ref.conv_forward(np.abs(dy), np.abs(Wt), geo["ind"], geo["k"], geo["s"], geo["p"], mode=1).reshape(-1, C)
    largest = max(S_mag.max(), dW_mag.max(), gg_mag.sum(0).max())
    return dict(S=S, dW=dW, rows=gg[sw.cells[:V]], g_all=gg.sum(0), largest=float(largest))
