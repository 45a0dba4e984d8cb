"""The synthetic sweeps and references of tests/field_cases.py, before any kernel is measured against them: the builder, the
reach of the two criteria (bit equality under integer operands; the elementwise rounding bound and relative L2 <= 2e-6 under
normal ones) on an fp32 emulation of the field decomposition, and what ONE wrong term does to each.  No GPU."""
import numpy as np
import pytest

import field_cases as F
import glue_ref as R

IDS = [c["name"] for c in F.CASES]


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
@pytest.mark.parametrize("integer", [True, False], ids=["int", "normal"])
def test_builder_hands_over_what_the_voxeliser_and_the_vfe_would(case, integer):
    sw, W, bias = F.draw(case, integer)
    ind, cap, V = case["geom"]["ind"], case["cap"], sw.V
    ncell = ind[0] * ind[1] * ind[2]
    assert V == min(sw.V_true, cap) and sw.info[F.NVOX] == sw.V_true and sw.info[F.OVERFLOW] == int(sw.V_true > cap)
    assert case["V_true"] is None or sw.V_true == case["V_true"]
    assert sw.coords.shape == (cap, 3) and sw.coords.dtype == np.int32 and sw.cell_voxel.shape == (ncell,)
    flat = (sw.coords[:V, 0] * ind[1] + sw.coords[:V, 1]) * ind[2] + sw.coords[:V, 2]
    assert np.array_equal(flat, sw.cells[:V]) and (np.diff(flat) > 0).all()                # sorted by cell, no cell twice
    # the map holds the ordinals below the capacity and -1 everywhere else, the cells of overflowed voxels included
    assert np.array_equal(np.flatnonzero(sw.cell_voxel >= 0), flat) and np.array_equal(sw.cell_voxel[flat], np.arange(V))
    assert sw.cell_voxel.max(initial=-1) < max(cap, 1) and (sw.cell_voxel[sw.cell_voxel < 0] == -1).all()
    assert sw.delta.shape == sw.vout.shape == (cap + 1, F.C)
    assert np.isfinite(sw.delta[:V]).all() and np.isnan(sw.delta[V:]).all()
    assert np.array_equal(sw.vout[:V], sw.c + sw.delta[:V]) and np.array_equal(sw.vout[V], sw.c) and np.isnan(sw.vout[V + 1:]).all()
    # the materialised grid, rebuilt through the cell map: c + scattered delta
    want = np.where((sw.cell_voxel >= 0)[:, None], sw.c.astype(np.float64) + sw.delta[np.maximum(sw.cell_voxel, 0)], sw.c)
    assert np.array_equal(sw.grid.reshape(ncell, F.C), want)
    if integer:
        for a in (W, bias, sw.c, sw.delta[:V]):
            assert np.array_equal(a, np.round(a))
        assert np.abs(W).max() <= 2 and np.abs(sw.c).max() <= 3 and np.abs(sw.delta[:V]).max(initial=0) <= 3 and np.abs(bias).max() <= 5


def test_layouts_reach_what_the_cases_are_listed_for():
    V = lambda name: F.draw(F.by_name(name), True)[0]
    assert V("G1 V=0").V == 0 and V("G1 V=128").V == 128 and V("G1 V=256").V == 256
    sw = V("G1 V=cap")
    assert sw.V == sw.cap == 200
    sw = V("G1 overflow")
    assert sw.V_true == 260 and sw.V == sw.cap == 200 and (sw.cell_voxel >= 0).sum() == 200
    for name, planes in (("G1 odd planes", (1, 3)), ("G1 even planes", (0, 2))):
        sw = V(name)
        assert sw.V == 480 and set(sw.coords[:sw.V, 0]) == set(planes)
    assert V("G1 full").V == 1920 and V("G1 full").V % 128 == 0
    sw = V("G1 faces")
    co = sw.coords[:sw.V]
    for a, n in enumerate((8, 6, 40)):
        assert (co[:, a] == 0).any() and (co[:, a] == n - 1).any()
    assert sw.V == 1920 - 6 * 4 * 38
    for name in ("G1 random", "G1 V=128", "G1 V=cap", "G1 overflow"):                     # the cells at G1's segment edges
        sw = V(name)
        assert all(sw.cell_voxel[(1 * 6 + 2) * 40 + w] >= 0 for w in F.SEGMENT_EDGE_W), name
    sw = V("G3 line")
    assert sw.V == 750 and (sw.cell_voxel[:600] == np.arange(600)).all()                   # tiles 0-3: line (0, 0) only
    sw = V("G4 one cell wide")
    assert sw.V == 150 and (sw.coords[:, 2] == 0).all()


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_integer_operands_stay_exact(case):
    """Sum of absolute values behind every output element < 2^24: every partial sum of every evaluation order is an integer
    fp32 holds exactly."""
    sw, W, bias = F.draw(case, True)
    ref, n, A = F.reference(sw, case["geom"], W, bias, bounds=True)
    taps = W.shape[0]
    assert A.max() < F.EXACT and A.max() <= taps * F.C * (2 * 3 + 2 * 3) + 5
    assert n.max() <= 2 * taps * F.C + 1
    assert np.array_equal(ref, np.round(ref))


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_emulated_decomposition_meets_both_criteria_and_one_wrong_term_misses_both(case):
    """fp32 emulation (F.emulate): bit equality under integer operands; err <= bound elementwise and relative L2 <= 2e-6 under
    normal ones.  The same emulation with one (tap, voxel) term dropped, and with one term read from the neighbouring cell,
    fails every one of the three."""
    geo = case["geom"]
    worst = {}
    for integer in (True, False):
        sw, W, bias = F.draw(case, integer)
        ref, n, A = F.reference(sw, geo, W, bias, bounds=True)
        variants = dict(clean=None, dropped=F.dropped_term(sw, geo), misplaced=F.misplaced_term(sw, geo))
        if sw.V == 0:
            assert variants["dropped"] is None and variants["misplaced"] is None
        else:
            assert variants["dropped"] is not None and variants["misplaced"] is not None, "no term to mutate"
        for kind, vox in variants.items():
            if kind != "clean" and vox is None:
                continue
            got = F.emulate(sw, geo, W, bias, voxel=vox)
            if integer:
                same = np.array_equal(got.astype(np.float64), ref)
                assert same == (kind == "clean"), f"{case['name']} integer, {kind}"
            else:
                ratio, l2 = F.criteria(got, ref, n, A)
                worst[kind] = (ratio, l2)
                if kind == "clean":
                    assert ratio <= 1.0 and l2 <= F.TOL_L2, f"{case['name']} {kind}: err/bound {ratio:.3e}, rel-L2 {l2:.3e}"
                else:
                    assert ratio > 1.0 and l2 > F.TOL_L2, f"{case['name']} {kind}: err/bound {ratio:.3e}, rel-L2 {l2:.3e}"
    print(case["name"], {k: f"err/bound {r:.3g}, rel-L2 {l:.3g}" for k, (r, l) in worst.items()})


@pytest.mark.parametrize("name", F.BACKWARD_CASES)
def test_backward_sums_of_integer_operands_stay_exact(name):
    """The sparse backward is compared bit for bit: every sum behind S, dW, the grid gradient and g_all stays below 2^24,
    and the dense definition agrees with the decomposition the layer computes (voxel rows + the constant's share)."""
    case = F.by_name(name)
    geo = case["geom"]
    sw, W, _ = F.draw(case, True)
    dy = F.draw_dy(case, geo)
    ref = F.backward_reference(sw, geo, W, dy)
    assert ref["largest"] < F.EXACT
    for k in ("S", "dW", "rows", "g_all"):
        assert np.array_equal(ref[k], np.round(ref[k]))
    assert ref["rows"].shape == (sw.V, F.C)
    # g_all and the constant's share of dW by their own formulas (tests/glue_ref.py)
    assert np.array_equal(R.const_field_g_all(W, ref["S"])[0], ref["g_all"])
    from oracle import conv_ref
    delta_grid = sw.grid - sw.c.astype(np.float64)
    sparse = conv_ref.conv_wgrad(delta_grid, dy, geo["outd"], geo["k"], geo["s"], geo["p"])
    assert np.array_equal(R.const_field_dw(sw.c, ref["S"], sparse), ref["dW"])
