"""Every case of tests/igemm_edge_cases.py engages the plan it is listed for (lisec_conv_plan_query answers on the host, 256 CUs
without a device), keeps the geometric corner it was written for (recomputed here from the dims, not from the planner), draws
inputs that meet the conditions the GPU test relies on, and between them the cases reach every launch form of csrc/igemm.hip
that REQUIRED names.  tests/test_gpu_igemm_edges.py runs the same table on the GPU; this file keeps the table honest."""
import numpy as np
import pytest

import igemm_edge_cases as E

IDS = [c["name"] for c in E.CASES]


def test_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", E.CASES, ids=IDS)
def test_case_engages_its_plan(case):
    with E.tuning(**case["knobs"]):
        plan = E.plan_of(case)
    got = {k: plan[k] for k in case["plan"]}
    assert got == case["plan"], f"{case['name']}: plan {got}, listed {case['plan']} ({plan})"


def test_knobs_are_restored():
    from lisec_amd import _lib
    before = _lib.get_tuning()
    for case in E.CASES:
        with E.tuning(**case["knobs"]):
            pass
    with pytest.raises(ZeroDivisionError):
        with E.tuning(lone_db=0, force_splitk=3, wide_tile=1, plane_pair=0):
            1 / 0
    assert _lib.get_tuning() == before


def test_the_table_reaches_every_required_form():
    reached = {}
    for case in E.CASES:
        with E.tuning(**case["knobs"]):
            reached.setdefault(E.form_of(E.plan_of(case)), case["name"])
    print("(kernel, cols, double_buffered, sliced, launches, plane_pair, parity_classes, tile_rows) reached:")
    for form in sorted(reached):
        print(f"  {form}: {reached[form]}")
    assert E.REQUIRED <= set(reached), f"not reached: {sorted(E.REQUIRED - set(reached))}"


def test_the_compared_forms_are_in_the_table():
    for a, b in E.IDENTICAL + E.REORDERED:
        ca, cb = E.by_name(a), E.by_name(b)
        assert (ca["mode"], ca["ind"], ca["outd"], ca["k"], ca["s"], ca["p"]) == (cb["mode"], cb["ind"], cb["outd"], cb["k"], cb["s"], cb["p"])
        with E.tuning(**ca["knobs"]):
            pa = E.plan_of(ca)
        with E.tuning(**cb["knobs"]):
            pb = E.plan_of(cb)
        assert E.form_of(pa) != E.form_of(pb), f"{a} and {b} run the same form"
    for a, b in E.IDENTICAL:                           # the same operands: everything but the name and the form switches agrees
        ca, cb = E.by_name(a), E.by_name(b)
        same = [k for k in ca if k not in ("name", "plan", "knobs", "flags", "queue", "facts", "like")]
        assert all(ca[k] == cb[k] for k in same), (a, b)
        assert E.operands_of(ca) == E.operands_of(cb)
    a, b = (E.by_name(n) for n in E.IDENTICAL[2])       # 64-row vs 128-row tiles: at EQUAL slicing
    assert a["plan"]["k_slices"] == b["plan"]["k_slices"] and a["plan"]["tile_rows"] == 64 and b["plan"]["tile_rows"] == 128


# ---- the corners, from the dims ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CASES, ids=IDS)
def test_case_keeps_its_corner(case):
    """The facts a case lists are what its dims give.  Beyond the listed ones: a tile of three lines only where the plan is the
    three-line halo kernel or the plain one; a dead second half or a ragged column block where half-N is listed with one; unequal
    depth taps wherever planes are paired."""
    facts = E.facts_of(case)
    for k, v in case["facts"].items():
        assert facts[k] == v, f"{case['name']}: {k} = {facts[k]}, listed {v}"
    kernel = case["plan"]["kernel"]
    if kernel in ("halo2", "wide") and case["plan"].get("tile_rows", 128) == 128:
        assert facts["max_lines"] <= 2, case["name"]
    if kernel in ("halo2", "halo3", "wide"):
        assert case["outd"][2] >= 64 and case["k"][2] == 3 and case["ind"][2] == case["outd"][2]
        assert (kernel == "halo3") == (case["outd"][2] < 126) or case["plan"].get("tile_rows") == 64
    if case["plan"].get("plane_pair"):
        assert len(set(facts["depth_taps"])) > 1 and case["outd"][0] % 2 == 0 and (case["outd"][1] * case["outd"][2]) % 128 == 0
    if case["plan"].get("parity_classes"):
        assert facts["class_rows"] == (case["outd"][1] // 2) * (case["outd"][2] // 2)
    if case["rows"]:
        assert 0 <= case["rows"][1] < case["rows"][0]


def test_the_corners_the_table_is_for():
    """One assertion per corner named in the table's reason for being: a later edit cannot lose one quietly."""
    F = {c["name"]: E.facts_of(c) for c in E.CASES}
    K = {c["name"]: c["plan"]["kernel"] for c in E.CASES}
    # two lines exactly at W = 126 and 127; three lines in one tile at the narrowest and the widest three-line width
    for w in (126, 127):
        assert F[f"halo W{w}"]["max_lines"] == 2 and F[f"halo W{w} sliced"]["max_lines"] == 2
    three = [n for n in F if F[n]["max_lines"] == 3 and K[n] == "halo3"]
    assert {"halo3 W65 three lines", "halo3 W125 three lines", "halo3 3D strided", "halo3 half-N dgrad"} <= set(three)
    # a last tile of one row (plain), of a few rows (halo2, half-N), ragged 64-row tiles
    assert F["plain M129"]["last_tile_rows"] == 1 and F["halo2 half-N KH1"]["last_tile_rows"] == 4
    assert F["halo W129"]["last_tile_rows"] == 3 and F["small tile halo"]["last_tile_rows_64"] == 18
    # tiles that span depth planes, on the plain and on the halo kernel
    assert F["plain 3D"]["crosses_depth"] and F["halo3 3D strided"]["crosses_depth"] and F["dead plane halo3"]["crosses_depth"]
    # parity classes: exactly one wave, a line wrap inside a wave (Wo / 2 = 33 > 32), a last tile of two rows
    assert F["parity one wave"]["class_rows"] == 32
    assert E.by_name("parity wrap")["outd"][2] // 2 == 33 and F["parity wrap"]["class_rows"] == 99
    assert F["parity 2 rows"]["class_last_tile_rows"] == 2 and F["parity 2 rows bwd sink"]["class_last_tile_rows"] == 2
    # plane pairs run planes of unequal tap counts; the dead-plane cases have a plane without any
    assert F["plane pairs halo3"]["depth_taps"] == [2, 3] and F["plane pairs transposed"]["depth_taps"] == [1, 2, 1, 1]
    for n in ("dead plane plain", "dead plane halo3", "dead plane halo3 sliced", "tail dead plane"):
        assert F[n]["depth_taps"] == [1, 1, 0]
    # column blocks with fewer than 64 / 32 live columns; a partial channel slab
    assert F["plain M129"]["last_block_cols"] == 1 and F["half-N 40"]["last_half_cols"] == 8 and F["half-N 16"]["last_block_cols"] == 16
    assert F["wide: bwd sink"]["last_block_cols"] == 8 and F["halo3 3D strided"]["last_block_cols"] == 8
    for n in ("plain M129", "halo3 3D strided", "wide W131 dgrad", "fold plain relu", "fold halo2 linear", "plane pairs halo3"):
        assert F[n]["partial_slab"] % 4 == 0 and 0 < F[n]["partial_slab"] < 64, n
    # row lists: no tile, one row, a second tile that starts AT the count, the last tile one row short; the queue likewise
    assert [F[f"rows count {n}"]["live_tiles"] for n in (0, 1, 128, 999)] == [0, 1, 1, 8]
    assert F["rows count 999"]["last_live_tile_rows"] == 103 and F["queue count 129"]["last_live_tile_rows"] == 1
    assert F[f"queue count {E.QUEUE_CAPACITY - 1}"]["last_live_tile_rows"] == 127
    # dense64: at its threshold, one tile short of it, and 769 tiles with a nearly empty last one for all five instantiations
    d64 = [c for c in E.CASES if c["name"].startswith("dense64 ") and c["ind"] == E.D64]
    assert len(d64) == 5 and all(E.facts_of(c)["last_tile_rows"] == 2 for c in d64) and int(np.prod(E.D64)) == 768 * 128 + 2
    assert {(bool(c["in_bn"]), c["stats"], c["dense_dw"]) for c in d64} == {
        (True, None, False), (False, None, False), (False, "bwd sink", False), (True, "bwd sink", False), (False, "bwd sink", True)}
    # every family has every epilogue switch
    for fam, spec in E.FAMILIES.items():
        mine = [c for c in E.CASES if c["name"].startswith(fam + ": ")]
        assert any(c["bias"] for c in mine) and any(c["accumulate"] for c in mine) and any(c["out_relu"] for c in mine)
        assert {c["stats"] for c in mine} >= {"sink", "bwd sink"}
        assert {c["bwd_relu"] for c in mine if c["stats"] == "bwd sink"} == {True, False}
        if spec[8]:
            assert any(c["gate"] for c in mine)
        if spec[7]:
            assert {c["stats"] for c in mine} >= {"table", "bwd table"}
    # BatchNormalization backward on load: the three tile kinds, with and without the ReLU gate, 72 channels on one
    folds = [c for c in E.CASES if c["fold"]]
    assert {c["plan"]["kernel"] for c in folds} == {"igemm", "halo2", "halo3"} and {c["fold"] for c in folds} == {"relu", "linear"}
    assert any(c["cin"] == 72 for c in folds)
    # a padded case with BatchNormalization + ReLU on load whose shifts are all positive
    assert any(c["in_bn"] == E.POS and c["in_relu"] and c["p"][2] == 1 for c in E.CASES)


# ---- the drawn inputs ----------------------------------------------------------------------------------------------------------------
def _big(c):
    return int(np.prod(c["outd"])) * c["cout"] > 4_000_000 or (c["rows"] and c["rows"][0] > 50_000)


@pytest.mark.parametrize("case", E.CASES, ids=IDS)
def test_drawn_inputs_meet_the_conditions(case):
    """No BatchNormalization gate argument within 1e-4 of zero (fp32 and fp64 agree on every gate); the output gates hold exact
    +0.0 and -0.0 next to positive and negative values; positive-shift cases draw every shift from (0.5, 1.5); the operands are
    float32 and the same on every draw."""
    c = case
    o = E.draw(c)
    for a in E.gate_arguments(c, o):
        assert np.abs(a).min() >= E.GATE_MARGIN, f"{c['name']}: a gate argument at {np.abs(a).min():.2e}"
    if c["bwd_relu"] or c["fold"] == "relu":
        assert E.gate_arguments(c, o), c["name"]
    if c["gate"]:
        gate = o["gate"]
        zeros = gate[gate == 0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any(), f"{c['name']}: the gate lacks a signed zero"
        assert (gate > 0).any() and (gate < 0).any()
    if c["in_bn"] == E.POS:
        shift = o["in_bn"][c["cin"]:2 * c["cin"]]
        assert shift.min() > 0.5 and shift.max() < 1.5 and c["in_relu"]
    assert all(v.dtype in (np.float32, np.int32) for v in o.values())
    if not _big(c):
        again = E.draw(c)
        assert all(np.array_equal(o[k], again[k]) for k in o)


# ---- the oracle at the two shapes no other test pins --------------------------------------------------------------------------------
def test_oracle_at_kernel_4_stride_4_transposed():
    """oracle/conv_ref.conv_forward in mode 1 at the exact shape of "k4 s4 transposed" against torch conv_transpose3d in fp64
    (tests/test_oracle_conv.py pins kernel == stride 4 on a 2 x 3 map)."""
    import torch
    import torch.nn.functional as F
    from oracle import conv_ref
    c = E.by_name("k4 s4 transposed")
    o = E.draw(c)
    x, W = o["x"].astype(np.float64), o["W"].astype(np.float64)
    got = conv_ref.conv_forward(x, W, c["outd"], c["k"], c["s"], c["p"], mode=1)
    wt = torch.from_numpy(W).reshape(*c["k"], c["cin"], c["cout"]).permute(3, 4, 0, 1, 2).contiguous()      # (in, out, kd, kh, kw)
    ref = F.conv_transpose3d(torch.from_numpy(x).permute(3, 0, 1, 2)[None], wt, stride=c["s"], padding=c["p"])[0]
    ref = ref.permute(1, 2, 3, 0).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12


def test_oracle_at_stride_2_2_2():
    """conv_ref.conv_forward in mode 0 at the exact shape of "plain 3D" (kernel 3, stride 2, pad 1 on all three axes) against
    torch conv3d in fp64."""
    import torch
    import torch.nn.functional as F
    from oracle import conv_ref
    c = E.by_name("plain 3D")
    o = E.draw(c)
    x, W, b = o["x"].astype(np.float64), o["W"].astype(np.float64), o["bias"].astype(np.float64)
    got = conv_ref.conv_forward(x, W, c["outd"], c["k"], c["s"], c["p"], mode=0, bias=b)
    wt = torch.from_numpy(W).reshape(*c["k"], c["cin"], c["cout"]).permute(4, 3, 0, 1, 2).contiguous()
    ref = F.conv3d(torch.from_numpy(x).permute(3, 0, 1, 2)[None], wt, torch.from_numpy(b), stride=c["s"], padding=c["p"])[0]
    ref = ref.permute(1, 2, 3, 0).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12
