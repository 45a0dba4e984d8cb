"""Every case of tests/wgrad_edge_cases.py engages the plan it is listed for (lisec_conv_wgrad_plan_query answers on the
host, 256 CUs without a device), and between them the cases reach every contraction kernel variant and every reduce form of
csrc/wgrad.hip.  tests/test_gpu_wgrad_edges.py runs the same table on the GPU; this file keeps the table honest."""
import pytest

import wgrad_edge_cases as E


def _check(plan, expect, name):
    got = {k: plan[k] for k in expect}
    assert got == expect, f"{name}: plan {got}, listed {expect} ({plan})"


@pytest.mark.parametrize("case", E.CASES, ids=[c["name"] for c in E.CASES])
def test_case_engages_its_plan(case):
    with E.tuning(**case["knobs"]):
        plan = E.plan_of(case)
    _check(plan, case["plan"], case["name"])


def test_knobs_are_restored():
    from lisec_amd import _lib
    before = _lib.get_tuning()
    for case in E.CASES:
        with E.tuning(**case["knobs"]):
            pass
    with pytest.raises(ZeroDivisionError):
        with E.tuning(wgrad_ring=0):
            1 / 0
    assert _lib.get_tuning() == before


def test_the_table_reaches_every_kernel_variant_and_reduce_form():
    reached = set()
    for case in E.CASES:
        with E.tuning(**case["knobs"]):
            reached.add(E.kernel_and_reduce(E.plan_of(case)))
    kernels, reduces = {k for k, _ in reached}, {r for _, r in reached}
    listing = sorted((kind, np_, r) for (kind, np_), r in reached)
    print("(kind, staging passes, reduce) reached:", listing)
    assert E.REQUIRED_KERNELS <= kernels, f"not reached: {sorted(E.REQUIRED_KERNELS - kernels)} of {listing}"
    assert E.REQUIRED_REDUCES <= reduces, f"not reached: {sorted(E.REQUIRED_REDUCES - reduces)} of {listing}"
    # the slab sums over taps that no workgroup ran, the slab sum behind a w-halo plan, the ring's own
    for triple in [("halo", 7, "SLAB_SUM"), ("halo", 7, "LANE_SUM"), ("ring", 3, "RING_SUM"), ("plain", 8, "LANE_SUM"),
                   ("plain", 8, "SLAB_SUM"), ("halo", 9, "in-kernel"), ("ring", 6, "in-kernel")]:
        assert triple in listing, f"{triple} not among {listing}"


def test_ring_runs_are_uneven_where_listed():
    """R6: 7 lines in 3 runs -- the run bounds run * Ho / R give 2, 2 and 3 lines, not three times Ho / R."""
    c = E.by_name("R6")
    with E.tuning(**c["knobs"]):
        plan = E.plan_of(c)
    Ho, R = c["outd"][1], plan["runs_per_column"]
    assert [(r + 1) * Ho // R - r * Ho // R for r in range(R)] == [2, 2, 3] and Ho % R != 0


def test_the_seven_pass_halo_variant_covers_its_image():
    """NP = 7 stages 112 rows of the A image, which has DR + 2 rows (DR = tile rows rounded up to 8): every width whose
    tiles have 105 .. 110 rows needs the nine-pass variant, 104 rows (DR 104) still take seven."""
    from lisec_amd import ops
    for wo in list(range(96, 129)) + [208, 209, 220, 221, 330, 440]:
        g = ops.geom(0, (1, 2, wo), (1, 2, wo), E.K113, E.S1, (0, 0, 1), 64, 64)
        plan = ops.wgrad_plan(g)
        assert plan["halo"] == 1, plan
        dr = (plan["tile_rows"] + 7) // 8 * 8
        assert plan["staging_passes"] == (7 if dr + 2 <= 7 * 16 else 9), (wo, plan)
        assert plan["staging_passes"] * 16 >= dr + 2, (wo, plan)


@pytest.mark.parametrize("batch", E.BATCHES, ids=[b[0] for b in E.BATCHES])
def test_batch_items_engage_their_plans(batch):
    """The items' own plans; B3's items differ in staging passes, so the batch runs them one by one and its workspace is
    the largest single one."""
    import torch
    from lisec_amd import ops
    name, items, knobs, expect = batch
    with E.tuning(**knobs):
        plans = [E.plan_of(c) for c in items]
        for c, plan in zip(items, plans):
            _check(plan, expect, name)
        dummy = torch.zeros(4)
        b = ops.WgradBatch([(E.geom_of(c), dummy, dummy, dummy, dummy if c.get("in_bn") else None, E.flags_of(c),
                             bool(c.get("transpose_out"))) for c in items])
        total = b.workspace_bytes()
        singles = [ops.wgrad_workspace_bytes(E.geom_of(c)) for c in items]
    assert total > 0
    if name == "B3":
        assert len({p["staging_passes"] for p in plans}) == 2
        assert total == max(singles)
    else:
        assert len({p["staging_passes"] for p in plans}) == 1
