"""The C-ABI library loads here (no GPU) and exports every symbol include/lisec_hip.h declares."""
import os
import re

from conftest import ROOT


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "lisec_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(lisec_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    from lisec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = _lib.load()
    names = _declared_functions()
    assert len(names) >= 5
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.lisec_abi_version() >= 1


def test_every_exported_lisec_symbol_is_declared():
    """exported <= declared: nothing the library exports under the lisec_ prefix is missing from the header (round 2's
    undeclared lisec_debug_* entry points)."""
    import subprocess
    from lisec_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("lisec_")})
    declared = set(_declared_functions())
    assert exported and not [n for n in exported if n not in declared]


def test_library_reads_no_environment_variables():
    """Launch plans are tuned through the lisec_tuning record of the ABI, never through getenv inside the library."""
    csrc = os.path.join(ROOT, "lisec_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_tuning_record_round_trip():
    from lisec_amd import _lib
    before = _lib.get_tuning()
    assert before["max_splitk"] == 12 and before["wgrad_blocks"] >= 1
    prev = _lib.set_tuning(max_splitk=8)
    try:
        assert _lib.get_tuning()["max_splitk"] == 8 and prev == {"max_splitk": 12}
    finally:
        _lib.set_tuning(**prev)
    import pytest
    with pytest.raises(KeyError):
        _lib.set_tuning(no_such_knob=1)


def test_plan_query_needs_no_gpu():
    """lisec_conv_plan_query answers on the host: the RPN block-2 layers are K-sliced, the mid2 data gradient pairs planes."""
    from lisec_amd import ops
    g = ops.geom(0, (1, 50, 100), (1, 50, 100), (1, 3, 3), (1, 1, 1), (0, 1, 1), 128, 128)
    plan = ops.conv_plan(g, in_bn=True, flags=ops.IN_RELU)
    assert plan["kernel"] == "halo3" and plan["k_slices"] >= 2 and plan["tail_tile0"] == 0 and plan["launches"] == 1
    g = ops.geom(1, (2, 200, 400), (4, 200, 400), (3, 3, 3), (1, 1, 1), (0, 1, 1), 64, 64)
    plan = ops.conv_plan(g)
    assert plan["kernel"] == "halo2" and plan["plane_pair"] == 1 and plan["k_slices"] == 1 and plan["workgroups"] == 1250


def test_wgrad_plan_query_needs_no_gpu():
    """lisec_conv_wgrad_plan_query answers on the host from the plan a call runs (256 CUs without a device): the second
    middle block and the stride-1 layer of RPN block 3 take the ring kernel, the strided first RPN layer the plain one."""
    from lisec_amd import ops

    def check(plan, **expect):
        assert {k: plan[k] for k in expect} == expect, plan

    g = ops.geom(0, (4, 200, 400), (2, 200, 400), (3, 3, 3), (1, 1, 1), (0, 1, 1), 64, 64)                  # mid2
    check(ops.wgrad_plan(g), ring=1, halo=0, mirrored=0, groups=6, tile_rows=100, staging_passes=5, taps_per_group=9,
          lane_reduce=1, combine_in_kernel=0, runs_per_column=10, lines_per_run=20, slabs=80, workgroups=240)
    g = ops.geom(0, (1, 25, 50), (1, 25, 50), (1, 3, 3), (1, 1, 1), (0, 1, 1), 256, 256)                    # rpn3.conv1
    check(ops.wgrad_plan(g, flags=ops.IN_RELU), ring=1, halo=0, groups=1, tile_rows=50, staging_passes=3, lane_reduce=0,
          combine_in_kernel=1, runs_per_column=13, workgroups=208)
    g = ops.geom(0, (1, 200, 400), (1, 100, 200), (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 128)                 # rpn1.conv0
    check(ops.wgrad_plan(g), ring=0, halo=0, mirrored=0, taps_per_group=3, groups=3, tile_rows=128, staging_passes=8,
          tiles=157, slabs=157, tiles_per_slab=1, workgroups=942, lane_reduce=1, combine_in_kernel=0)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from lisec_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    import pytest
    with pytest.raises(_lib.LisecError):
        _lib.load()


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under lisec_amd/ may import it."""
    pkg = os.path.join(ROOT, "lisec_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def test_tuning_spec_accepts_host_knobs_and_record_fields(monkeypatch):
    from lisec_amd import _lib
    monkeypatch.setenv("LISEC_TUNING", "winograd=7, max_splitk=8,step_plan=0")
    assert _lib._tuning_spec() == {"winograd": "7", "max_splitk": "8", "step_plan": "0"}
    assert _lib.knob("winograd", 15) == 7 and _lib.knob("step_plan", True) is False and _lib.knob("field_conv", True)


def test_load_rejects_an_unknown_tuning_knob():
    """A LISEC_TUNING key that is neither a host knob nor a lisec_tuning field -- here a schedule knob that was retired --
    is an error at load(), not a run that silently measures the default."""
    import subprocess
    import sys
    env = dict(os.environ, LISEC_TUNING="max_splitk=8,chain_first=0")
    r = subprocess.run([sys.executable, "-c", "from lisec_amd import _lib; _lib.load()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "LisecError" in r.stderr and "unknown knob(s) chain_first:" in r.stderr, r.stderr[-2000:]
