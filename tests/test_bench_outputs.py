"""bench.py --dump-outputs / --steps: what the timed path computed in its last step, written for comparison between builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, *argv], env=e, capture_output=True, text=True, timeout=900)


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    import bench
    arrays = {"loss": np.arange(3, dtype=np.float32), "theta": np.linspace(0, 1, 7)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "theta.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == a.dtype and np.array_equal(got, a)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_bench_refuses_a_timed_region_without_steps(argv):
    r = _bench(*argv, env=dict(LISEC_BENCH_DRYRUN="1"))
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_reproducibly(tmp_path):
    """--steps K times K steps, ms_per_step is their mean, and the dump holds the loss the result line reports and the
    variables after that step: bit-identical from run to run with the same arguments (seeded inputs and variables)."""
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = _bench("--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(out))
        assert r.returncode == 0, r.stderr[-3000:]
        j = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][0]
        assert j["steps"] == 3 and j["ms_per_step"] > 0
        assert abs(j["value"] - 3 / (j["ms_per_step"] * 3e-3)) < 1e-6 * j["value"]
        assert sorted(os.listdir(out)) == ["loss.npy", "state.npy", "theta.npy", "velocity.npy"]
        d = {n: np.load(out / f"{n}.npy") for n in ("loss", "state", "theta", "velocity")}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
        assert sum(a.nbytes for a in d.values()) <= 64 * 1000 * 1000
        assert d["loss"].shape == (3,) and float(d["loss"][0]) == j["config"]["final_loss"]
        assert d["theta"].shape == d["velocity"].shape and np.abs(d["velocity"]).max() > 0
        dumps.append(d)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n


@pytest.mark.gpu
def test_bench_full_adds_the_side_measurements():
    """A plain run prints the headline line with the side measurements null; --full times the same steps and then adds
    them (rank 0): the rooflines, the voxeliser alone, the R200k and other-loss steps."""
    lines = {}
    for mode, extra in (("plain", ()), ("full", ("--full", "--no-cpu-baseline"))):
        r = _bench("--steps", "3", "--warmup", "1", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(got) == 1
        lines[mode] = got[0]
    p, f = lines["plain"], lines["full"]
    for j in (p, f):
        assert j["metric"] == "lyft_samples_per_sec_fwd_bwd" and j["unit"] == "samples/s" and j["dtype"] == "f32"
        assert j["higher_is_better"] is True and j["steps"] == 3 and j["ms_per_step"] > 0
    assert all(p[k] is None for k in ("roofline", "roofline_vfe", "voxelizer", "r200k", "cpu_baseline"))
    assert "smoothl1_ce" not in p
    assert p["config"]["final_loss"] == f["config"]["final_loss"] and p["config"]["voxels"] == f["config"]["voxels"]
    assert f["roofline"]["us_per_launch"] > 0 and f["roofline"]["others"]["mid1_dense_form"]["us_per_launch"] > 0
    assert f["roofline_vfe"]["us_per_launch"] > 0
    assert f["voxelizer"]["u20k"]["voxels"] == f["config"]["voxels"] and "cpu_restatement" not in f["voxelizer"]
    assert f["r200k"]["value"] > 0 and f["r200k"]["points"] == 200000
    assert f["smoothl1_ce"]["loss"] == "smoothl1_ce" and f["smoothl1_ce"]["value"] > 0
    assert f["cpu_baseline"] is None
