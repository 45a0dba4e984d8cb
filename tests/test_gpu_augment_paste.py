"""Ground-truth object sampling on the GPU (csrc/augment.hip: lisec_augment_owner / _sample / _paste and the device-count
entries; lisec_amd/augment.py: ObjectDatabase, sample_objects, the database pipeline of AugmentedSweeps) against the numpy
oracle of tests/augment_paste_ref.py on the inputs of tests/augment_paste_cases.py, whose decisions
tests/test_augment_paste_oracle.py shows to be clear of rounding: every comparison below is over every row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_paste_cases as C
import augment_paste_ref as P
import augment_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    from lisec_amd import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_lib.require_gpu(), dtype=dtype)


def _bits(t):
    return t.cpu().numpy().view(np.uint8)


# ---- owner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.OWNER_CASES)
def test_owner_is_the_lowest_box_holding_the_point(name):
    from lisec_amd import augment, ops
    pts, boxes = C.owner_case(name)
    d_pts = _dev(pts)
    assert d_pts.shape[1] == (5 if name == "strided" else 3) and d_pts.cpu().numpy().dtype == pts.dtype
    got = ops.augment_owner(d_pts, _dev(boxes.reshape(-1, 7)), augment.PAD_LIMIT).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, P.owner(pts, boxes))


# ---- database -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DATABASE_CASES)
def test_database_equals_the_oracles(name):
    import torch
    from lisec_amd import augment
    pts, boxes = C.database_sweeps(name)
    want = C.database(name)
    db = augment.ObjectDatabase(pts, boxes, min_points=C.MIN_POINTS)
    assert len(db) == len(want["boxes"]) and db.dtype == (torch.float64 if name == "mixed" else torch.float32)
    assert db.points.dtype == db.dtype and db.offsets.dtype == torch.int32 and db.boxes.is_cuda and db.points.is_cuda
    assert np.array_equal(db.boxes.cpu().numpy(), want["boxes"]) and np.array_equal(db.counts.cpu().numpy(), want["counts"])
    assert np.array_equal(db.offsets.cpu().numpy(), want["offsets"]) and np.array_equal(db.points.cpu().numpy(), want["points"])
    assert [db.bound(k) for k in (0, 1, 3, 64)] == [P.bound(want, k) for k in (0, 1, 3, 64)]
    empty = augment.ObjectDatabase([], [])
    assert len(empty) == 0 and empty.bound(5) == 0 and empty.offsets.tolist() == [0]
    none_kept = augment.ObjectDatabase(pts[:1], boxes[:1], min_points=10 ** 6)
    assert len(none_kept) == 0 and tuple(none_kept.points.shape) == (0, 3)


# ---- sample ---------------------------------------------------------------------------------------------------------------
def _sample(scene, db, K, seed, item=3, epoch=1):
    from lisec_amd import ops
    index, n_boxes, boxes_all, point_offset, draws = ops.augment_sample(
        _dev(np.asarray(scene, dtype=np.float64).reshape(-1, 7)), _dev(db["boxes"].reshape(-1, 7)), _dev(db["offsets"]), K,
        seed, item, epoch)
    return dict(index=index, n_boxes=n_boxes, boxes_all=boxes_all, point_offset=point_offset, draws=draws)


def _check_sample(got, want):
    assert np.array_equal(got["index"].cpu().numpy(), want["index"])
    assert got["n_boxes"].cpu().numpy().tolist() == [want["n_boxes"]]
    assert np.array_equal(got["point_offset"].cpu().numpy(), want["point_offset"])
    assert np.array_equal(got["draws"].cpu().numpy().view(np.uint32), want["draws"])
    assert np.array_equal(got["boxes_all"].cpu().numpy(), want["boxes_all"])           # live rows exact, zero past them
    assert not got["boxes_all"].cpu().numpy()[want["n_boxes"]:].any()


@pytest.mark.parametrize("name", C.SAMPLE_CASES)
def test_sample_matches_the_oracle(name):
    scene, db, sample_to, seed = C.sample_case(name)
    K = P.sample_count(len(scene), sample_to)
    want, _ = C.sample_expected(name)
    got = _sample(scene, db, K, seed)
    _check_sample(got, want)
    if name == "chain":
        assert got["index"].cpu().numpy().tolist() == [-1, 1, -1]
    if name in ("crowded", "k64"):
        idx = got["index"].cpu().numpy()
        assert (idx >= 0).any() and (idx < 0).any()
    again = _sample(scene, db, K, seed)
    assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got)              # bit-identical rerun
    for other in (dict(epoch=2), dict(item=4)):
        item, epoch = other.get("item", 3), other.get("epoch", 1)
        d = _sample(scene, db, K, seed, item, epoch)
        _check_sample(d, C.sample_expected(name, item, epoch)[0])
        assert K == 0 or not np.array_equal(_bits(d["draws"]), _bits(got["draws"]))


def test_sample_capacity_is_refused_not_truncated():
    from lisec_amd import _lib
    db = C.database("f32")
    one = R.scene(np.random.default_rng(0), 1)
    got = _sample(np.tile(one, (448, 1)), db, 64, C.SEED)                               # B + K = 512
    n = int(got["n_boxes"].cpu().numpy()[0])
    idx = got["index"].cpu().numpy()
    assert 448 <= n <= 512 and n - 448 == (idx >= 0).sum() and tuple(got["boxes_all"].shape) == (512, 7)
    with pytest.raises(_lib.LisecError, match="LISEC_AUG_MAX_BOXES"):
        _sample(np.tile(one, (449, 1)), db, 64, C.SEED)
    with pytest.raises(_lib.LisecError, match="LISEC_AUG_MAX_SAMPLES"):
        _sample(one, db, 65, C.SEED)


# ---- paste ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PASTE_CASES)
def test_paste_equals_the_oracle_bit_for_bit(name):
    import torch
    from lisec_amd import augment, ops
    c = C.paste_case(name)
    s, db, B = c["sample"], c["db"], len(c["boxes"])
    pts = _dev(c["points"])
    out = torch.full((c["cap"], 3), 7.0, dtype=pts.dtype, device=pts.device)
    ops.augment_paste(pts, _dev(db["points"]), _dev(db["offsets"]), _dev(s["index"]), _dev(s["point_offset"]),
                      _dev(s["boxes_all"]), _dev(np.array([s["n_boxes"]], dtype=np.int32)), out, augment.PAD_LIMIT)
    got = out.cpu().numpy()
    assert got.dtype == c["want"].dtype and got.shape == c["want"].shape
    assert np.array_equal(got.view(np.uint8), c["want"].view(np.uint8))                 # every row, bit for bit
    n = len(c["points"])
    assert np.all(got[:n][c["removed"]] == 1.0e6) and (name == "n0" or c["removed"].sum() > 0)
    print(f"{name}: {int(c['removed'].sum())} scene rows removed, {int(s['point_offset'][-1])} pasted, cap {c['cap']}")
    if name == "big":
        assert (db["counts"][s["index"][s["index"] >= 0]] > 256).any()                  # an object that crosses workgroups
    if name == "f32":
        with pytest.raises(ValueError):
            ops.augment_paste(pts, _dev(db["points"].astype(np.float64)), _dev(db["offsets"]), _dev(s["index"]),
                              _dev(s["point_offset"]), _dev(s["boxes_all"]),
                              _dev(np.array([s["n_boxes"]], dtype=np.int32)), out, augment.PAD_LIMIT)


# ---- device-side counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 10])
def test_device_counts_equal_the_host_counts(n):
    """The _n entries on max_boxes = 10 rows with NaN past the device count against the existing entries on the first n."""
    import torch
    from lisec_amd import augment, boxes, ops
    rng = np.random.default_rng(77)
    rows = R.scene(rng, 10)
    junk = rows.copy()
    junk[n:] = np.nan
    pts = _dev(R.points_around(rng, rows, 3000).astype(np.float32))
    d_junk, d_rows, d_n = _dev(junk), _dev(rows[:n].reshape(-1, 7)), _dev(np.array([n], dtype=np.int32))
    p = augment._params({})
    want = ops.augment_draw(d_rows, p, C.SEED, 2, 1)
    got = ops.augment_draw(d_junk, p, C.SEED, 2, 1, n_boxes=d_n)
    for w, g, rows_of in zip(want, got, (n, None, n, n, 4 + 8 * n)):
        g_live = g if rows_of is None else g[:rows_of]
        assert np.array_equal(_bits(w), _bits(g_live))
        assert rows_of is None or not g[rows_of:].cpu().numpy().any()                   # nothing written past the count
    out_w = ops.augment_apply(pts, d_rows, want[0], want[1], torch.empty_like(pts), augment.PAD_LIMIT)
    out_g = ops.augment_apply(pts, d_junk, got[0], got[1], torch.empty_like(pts), augment.PAD_LIMIT, n_boxes=d_n)
    assert np.array_equal(_bits(out_w), _bits(out_g))
    moved = torch.nan_to_num(got[2], nan=0.0)
    moved[n:] = float("nan")
    for balance in (False, True):
        y_w = boxes.rpnTargets(want[2], seed=5, item=2, epoch=1, balance=balance)
        y_g = boxes.rpnTargets(moved, seed=5, item=2, epoch=1, balance=balance, n_boxes=d_n)
        assert np.array_equal(_bits(y_w[0]), _bits(y_g[0])) and np.array_equal(_bits(y_w[1]), _bits(y_g[1]))
        assert n == 0 or (y_w[0] == 2).sum() >= 1


# ---- the whole item -------------------------------------------------------------------------------------------------------
def _device_database():
    from lisec_amd import augment
    return augment.ObjectDatabase(*C.database_sweeps("f32"), min_points=C.MIN_POINTS)


def test_sample_objects_is_sample_then_paste():
    from lisec_amd import augment
    pts, scene, db = C.item_case()
    K = P.sample_count(len(scene), C.ITEM_SAMPLE_TO)
    item, epoch = C.ITEM_AT
    want = P.sample(scene, db, K, C.SEED, item, epoch)
    want_p, _ = P.paste(pts, db, want, len(scene))
    got_p, boxes_all, n_boxes, index = augment.sample_objects(pts, scene, _device_database(), C.ITEM_SAMPLE_TO, C.SEED, item,
                                                                epoch)
    assert tuple(got_p.shape) == (len(pts) + P.bound(db, K), 3) and tuple(boxes_all.shape) == (len(scene) + K, 7)
    assert np.array_equal(got_p.cpu().numpy().view(np.uint8), want_p.view(np.uint8))
    assert np.array_equal(boxes_all.cpu().numpy(), want["boxes_all"]) and n_boxes.tolist() == [want["n_boxes"]]
    assert np.array_equal(index.cpu().numpy(), want["index"])
    with pytest.raises(ValueError):
        augment.sample_objects(pts, np.tile(scene[:1], (449, 1)), _device_database(), 1000, C.SEED)


def test_augment_sweep_with_a_database_is_the_oracles_pipeline():
    from lisec_amd import augment, boxes
    pts, scene, _ = C.item_case()
    item, epoch = C.ITEM_AT
    want_p, want_b, smp, _ = C.item_expected()
    got_p, got_b, n_boxes = augment.augment_sweep(pts, scene, C.SEED, item=item, epoch=epoch, database=_device_database(),
                                                  sample_to=C.ITEM_SAMPLE_TO)
    nb = smp["n_boxes"]
    assert n_boxes.tolist() == [nb] and nb > len(scene) and got_p.cpu().numpy().dtype == np.float32
    assert tuple(got_p.shape) == want_p.shape and tuple(got_b.shape) == (len(smp["boxes_all"]), 7)
    err_b = np.abs(got_b.cpu().numpy()[:nb] - want_b).max()
    err_p = np.abs(got_p.cpu().numpy() - want_p).max()
    print(f"boxes max error {err_b:.3e}, points max error {err_p:.3e}")
    assert err_b <= 1e-12 and not got_b.cpu().numpy()[nb:].any()
    assert err_p <= 1e-5                                                                # float32 points, every row
    pad = np.abs(want_p[:, 0]) >= R.PAD_LIMIT
    assert pad.any() and np.all(got_p.cpu().numpy()[pad] == 1.0e6)
    y = boxes.rpnTargets(got_b, seed=C.SEED, item=item, epoch=epoch, n_boxes=n_boxes)
    y_w = boxes.rpnTargets(want_b, seed=C.SEED, item=item, epoch=epoch)
    assert np.array_equal(y[0].cpu().numpy(), y_w[0].cpu().numpy()) and np.array_equal(y[1].cpu().numpy(), y_w[1].cpu().numpy())


@pytest.mark.parametrize("augment_on", [True, False])
def test_augmented_sweeps_item_with_a_database(augment_on):
    from lisec_amd import augment, boxes
    pts, scene, db = C.item_case()
    other = C.database_sweeps("f32")
    seq = augment.AugmentedSweeps([other[0][1], pts], [other[1][1], scene], seed=C.SEED, augment=augment_on,
                                  database=_device_database(), sample_to=C.ITEM_SAMPLE_TO)
    item, epoch = C.ITEM_AT
    assert item == 1
    for _ in range(epoch):
        seq.on_epoch_end()
    K = P.sample_count(len(scene), C.ITEM_SAMPLE_TO)
    assert seq.rows(1) == len(pts) + P.bound(db, K) and seq.max_points == max(seq.rows(0), seq.rows(1))
    got_p, (y_cls, y_reg) = seq[1]
    if augment_on:
        want_p, want_b, smp, _ = C.item_expected()
    else:
        smp = P.sample(scene, db, K, C.SEED, item, epoch)
        want_p, want_b = P.paste(pts, db, smp, len(scene))[0].astype(np.float64), smp["boxes_all"][:smp["n_boxes"]]
    assert tuple(got_p.shape) == want_p.shape == (seq.rows(1), 3)                       # pad rows included
    assert np.abs(got_p.cpu().numpy() - want_p).max() <= (1e-5 if augment_on else 0.0)
    y_w = boxes.rpnTargets(want_b, seed=C.SEED, item=item, epoch=epoch)
    assert np.array_equal(y_cls.cpu().numpy(), y_w[0].cpu().numpy()) and np.array_equal(y_reg.cpu().numpy(), y_w[1].cpu().numpy())
    assert (y_cls == 2).sum() >= 1


# ---- Model.fit ------------------------------------------------------------------------------------------------------------
_FIT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import augment_cases as C0
import augment_paste_cases as C
import augment_paste_ref as P
from lisec_amd import Constants, _lib, augment
from lisec_amd import model_training as mt
Constants.nx, Constants.ny = 16, 32                 # the label maps of the (16, 32, 8) grid: 8 x 16 cells
assert (_lib.knob("step_plan", True)) == (sys.argv[2] == "plan")
pts, bxs = C0.fit_sweeps()
want_db = P.build_database(pts, bxs)


def model():
    np.random.seed(0)
    torch.manual_seed(0)
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    return m


class Logged(augment.AugmentedSweeps):
    def stage(self, i, points, y_cls, y_reg):
        n = super().stage(i, points, y_cls, y_reg)
        self.log.setdefault((self.epoch, i), points[:n].clone())
        return n


def run(database):
    m = model()
    s = Logged(pts, bxs, seed=C.FIT_SEED, database=database, sample_to=C.FIT_SAMPLE_TO)
    s.log = {}
    h = m.fit(x=s, batch_size=1, verbose=0, epochs=2, shuffle=False)
    torch.cuda.synchronize()
    assert (m._captured is not None) == (sys.argv[2] == "plan")
    return h.history, m.net.params.theta.cpu().numpy().copy(), s, m


db = augment.ObjectDatabase(pts, bxs)
assert len(db) == len(want_db["boxes"]) >= 6
h1, t1, s1, m1 = run(db)
h2, t2, s2, _ = run(db)
h0, t0, s0, _ = run(None)
assert np.array_equal(t1, t2) and h1 == h2                                   # two runs from one seed: bit-equal variables
assert not np.array_equal(t1, t0)                                            # and other than without the database
assert sorted(h1) == sorted(h0) == ['ClassificationLayer_loss', 'RegressionLayer_loss', 'loss'] and len(h1['loss']) == 2
assert sorted(s1.log) == [(e, i) for e in range(2) for i in range(3)]
bounds = [P.bound(want_db, P.sample_count(len(b), C.FIT_SAMPLE_TO)) for b in bxs]
assert s1.max_points == max(len(p) + b for p, b in zip(pts, bounds)) > s0.max_points
if sys.argv[2] == "plan":
    assert m1._captured[1].capacity >= s1.max_points                         # the plan's capacity covers n + bound
accepted = 0
for i in range(3):
    want, _, smp, _ = P.item(pts[i], bxs[i], want_db, C.FIT_SAMPLE_TO, C.FIT_SEED, i, 1)
    accepted += smp["n_boxes"] - len(bxs[i])
    got = s1.log[(1, i)].cpu().numpy()
    assert got.shape == want.shape == (len(pts[i]) + bounds[i], 3)
    assert np.abs(got - want).max() <= 1e-5, (i, np.abs(got - want).max())
assert accepted > 0
print("FIT-OK")
"""


@pytest.mark.parametrize("path", ["plan", "eager"])
def test_fit_on_sampled_sweeps(tmp_path, path):
    """fit(x=AugmentedSweeps(database=...)) on the recorded plan and on the Python schedule: reproducible from the seed,
    other than without the database, the staged points the oracle's, the plan's capacity n + bound, the History keys as
    they were.  A child process: the schedule is chosen by LISEC_TUNING at start-up."""
    script = tmp_path / "fit_sampled.py"
    script.write_text(_FIT)
    env = dict(os.environ, LISEC_TUNING="step_plan=%d" % (path == "plan"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), path], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FIT-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
