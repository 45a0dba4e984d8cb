"""Training-time augmentation on the GPU (csrc/augment.hip, lisec_amd/augment.py) against the numpy oracle of
tests/augment_ref.py on the inputs of tests/augment_cases.py, and Model.fit on a Sequence of augmented sweeps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_cases as C
import augment_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    from lisec_amd import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_lib.require_gpu(), dtype=dtype)


# ---- apply, transforms given ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.APPLY_CASES)
def test_apply_moves_points_with_their_boxes(name):
    import torch
    from lisec_amd import augment, ops
    c = C.apply_case(name)
    want = C.apply_expected(name)
    pts = _dev(c["points"])
    assert pts.shape[1] == (5 if name == "strided" else 3)
    boxes, tr = _dev(c["boxes"].reshape(-1, 7)), _dev(c["transforms"].reshape(-1, 4))
    glob = _dev(np.array([c["scale"], c["alpha"]]))
    out = torch.full((pts.shape[0], 3), 7.0, dtype=pts.dtype, device=pts.device)
    ops.augment_apply(pts, boxes, tr, glob, out, augment.PAD_LIMIT)
    got = out.cpu().numpy()
    assert got.shape == want.shape and got.dtype == c["points"].dtype      # the point count and dtype are the input's
    if len(want) == 0:
        return
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{name}: max |got - oracle| = {err:.3e} m")
    if got.dtype == np.float64:
        assert err <= 1e-12
    else:
        w32 = want.astype(np.float32)
        assert np.all(np.abs(got - w32) <= np.spacing(np.abs(w32)))         # 1 ulp of float32(oracle)
    pad = ~(np.abs(c["points"][:, 0]) < R.PAD_LIMIT)
    assert np.array_equal(got[pad], c["points"][pad, :3])                   # pad rows bit for bit
    if name == "pad":
        assert pad.sum() == 300 and np.abs(got[pad, 0]).min() == 1.0e6
    moved = np.abs(want - c["points"][:, :3]).max(1) > 1e-3
    assert moved[~pad].mean() > 0.99                                        # the global transform reaches the live points


# ---- draw -----------------------------------------------------------------------------------------------------------------
def _draw(boxes, item=3, epoch=1, seed=C.DRAW_SEED, **params):
    from lisec_amd import augment, ops
    t, g, b, a, w = ops.augment_draw(_dev(np.asarray(boxes, dtype=np.float64).reshape(-1, 7)), augment._params(params), seed,
                                     item, epoch)
    return dict(transforms=t.cpu().numpy(), glob=g.cpu().numpy(), boxes=b.cpu().numpy(), attempt=a.cpu().numpy(),
                draws=w.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", C.DRAW_CASES)
def test_draw_matches_the_oracle(name):
    boxes, params = C.draw_case(name), C.DRAW_PARAMS.get(name, {})
    want, _ = C.draw_expected(name)
    got = _draw(boxes, **params)
    assert np.array_equal(got["attempt"], want["attempt"])                  # the same candidate accepted, box by box
    assert np.array_equal(got["draws"], want["draws"])                      # and the same integer draws behind it
    for key, w in (("transforms", want["transforms"]), ("boxes", want["boxes"]),
                   ("glob", np.array([want["scale"], want["alpha"]]))):
        err = np.abs(got[key] - w).max() if w.size else 0.0
        print(f"{name}: {key} max error {err:.3e}")
        assert err <= 1e-12
    if name == "crowded":
        assert (got["attempt"] < 0).any() and (got["attempt"] >= 0).any()
    again = _draw(boxes, **params)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)       # bit-identical rerun
    for other in (dict(epoch=2), dict(item=4)):
        d = _draw(boxes, **dict(params, **other))
        w, _ = C.draw_expected(name, other.get("item", 3), other.get("epoch", 1))
        assert not np.array_equal(d["glob"], got["glob"]) and np.array_equal(d["attempt"], w["attempt"])
        assert np.array_equal(d["draws"], w["draws"]) and (len(boxes) == 0 or not np.array_equal(d["boxes"], got["boxes"]))


def test_draw_identity_and_capacity():
    from lisec_amd import _lib
    boxes = C.draw_case("b7")
    for params in (R.IDENTITY, dict(R.IDENTITY, attempts=10)):
        d = _draw(boxes, **params)
        assert np.array_equal(d["boxes"], boxes) and d["glob"].tolist() == [1.0, 0.0] and not d["transforms"].any()
    rng = np.random.default_rng(0)
    with pytest.raises(_lib.LisecError, match="LISEC_AUG_MAX_BOXES"):       # refused, not truncated
        _draw(np.tile(R.scene(rng, 1), (513, 1)))
    with pytest.raises(_lib.LisecError, match="attempts"):
        _draw(boxes, attempts=33)
    assert len(_draw(np.tile(R.scene(rng, 1), (512, 1)), attempts=1)["attempt"]) == 512


def test_augment_sweep_is_draw_then_apply():
    from lisec_amd import augment
    c = C.apply_case("f32")
    boxes = C.draw_case("b7")
    pts, bx = augment.augment_sweep(c["points"], boxes, C.DRAW_SEED, item=3, epoch=1)
    want_p, want_b = R.augment(c["points"].astype(np.float64), boxes, C.DRAW_SEED, 3, 1)
    assert pts.dtype.is_floating_point and pts.cpu().numpy().dtype == np.float32 and pts.is_cuda and bx.is_cuda
    assert np.abs(bx.cpu().numpy() - want_b).max() <= 1e-12
    # the oracle's owner test runs on its own transforms; a point is judged against the ORIGINAL boxes in both
    assert np.abs(pts.cpu().numpy() - want_p).max() <= 1e-5


# ---- label maps -----------------------------------------------------------------------------------------------------------
def _label_sets():
    g = np.load(os.path.join(GOLDEN, "box_fixscaling.npz"))
    rng = np.random.default_rng(5)
    return {"golden_data": g["data"], "golden_fixed": g["fixed"], "empty": np.zeros((0, 7)), "scene": R.scene(rng, 40, 44.0, 8.5)}


@pytest.mark.parametrize("name", ["golden_data", "golden_fixed", "empty", "scene"])
def test_rpn_targets_unbalanced_equal_preprocessLabels(name):
    import torch
    from lisec_amd import boxes
    data = _label_sets()[name]
    cls_r, reg_r = (a.astype(np.float32) for a in boxes.preprocessLabels(data, balance=False))
    y_cls, y_reg = boxes.rpnTargets(data, balance=False)
    assert y_cls.dtype == torch.float32 and y_cls.is_cuda and tuple(y_cls.shape) == (100, 200, 2) and tuple(y_reg.shape) == (100, 200, 14)
    assert np.array_equal(y_cls.cpu().numpy(), cls_r)
    assert np.array_equal(y_reg.cpu().numpy(), reg_r, equal_nan=True)       # (the golden rows have negative extents: NaN logs)
    # out=: the caller's buffers are written, device rows are accepted
    out = [torch.full_like(y_cls, 9.0), torch.full_like(y_reg, 9.0)]
    back = boxes.rpnTargets(_dev(data.reshape(-1, 7)), balance=False, out=out)
    assert back[0] is out[0] and torch.equal(out[0], y_cls) and np.array_equal(out[1].cpu().numpy(), reg_r, equal_nan=True)
    if name == "scene":
        assert (cls_r == 2).sum() >= 40


@pytest.mark.parametrize("max_regions", [256, 16])
def test_rpn_targets_balanced_keep_the_oracles_set(monkeypatch, max_regions):
    from lisec_amd import Constants, boxes
    monkeypatch.setattr(Constants, "maxRegions", max_regions)
    data = _label_sets()["scene"]
    cls0, reg0 = (a.cpu().numpy() for a in boxes.rpnTargets(data, balance=False))
    overlap, valid = (cls0 == 2).astype(np.float64), (cls0 >= 1).astype(np.float64)
    n_pos, n_neg = int(overlap.sum()), int((cls0 == 1).sum())
    assert n_neg > max_regions and (max_regions == 256 or n_pos > max_regions // 2)
    seen = []
    for seed, item, epoch in ((0, 0, 0), (9, 2, 1), (9, 2, 2)):
        y_cls, y_reg = (a.cpu().numpy() for a in boxes.rpnTargets(data, seed=seed, item=item, epoch=epoch))
        want = R.balance_keep(valid, overlap, max_regions, seed, item, epoch)
        assert np.array_equal(y_cls, (want + overlap).astype(np.float32))   # the kept set is the oracle's, exactly
        assert np.array_equal(y_reg, reg0)
        kept_pos = int(((want == 1) & (overlap == 1)).sum())
        kept_neg = int(((want == 1) & (overlap == 0)).sum())
        got_valid = np.where(overlap == 1, (y_cls == 2), (y_cls == 1))      # a dropped positive keeps overlap: 1, not 2
        assert int((got_valid & (overlap == 1)).sum()) == kept_pos == min(n_pos, max_regions // 2)
        assert int((got_valid & (overlap == 0)).sum()) == kept_neg == kept_pos            # negatives are plentiful
        assert kept_pos + kept_neg <= max_regions
        seen.append(y_cls)
    assert not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[1])
    # no boxes: no positives, so the reference's rule keeps no negatives either
    assert not boxes.rpnTargets(np.zeros((0, 7)))[0].any()


# ---- Model.fit on a Sequence ----------------------------------------------------------------------------------------------
_FIT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import augment_cases as C
import augment_ref as R
from lisec_amd import Constants, _lib, augment, boxes
from lisec_amd import model_training as mt
Constants.nx, Constants.ny = 16, 32                 # the label maps of the (16, 32, 8) grid: 8 x 16 cells
assert (_lib.knob("step_plan", True)) == (sys.argv[2] == "plan")
pts, bxs = C.fit_sweeps()
SMALL = (0.5, 0.25, 0.25, 35, 8, 16, 8)


def model():
    np.random.seed(0)
    torch.manual_seed(0)
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    return m


def run(m, **kw):
    h = m.fit(batch_size=1, verbose=0, epochs=2, shuffle=False, **kw)
    torch.cuda.synchronize()
    assert (m._captured is not None) == (sys.argv[2] == "plan")
    return h.history, m.net.params.theta.cpu().numpy().copy()


labels = [[a.astype(np.float32) for a in boxes.preprocessLabels(b, balance=False)] for b in bxs]
y = [np.stack([l[0] for l in labels]), np.stack([l[1] for l in labels])]
assert y[0].shape == (3, 8, 16, 2) and (y[0] == 2).sum() >= 3
h_list, t_list = run(model(), x=[mt.VFE_preprocessing(p, *SMALL) for p in pts], y=y)
seq = augment.AugmentedSweeps(pts, bxs, seed=4, balance=False, **augment.IDENTITY)
h_seq, t_seq = run(model(), x=seq)
assert seq.epoch == 2 and len(seq) == 3
assert h_list == h_seq and sorted(h_seq) == ['ClassificationLayer_loss', 'RegressionLayer_loss', 'loss'], (h_list, h_seq)
assert len(h_seq['loss']) == 2 and np.array_equal(t_list, t_seq)
plain = augment.AugmentedSweeps(pts, bxs, seed=4, augment=False, balance=False)
p0, (c0, r0) = plain[1]
assert torch.equal(p0, torch.from_numpy(pts[1]).to(p0.device)) and np.array_equal(c0.cpu().numpy(), labels[1][0])
if sys.argv[2] == "plan":
    class Logged(augment.AugmentedSweeps):
        def stage(self, i, points, y_cls, y_reg):
            n = super().stage(i, points, y_cls, y_reg)
            self.log.setdefault((self.epoch, i), points[:n].clone())
            return n
    thetas = []
    for _ in range(2):
        s = Logged(pts, bxs, seed=11)
        s.log = {}
        _, t = run(model(), x=s)
        thetas.append(t)
    assert np.array_equal(thetas[0], thetas[1]) and not np.array_equal(thetas[0], t_seq)
    assert sorted(s.log) == [(e, i) for e in range(2) for i in range(3)]
    for i in range(3):
        assert not torch.equal(s.log[(0, i)], s.log[(1, i)])                 # another epoch, other points
        want, _ = R.augment(pts[i].astype(np.float64), bxs[i], 11, i, 1)
        assert np.abs(s.log[(1, i)].cpu().numpy() - want).max() <= 1e-5
    item = s[2]
    assert torch.equal(item[0], s[2][0]) and tuple(item[1][0].shape) == (8, 16, 2)
    try:
        model().fit(x=seq, y=y, verbose=0)
    except ValueError as e:
        assert "Sequence" in str(e)
    else:
        raise AssertionError("y alongside a Sequence must be refused")
print("FIT-OK")
"""


@pytest.mark.parametrize("path", ["plan", "eager"])
def test_fit_on_a_sequence(tmp_path, path):
    """Identity parameters and balance=False: the History and the final variables of fit(x=list, y=labels), bit for bit, on
    the recorded and on the Python schedule; with augmentation: other points every epoch, reproducible from the seed; y
    alongside a Sequence is a ValueError.  A child process: the schedule is chosen by LISEC_TUNING at start-up."""
    script = tmp_path / "fit_sequence.py"
    script.write_text(_FIT)
    env = dict(os.environ, LISEC_TUNING="step_plan=%d" % (path == "plan"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), path], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FIT-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
