"""optimizers.MovingAverage / optimizers.SWA in Model.fit on the small grid of the optimizer tests (createModel(16, 32, 8,
35)): the average is the numpy definition (tests/weight_average_ref.py) of the variables after each update, bit for bit;
the training itself is untouched; the recorded plans leave the bits of the Python schedule and grow by exactly the one
averaging launch; average_weights() swaps in and back without a trace; checkpoints carry the average."""
import os
import subprocess
import sys

import numpy as np
import pytest

import weight_average_ref as R
from test_gpu_batch_fit import PARENT_LAUNCHES, _tuning
from test_gpu_optimizers import _data, _targets  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

AVERAGE_LAUNCHES = 1                       # what a wrapper adds to the plan of a step that updates: the averaging pass


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _floats(b):
    return b.view(np.float32)


def _opt(name, wrapped):
    from lisec_amd import model_training as mt
    O = mt.optimizers
    inner = {"ema": lambda: O.SGD(lr=0.01, decay=1e-3, momentum=0.9),
             "swa": lambda: O.SGD(lr=0.01, decay=1e-3, momentum=0.9),
             "adam": lambda: O.Adam(learning_rate=1e-3, decay=1e-3),
             "reg": lambda: O.SGD(lr=0.01, decay=1e-3, momentum=0.9)}[name]()
    if not wrapped:
        return inner
    if name == "swa":
        return O.SWA(inner, start_averaging=1, average_period=2)
    return O.MovingAverage(inner, average_decay=0.9, dynamic_decay=True)


def _reference_average(name, thetas):
    """The numpy definition over the variables after each update (thetas[0]: the start, where the average starts too)."""
    a = _floats(thetas[0]).copy()
    for s, th in enumerate(thetas[1:]):
        if name == "swa":
            a = R.swa_step(a, _floats(th), s, 1, 2)
        else:
            a = R.ema_step(a, _floats(th), s, 0.9, dynamic_decay=True)
    return R.bits(a)


def _model(name):
    from lisec_amd import model_training as mt
    kw = dict(kernel_regularizer=mt.regularizers.l2(1e-4)) if name == "reg" else {}
    return mt.createModel(16, 32, 8, 35, **kw)


_RUNS = {}


def _run(name, wrapped, tuning, B=1):
    """Five sweeps, one epoch (B = 3: batches of three and two sweeps, two epochs: four updates), from the default
    initial weights; run once and shared.  Under the Python schedule theta is read after every update."""
    key = (name, wrapped, tuning, B)
    if key in _RUNS:
        return _RUNS[key]
    from lisec_amd import _lib
    from lisec_amd import model_training as mt
    with _tuning(tuning):
        eager = tuning == "step_plan=0"
        model = _model(name)
        opt = _opt(name, wrapped)
        model.compile(optimizer=opt, loss=['mse', 'mse'])
        net = model.net
        thetas = [_bits(net.params.theta)]
        x, y = _data(mt, not eager, n=5)
        if eager:
            inner = net.train_micro_step

            def spy(sample, yc, yr, position, **kw):
                out = inner(sample, yc, yr, position, **kw)
                if position in ("single", "last"):
                    thetas.append(_bits(net.params.theta))
                return out
            net.train_micro_step = spy
        model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=1 if B == 1 else 2, shuffle=False)
        assert (model._captured is None) == eager
        r = dict(thetas=thetas, theta=_bits(net.params.theta), state=_bits(net.params.state),
                 iterations=net.iterations, iter_dev=net._iter_dev.cpu().tolist(),
                 slots={k: _bits(net.slot(k)) for k in opt.spec().slots})
        if wrapped:
            r["average"] = _bits(net.average)
        else:
            assert net._average is None                      # nothing of an average exists without a wrapper
        step = None if eager else model._captured[1]
        if step is not None:
            r["launches"] = step.launches
            r["micro"] = {k: _lib.load().lisec_step_plan_size(p) for k, p in step.micro.items()}
            r["kind"] = type(step).__name__
            step.close()
    _RUNS[key] = r
    return r


def _same_training(a, b):
    assert a["iterations"] == b["iterations"] and a["iter_dev"] == b["iter_dev"]
    assert np.array_equal(a["theta"], b["theta"]) and np.array_equal(a["state"], b["state"])
    assert sorted(a["slots"]) == sorted(b["slots"])
    for k in a["slots"]:
        assert np.array_equal(a["slots"][k], b["slots"][k]), k


@pytest.mark.parametrize("name", ["ema", "swa", "adam", "reg"])
def test_the_average_is_the_definition_and_training_is_untouched(name):
    """Python schedule: the final average is the numpy definition over the five theta snapshots, bit for bit; the sequence of
    theta is that of the same run without the wrapper (Adam: its device-side bias correction reads the count the pass
    reads too, and must not see it disturbed)."""
    w, plain = _run(name, True, "step_plan=0"), _run(name, False, "step_plan=0")
    assert w["iterations"] == 5 and w["iter_dev"] == [5, 0] and len(w["thetas"]) == 6
    assert np.array_equal(w["thetas"][-1], w["theta"])
    want = _reference_average(name, w["thetas"])
    assert np.array_equal(w["average"], want)
    assert not np.array_equal(w["average"], w["theta"]) and not np.array_equal(w["average"], w["thetas"][0])
    assert len(plain["thetas"]) == 6
    for s, (a, b) in enumerate(zip(w["thetas"], plain["thetas"])):
        assert np.array_equal(a, b), s
    _same_training(w, plain)
    if name == "swa":                                        # snapshots at s = 1 and 3: not the mean over all five
        assert not np.array_equal(want, _reference_average("ema", w["thetas"]))


@pytest.mark.parametrize("name,tuning", [("ema", "pipeline_voxels=0"), ("ema", ""), ("swa", ""), ("adam", ""), ("reg", "")])
def test_recorded_plans_leave_the_bits_of_the_python_schedule(name, tuning):
    eager, plan = _run(name, True, "step_plan=0"), _run(name, True, tuning)
    assert plan["kind"] == ("RecordedStep" if tuning else "PipelinedStep")
    _same_training(eager, plan)
    assert np.array_equal(eager["average"], plan["average"])


def test_batches_average_once_per_update():
    """batch_size=3 on five sweeps, two epochs: four updates, four passes -- by the value, and by the launch counts of the
    recorded plans (a sweep that only accumulates records nothing more than without the wrapper)."""
    eager = _run("ema", True, "step_plan=0", B=3)
    assert eager["iterations"] == 4 and len(eager["thetas"]) == 5
    assert np.array_equal(eager["average"], _reference_average("ema", eager["thetas"]))
    plan, plain = _run("ema", True, "pipeline_voxels=0", B=3), _run("ema", False, "pipeline_voxels=0", B=3)
    _same_training(eager, plan)
    assert np.array_equal(eager["average"], plan["average"])
    _same_training(plan, plain)
    assert plain["micro"]["last", 0] == PARENT_LAUNCHES + 2
    assert plan["micro"]["last", 0] == plain["micro"]["last", 0] + AVERAGE_LAUNCHES
    for position in ("first", "middle"):
        assert plan["micro"][position, 0] == plain["micro"][position, 0] < PARENT_LAUNCHES


def test_plan_sizes():
    """Without a wrapper the batch-1 plan is the one test_gpu_batch_fit pins; with one it holds exactly the averaging pass
    more (the SWA pass is launched at every update: whether it is a snapshot is decided on the device)."""
    assert _run("ema", False, "pipeline_voxels=0")["launches"] == PARENT_LAUNCHES
    assert _run("ema", True, "pipeline_voxels=0")["launches"] == PARENT_LAUNCHES + AVERAGE_LAUNCHES
    assert _run("ema", True, "pipeline_voxels=0", B=3)["launches"] == PARENT_LAUNCHES + AVERAGE_LAUNCHES
    assert _run("ema", False, "pipeline_voxels=0", B=3)["launches"] == PARENT_LAUNCHES
    with _tuning("pipeline_voxels=0"):
        from lisec_amd import model_training as mt
        model = _model("swa")
        model.compile(optimizer=_opt("swa", True), loss=['mse', 'mse'])
        x, y = _data(mt, True, n=2)
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False)
        assert model._captured[1].launches == PARENT_LAUNCHES + AVERAGE_LAUNCHES
        model._captured[1].close()


def test_recompiling_restarts_the_average_under_the_cached_plan():
    """compile() again with an equal wrapper: the plan of the first fit is replayed (same key), the iteration count and
    the average start again -- the average from the variables as they are at the first step after compile()."""
    from lisec_amd import model_training as mt
    model = _model("ema")
    x, y = _data(mt, True, n=2)
    seen = []

    class Reader(mt.callbacks.Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append(_bits(model.net.params.theta))

    model.compile(optimizer=_opt("ema", True), loss=['mse', 'mse'])
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, steps_per_epoch=1, shuffle=False, callbacks=[Reader()])
    step, first = model._captured[1], _bits(model.net.average)
    model.compile(optimizer=_opt("ema", True), loss=['mse', 'mse'])
    start = _bits(model.net.params.theta)
    del seen[:]
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, steps_per_epoch=1, shuffle=False, callbacks=[Reader()])
    assert model._captured[1] is step and model.net.iterations == 2 and len(seen) == 2
    want = _reference_average("ema", [start] + seen)
    assert np.array_equal(_bits(model.net.average), want) and not np.array_equal(want, first)
    step.close()


def test_average_weights_swaps_in_and_back_without_a_trace():
    """Three updates, then predict / evaluate inside average_weights() against a fresh model that is GIVEN the average as
    its weights; afterwards theta, predict and two more updates from the recorded plans are those of the uninterrupted run
    of five (test_recorded_plans_...'s)."""
    import torch
    from lisec_amd import model_training as mt
    whole = _run("ema", True, "")
    model = _model("ema")
    model.compile(optimizer=_opt("ema", True), loss=['mse', 'mse'])
    net = model.net
    x, y = _data(mt, True, n=5)
    model.fit(x=x[:3], y=[a[:3] for a in y], batch_size=1, verbose=0, epochs=1, shuffle=False)
    step = model._captured[1]
    theta3, avg3, state3 = _bits(net.params.theta), _bits(net.average), _bits(net.params.state)
    assert not np.array_equal(theta3, avg3)
    live = [a.copy() for a in model.predict(x[0])]
    with model.average_weights() as inside:
        assert inside is model
        assert np.array_equal(_bits(net.params.theta), avg3) and np.array_equal(_bits(net.average), theta3)
        got = [a.copy() for a in model.predict(x[0])]
        got_eval = model.evaluate(x[:3], [a[:3] for a in y], verbose=0)
    assert any(not np.array_equal(a, b) for a, b in zip(got, live))        # the averages are another model
    # swapped back: bit for bit, and predict sees the live weights again
    assert np.array_equal(_bits(net.params.theta), theta3) and np.array_equal(_bits(net.average), avg3)
    assert np.array_equal(_bits(net.params.state), state3)
    for a, b in zip(model.predict(x[0]), live):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # also on an exception
    with pytest.raises(KeyError):
        with model.average_weights():
            raise KeyError("inside")
    assert np.array_equal(_bits(net.params.theta), theta3) and np.array_equal(_bits(net.average), avg3)
    # the next steps, from the same recorded plans: the uninterrupted run
    model.fit(x=x[3:], y=[a[3:] for a in y], batch_size=1, verbose=0, epochs=1, shuffle=False)
    assert model._captured[1] is step and net.iterations == 5
    assert np.array_equal(_bits(net.params.theta), whole["theta"])
    assert np.array_equal(_bits(net.average), whole["average"])
    for k, v in whole["slots"].items():
        assert np.array_equal(_bits(net.slot(k)), v), k
    # assign_average_vars: theta <- average, the average is kept
    model.optimizer.assign_average_vars(model)
    assert np.array_equal(_bits(net.params.theta), whole["average"]) and np.array_equal(_bits(net.average), whole["average"])
    step.close()
    # what was seen inside: a fresh model GIVEN the average as its weights (made last: a second model's workspaces make
    # the first one's recorded plans stale, and the steps above were to replay the plans recorded before the swap)
    fresh = _model("ema")
    fresh._restore_weights((torch.from_numpy(_floats(avg3).copy()).to(net.device),
                            torch.from_numpy(_floats(state3).copy()).to(net.device)))
    fresh.compile(optimizer=_opt("ema", False), loss=['mse', 'mse'])
    want = fresh.predict(x[0])
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert got_eval == fresh.evaluate(x[:3], [a[:3] for a in y], verbose=0)
    # a model without a wrapper has no averages to swap in
    with pytest.raises(ValueError):
        with fresh.average_weights():
            pass


def test_a_swap_with_an_early_update_pending_is_refused():
    import torch
    from lisec_amd import model_training as mt
    with _tuning("step_plan=0"):
        model = _model("ema")
        opt = _opt("ema", True)
        model.compile(optimizer=opt, loss=['mse', 'mse'])
        net, spec = model.net, opt.spec()
        x, y = _data(mt, False, n=1)
        yc, yr = (torch.from_numpy(a[0]).to(net.device) for a in y)
        theta0 = _bits(net.params.theta)
        net.forward(x[0].sample, training=True)
        net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
        assert net._early is not None
        with pytest.raises(RuntimeError, match="early update"):
            net.swap_average()
        with pytest.raises(RuntimeError, match="early update"):
            with model.average_weights():
                pass
        net.apply_gradients(opt=spec)
        theta1 = _bits(net.params.theta)
        # the average started from the variables BEFORE any part of them was updated
        want = R.bits(R.ema_step(_floats(theta0), _floats(theta1), 0, 0.9, dynamic_decay=True))
        assert np.array_equal(_bits(net.average), want) and not np.array_equal(theta0, theta1)
        net.swap_average()
        assert np.array_equal(_bits(net.params.theta), want) and np.array_equal(_bits(net.average), theta1)


def test_save_load_resume_and_average_model_checkpoint(tmp_path):
    """One epoch of three updates -> save -> load_model -> one more epoch: theta, the slots and the average of the
    uninterrupted two epochs, bit for bit (.h5).  AverageModelCheckpoint(update_weights=False) writes a file whose model
    weights are the average and whose average slot holds the live weights, and leaves the training as it was."""
    from lisec_amd import keras_h5
    from lisec_amd import model_training as mt
    x, y = _data(mt, True, n=3)
    ck_path, avg_path = str(tmp_path / "half.h5"), str(tmp_path / "avg-{epoch}.h5")

    def fresh():
        m = _model("ema")
        m.compile(optimizer=_opt("ema", True), loss=['mse', 'mse'])
        return m

    def fit(m, epochs, callbacks=None):
        m.fit(x=x, y=y, batch_size=1, verbose=0, epochs=epochs, shuffle=False, callbacks=callbacks)

    def variables(m):
        net = m.net
        return dict(theta=_bits(net.params.theta), average=_bits(net.average), state=_bits(net.params.state),
                    iter_dev=np.array(net._iter_dev.cpu().tolist()),
                    **{"slot_" + k: _bits(net.slot(k)) for k in m.optimizer.spec().slots})

    def check(a, b):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k

    whole = fresh()
    fit(whole, 2)
    want = variables(whole)
    assert want["iter_dev"].tolist() == [6, 0] and "slot_velocity" in want
    half = fresh()
    fit(half, 1)
    half.save(ck_path)
    resumed = mt.load_model(ck_path)
    assert type(resumed.optimizer) is mt.optimizers.MovingAverage
    assert resumed.optimizer.get_config() == half.optimizer.get_config() and resumed.net.iterations == 3
    check(variables(resumed), variables(half))
    fit(resumed, 1)
    check(variables(resumed), want)
    # .npz: the variables, the wrapper and the average travel (the wrapped optimizer's slots do not)
    npz = str(tmp_path / "half.npz")
    half.save(npz)
    again = mt.load_model(npz)
    assert again.optimizer.get_config() == half.optimizer.get_config() and again.net.iterations == 3
    assert np.array_equal(_bits(again.net.average), _bits(half.net.average))
    assert np.array_equal(_bits(again.net.params.theta), _bits(half.net.params.theta))
    # AverageModelCheckpoint, with callbacks in both runs (a rate read from the device descriptor: another plan key)
    plain, ckpt = fresh(), fresh()
    fit(plain, 2, callbacks=[mt.callbacks.Callback()])
    fit(ckpt, 2, callbacks=[mt.callbacks.AverageModelCheckpoint(False, avg_path)])
    check(variables(ckpt), variables(plain))
    ck = keras_h5.load_model(avg_path.format(epoch=2))
    p = ckpt.net.params
    for n in p.trainable_names():
        assert np.array_equal(R.bits(ck["params"][n]), _bits(p.view(n, buf=ckpt.net.average))), n
        assert np.array_equal(R.bits(ck["average"][n]), _bits(p.view(n))), n
    assert ck["wrapper"]["class_name"] == "MovingAverage" and os.path.exists(avg_path.format(epoch=1))
    # update_weights=True: training goes on from the averages
    moved = fresh()
    fit(moved, 1, callbacks=[mt.callbacks.AverageModelCheckpoint(True, str(tmp_path / "moved.h5"))])
    assert np.array_equal(_bits(moved.net.params.theta), _bits(moved.net.average))
    ck = keras_h5.load_model(str(tmp_path / "moved.h5"))
    for n in ("cls.kernel", "mid1.conv.kernel"):
        assert np.array_equal(R.bits(ck["params"][n]), R.bits(ck["average"][n]))
    with pytest.raises(ValueError, match="MovingAverage"):
        m = _model("ema")
        m.compile(optimizer=_opt("ema", False), loss=['mse', 'mse'])
        fit(m, 1, callbacks=[mt.callbacks.AverageModelCheckpoint(False, str(tmp_path / "never.h5"))])
    for m in (whole, half, resumed, plain, ckpt, moved):
        if m._captured is not None:
            m._captured[1].close()


_DETECTION = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import augment_cases as C
from test_gpu_detection_eval import OUTPUTS
from test_gpu_optimizers import _targets
from lisec_amd import Constants, boxes, callbacks
from lisec_amd import model_training as mt
from lisec_amd.Predict import _cut_to_counts, _detect_sweep
Constants.nx, Constants.ny = 16, 32                 # the (16, 32, 8) grid of the augmentation tests
pts, _ = C.fit_sweeps()
# labels all over what the detector can report on this grid (its boxes are shifted by -50 m), so that predictions meet them
labels = [np.array([[x, y, 1.0, 3.9, 1.6, 1.56, 0.0] for x in np.arange(-52.0, -42.0, 2.0) for y in np.arange(-52.0, -42.0, 1.0)])
          for _ in pts]
grid = (Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, 8, 16, Constants.nz)
x = [mt.VFE_preprocessing(p, *grid) for p in pts]
ys = [_targets(s) for s in range(len(pts))]
y = [np.stack([t[0] for t in ys]), np.stack([t[1] for t in ys])]


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def run(with_callback):
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=mt.optimizers.MovingAverage(mt.optimizers.SGD(lr=0.01, momentum=0.9), average_decay=0.9,
                                                    dynamic_decay=True), loss=['mse', 'mse'])
    ev = callbacks.DetectionEvaluation(pts, labels, iou_thresholds=[0.3, 0.1], average_weights=True)
    h = m.fit(x, y, verbose=0, epochs=2, shuffle=False, callbacks=[ev if with_callback else callbacks.Callback()])
    return m, ev, h.history


def by_hand(m):
    found, probs, counts = [], [], []
    for p in pts:
        for b, s, c in _detect_sweep(p, m, None):
            found.append(b); probs.append(s); counts.append(c)
    found, probs = _cut_to_counts(found, probs, counts)
    return boxes.evaluate_detections(found, probs, labels, iou_thresholds=[0.3, 0.1])


m, ev, hist = run(True)
plain, _, plain_hist = run(False)
for a, b in ((m.net.params.theta, plain.net.params.theta), (m.net.average, plain.net.average),
             (m.net.params.state, plain.net.params.state), (m.net.slot("velocity"), plain.net.slot("velocity"))):
    assert np.array_equal(bits(a), bits(b))
assert m.net.iterations == plain.net.iterations == 6 and hist["loss"] == plain_hist["loss"]
assert len(hist["val_mAP"]) == 2 and "val_mAP" not in plain_hist
with m.average_weights():
    want = by_hand(m)
live = by_hand(m)
assert hist["val_mAP"][-1] == float(want.mAP) and ev.last.n_predictions == want.n_predictions > 0
for name in OUTPUTS:
    a, b = getattr(ev.last, name), getattr(want, name)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
# the live weights are scored differently: the callback did evaluate the averages
assert any(not np.array_equal(getattr(live, n), getattr(want, n), equal_nan=getattr(live, n).dtype.kind == "f") for n in OUTPUTS)
# on a model without a wrapper the callback refuses
bare = mt.createModel(16, 32, 8, 35)
bare.compile(optimizer=mt.optimizers.SGD(lr=0.01), loss=['mse', 'mse'])
try:
    bare.fit(x, y, verbose=0, epochs=1, shuffle=False,
             callbacks=[callbacks.DetectionEvaluation(pts, labels, average_weights=True)])
except ValueError as e:
    assert "MovingAverage" in str(e)
else:
    raise AssertionError("no ValueError")
print("DETECTION-OK")
"""


def test_detection_evaluation_scores_the_averages(tmp_path):
    """fit(epochs=2, callbacks=[DetectionEvaluation(..., average_weights=True)]) ends with the theta and average of the same
    fit without it and logs the val_mAP of the averages.  A child process: the label grid is a module constant."""
    script = tmp_path / "fit_detection.py"
    script.write_text(_DETECTION)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("LISEC_TUNING", None)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "DETECTION-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
