"""The detection metrics in Model.fit / evaluate / save / load_model: compile(loss=VoxelNetLoss, metrics=[all five]) on the small
grid and the fixtures of tests/test_gpu_detection_fit.py, against the fp64 definitions of tests/detection_metrics_ref.py on
the net's own head map, read back after every step.

Tolerances, per logged value (a ratio of two pooled sums): the three count metrics are == (exact integers divided once, in
IEEE double on both sides; the worker asserts that no looked-at anchor lies within 1e-6 of a threshold); positive_mae rtol
1e-10 and positive_iou atol 1e-9, the bounds tests/test_gpu_detection_metrics.py holds the sums to, carried through the
division by the exact denominator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import detection_metrics_ref as R  # noqa: E402
from test_gpu_detection_fit import NAMES, PARAMS, WEIGHTS  # noqa: E402
from test_gpu_optimizers import _data, _dump, _same  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE = ["anchor_precision", "anchor_recall", "anchor_accuracy", "positive_mae", "positive_iou"]
METRIC_NAMES = ["ClassificationLayer_" + n for n in FIVE[:3]] + ["RegressionLayer_" + n for n in FIVE[3:]]
ALL = NAMES + METRIC_NAMES
RECALL = "val_ClassificationLayer_anchor_recall"


def _compile(model, metrics=True):
    from lisec_amd import model_training as mt
    # a flat list in any order: each metric finds its output, the class output's come first
    given = [mt.metrics.PositiveMeanAbsoluteError(), mt.metrics.AnchorPrecision(), "anchor_recall", "positive_iou",
             "anchor_accuracy"]
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.9, nesterov=True),
                  loss=mt.losses.VoxelNetLoss(**PARAMS), loss_weights=WEIGHTS, metrics=given if metrics else None)


def _fresh(metrics=True):
    from lisec_amd import model_training as mt
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    _compile(model, metrics)
    return model


def _pairs(head, y_cls, y_reg):
    """The five (num, den) of one sweep from the oracle, in the order of METRIC_NAMES."""
    head = np.asarray(head, np.float64).reshape(-1, 16)
    return [list(R.pair(n, head, y_cls, y_reg)) for n in FIVE]


def _margin(head, y_cls):
    """The smallest |p - 0.5| over the looked-at anchors (the three thresholds are the default 0.5)."""
    pos, neg = R.masks(np.asarray(y_cls).reshape(-1, 2))
    p = R.sigmoid(np.asarray(head, np.float64).reshape(-1, 16)[:, :2])[pos | neg]
    return float(np.abs(p - 0.5).min())


def _values(pairs_per_sweep):
    return [R.value([s[k] for s in pairs_per_sweep]) for k in range(len(FIVE))]


def _close(got, want):
    """got, want: the five metric values in the order of METRIC_NAMES."""
    assert got[:3] == want[:3], (got, want)
    np.testing.assert_allclose(got[3], want[3], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got[4], want[4], rtol=0, atol=1e-9)


# ---- eager schedule against the recorded plan (worker processes: the step-plan knob is read once per process) ----------
def _worker(args):
    import torch
    step_plan, metrics = bool(args["step_plan"]), bool(args["metrics"])
    model = _fresh(metrics)
    from lisec_amd import model_training as mt
    assert model.metrics_names == (ALL if metrics else NAMES)
    tx, ty = _data(mt, step_plan, n=3)
    # the validation sweep runs the eager forward in both workers: padded in both, so that its kernels plan alike
    x, y = _data(mt, False, n=4)
    vx, vy = x[3:], [y[0][3:], y[1][3:]]
    seen, net = [], model.net
    if not step_plan and metrics:
        inner = net.train_step

        def train_step(sample, y_cls, y_reg, **kw):              # the step, then its head map and targets read back
            out = inner(sample, y_cls, y_reg, **kw)
            torch.cuda.synchronize()
            seen.append((net.act["head"].cpu().numpy().copy(), y_cls.cpu().numpy(), y_reg.cpu().numpy()))
            return out
        net.train_step = train_step
    hist = model.fit(x=tx, y=ty, batch_size=1, verbose=0, epochs=2, steps_per_epoch=3, shuffle=False,
                     validation_data=(vx, vy))
    assert (getattr(model, "_captured", None) is not None) == step_plan
    names = ALL if metrics else NAMES
    assert list(hist.history) == names + ["val_" + n for n in names]
    out = dict(history=hist.history)
    if seen:
        assert len(seen) == 6
        out["oracle"] = [_values([_pairs(*s) for s in seen[3 * e:3 * e + 3]]) for e in range(2)]
        out["margin"] = min(_margin(s[0], s[1]) for s in seen)
        # the validation sweep of the last epoch is the last forward: evaluate() runs it again on unchanged weights
        ev = model.evaluate(vx, vy, verbose=0)
        torch.cuda.synchronize()
        head = net.act["head"].cpu().numpy().copy()
        assert ev == [hist.history["val_" + n][1] for n in names]
        out["val_oracle"] = _values([_pairs(head, vy[0][0], vy[1][0])])
        out["margin"] = min(out["margin"], _margin(head, vy[0][0]))
    _dump(model, args["out"])
    with open(args["out"] + ".json", "w") as f:
        json.dump(out, f)


def _run(tmp, tag, **args):
    out = str(tmp / f"{tag}.npz")
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out + ".json") as f:
        return dict(np.load(out)), json.load(f)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """Two epochs of three steps with validation from the recorded plan, all five metrics compiled."""
    return _run(tmp_path_factory.mktemp("plan"), "plan", step_plan=1, metrics=1)


def test_fit_logs_the_oracles_pooled_ratios_and_the_plan_logs_the_eager_bits(tmp_path, planned):
    state_p, plan = planned
    state_e, eager = _run(tmp_path, "eager", step_plan=0, metrics=1)
    hp, he = plan["history"], eager["history"]
    print("margin", eager["margin"], "oracle", eager["oracle"], "val", eager["val_oracle"])
    print("logged", [[he[n][e] for n in METRIC_NAMES] for e in range(2)], [he["val_" + n][1] for n in METRIC_NAMES])
    assert eager["margin"] >= 1e-6
    for e in range(2):
        _close([he[n][e] for n in METRIC_NAMES], eager["oracle"][e])
    _close([he["val_" + n][1] for n in METRIC_NAMES], eager["val_oracle"])
    # the labels of the fixtures hold positives and negatives in every sweep: accuracy and MAE are not trivially 0
    assert all(0 < he[n][e] for n in METRIC_NAMES[2:4] for e in range(2))
    assert all(np.isfinite(v).all() and len(v) == 2 for v in he.values())
    # eager schedule == recorded plan, to the bit: the variables and every logged value
    _same(state_p, state_e)
    assert hp == he


def test_the_metrics_perturb_nothing(tmp_path, planned):
    """The same model compiled without metrics: three names, and the same bits in its variables and on the loss keys."""
    state_p, plan = planned
    state_n, bare = _run(tmp_path, "bare", step_plan=1, metrics=0)
    assert list(bare["history"]) == NAMES + ["val_" + n for n in NAMES]
    _same(state_p, state_n)
    for key, v in bare["history"].items():
        assert plan["history"][key] == v, key


# ---- evaluate, callbacks, save / load_model (in this process; sweeps padded to the plan's capacity) --------------------
def test_evaluate_eval_plan_early_stopping_and_save_load(tmp_path, monkeypatch):
    from lisec_amd import model_training as mt
    model = _fresh()
    assert model.metrics_names == ALL and model.loss.n_metrics == 5
    assert len(_fresh(metrics=False).metrics_names) == 3
    x, y = _data(mt, False, n=4)                                 # padded sweeps: the evaluation plan gives the eager bits
    tx, ty, vx, vy = x[:3], [y[0][:3], y[1][:3]], x[3:], [y[0][3:], y[1][3:]]

    class Rec(mt.callbacks.Callback):
        def __init__(self):
            super().__init__()
            self.seen = []

        def on_epoch_end(self, epoch, logs=None):
            assert list(logs) == ALL + ["val_" + n for n in ALL]
            self.seen.append(logs[RECALL])

    rec = Rec()
    hist = model.fit(x=tx, y=ty, batch_size=1, verbose=0, epochs=2, shuffle=False, validation_data=(vx, vy), callbacks=[rec])
    assert list(hist.history) == ALL + ["val_" + n for n in ALL] and rec.seen == hist.history[RECALL]
    # evaluate(): list and dict, eagerly and from the recorded evaluation plan
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=0")
    eager = model.evaluate(x, y, verbose=0)
    assert model._eval_captured is None
    d = model.evaluate(x, y, verbose=0, return_dict=True)
    assert list(d) == ALL and list(d.values()) == eager
    assert model.evaluate(vx, vy, verbose=0) == [hist.history["val_" + n][1] for n in ALL]
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=1")
    replay = model.evaluate(x, y, verbose=0)
    assert model._eval_captured is not None and model._eval_captured[1].nacc == 4 + 2 * 5
    assert replay == eager
    assert model.evaluate(x, y, verbose=0) == eager                # the accumulator is zeroed between evaluations
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=0")
    # pooled over the four sweeps, not a mean of four ratios: the oracle on predict()'s maps
    cls, reg = model.predict(x)
    pairs = [_pairs(np.concatenate([cls[i].reshape(-1, 2), reg[i].reshape(-1, 14)], 1), y[0][i], y[1][i]) for i in range(4)]
    assert min(_margin(np.concatenate([cls[i].reshape(-1, 2), reg[i].reshape(-1, 14)], 1), y[0][i]) for i in range(4)) >= 1e-6
    _close(eager[3:], _values(pairs))
    # save() -> load_model: compiled with equal metrics, evaluates to the same numbers
    ckpt = str(tmp_path / "ckpt.h5")
    model.save(ckpt)
    from lisec_amd import keras_h5
    saved = keras_h5.load_model(ckpt)["metrics"]
    assert [m if isinstance(m, str) else m["class_name"] for m in saved] == [
        "PositiveMeanAbsoluteError", "AnchorPrecision", "anchor_recall", "positive_iou", "anchor_accuracy"]
    loaded = mt.load_model(ckpt)
    assert loaded.loss == model.loss and hash(loaded.loss) == hash(model.loss) and loaded.metrics_names == ALL
    assert loaded.evaluate(x, y, verbose=0) == eager
    # EarlyStopping on the validation recall: nothing beats a baseline of 2 in mode max ...
    es = mt.callbacks.EarlyStopping(monitor=RECALL, mode="max", patience=0, baseline=2.0)
    h = model.fit(x=tx, y=ty, batch_size=1, verbose=0, epochs=5, shuffle=False, validation_data=(vx, vy), callbacks=[es])
    assert len(h.history[RECALL]) == 1 and model.stop_training
    # ... and without one it stops at the first epoch that does not improve on the best so far
    rec, es = Rec(), mt.callbacks.EarlyStopping(monitor=RECALL, mode="max", patience=0)
    h = model.fit(x=tx, y=ty, batch_size=1, verbose=0, epochs=6, shuffle=False, validation_data=(vx, vy),
                  callbacks=[rec, es])
    stops = [i for i in range(1, len(rec.seen)) if not rec.seen[i] > max(rec.seen[:i])]
    assert len(h.history["loss"]) == (stops[0] + 1 if stops else 6) == len(rec.seen)
    # a detection metric needs the detection loss; the Keras metrics stay refused beside it
    with pytest.raises(NotImplementedError, match="loss='voxelnet'"):
        model.compile(optimizer="sgd", loss="mse", metrics=["anchor_recall"])
    with pytest.raises(NotImplementedError, match="metrics"):
        model.compile(optimizer="sgd", loss="voxelnet", metrics=["anchor_recall", "mae"])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _worker(json.loads(sys.argv[2]))
