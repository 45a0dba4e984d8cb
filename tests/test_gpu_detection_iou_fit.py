"""The detection loss with the IoU term in Model.fit / evaluate / save / load_model: losses.VoxelNetIoULoss on the small grid
and sweeps of tests/test_gpu_detection_fit.py, against the fp64 definition (tests/detection_iou_loss_ref.py) and, with
iou_weight=0, against loss='voxelnet' bit for bit."""
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

import detection_iou_loss_ref as R  # noqa: E402
from test_gpu_optimizers import _data, _dump, _same  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["loss", "ClassificationLayer_loss", "RegressionLayer_loss", "RegressionLayer_positive_iou"]
PARAMS = dict(alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0)
IOU = dict(iou_weight=2.0, iou_mode="3d")
WEIGHTS = [2.0, 0.5]


def _model(mt, loss, **kw):
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.9, nesterov=True), loss=loss,
                  loss_weights=WEIGHTS, **kw)
    return model


def _fit(model, x, y, lo, hi):
    return model.fit(x=x[lo:hi], y=[y[0][lo:hi], y[1][lo:hi]], batch_size=1, verbose=0, epochs=1, shuffle=False)


# ---- worker processes: the step-plan knob is read once per process -------------------------------------------------------
def _worker(args):
    from lisec_amd import model_training as mt
    mode, step_plan, out = args["mode"], bool(args["step_plan"]), args["out"]
    x, y = _data(mt, step_plan, n=4)
    hists = {}
    if mode == "resume":
        model = mt.load_model(args["ckpt"])
        want = mt.losses.compile_loss(mt.losses.VoxelNetIoULoss(**PARAMS, **IOU), loss_weights=WEIGHTS,
                                      metrics=["positive_iou"])[0]
        assert isinstance(model.loss, mt.losses.DetectionIoULossSpec) and model.loss == want
        assert model.metrics_names == NAMES
        hists["resumed"] = _fit(model, x, y, 3, 4).history
        _dump(model, out + ".resumed.npz")
    else:
        model = _model(mt, mt.losses.VoxelNetIoULoss(**PARAMS, **IOU), metrics=["positive_iou"])
        assert isinstance(model.loss, mt.losses.DetectionIoULossSpec) and model.metrics_names == NAMES
        hist = _fit(model, x, y, 0, 3)
        assert (getattr(model, "_captured", None) is not None) == step_plan
        assert list(hist.history) == NAMES
        hists["three"] = hist.history
        _dump(model, out + ".three.npz")
    if mode == "plan":
        model.save(args["ckpt"])
        four = _model(mt, mt.losses.VoxelNetIoULoss(**PARAMS, **IOU), metrics=["positive_iou"])
        _fit(four, x, y, 0, 3)
        _fit(four, x, y, 3, 4)
        _dump(four, out + ".four.npz")
        for tag, loss in (("plain", "voxelnet"), ("zero", mt.losses.VoxelNetIoULoss(iou_weight=0.0))):
            m = _model(mt, loss)
            hists[tag] = _fit(m, x, y, 0, 3).history
            assert getattr(m, "_captured", None) is not None
            _dump(m, out + f".{tag}.npz")
    with open(out + ".json", "w") as f:
        json.dump(hists, f)


def _run(tmp, tag, **args):
    out = str(tmp / tag)
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out + ".json") as f:
        hists = json.load(f)
    return (lambda name: dict(np.load(f"{out}.{name}.npz"))), hists


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """From the recorded plan, in one process: three steps (saved), three steps and one more, and three steps each under
    'voxelnet' and under VoxelNetIoULoss(iou_weight=0)."""
    tmp = tmp_path_factory.mktemp("plan")
    ckpt = str(tmp / "ckpt.h5")
    load, hists = _run(tmp, "plan", mode="plan", step_plan=1, ckpt=ckpt)
    return load, hists, ckpt


def test_fit_history_and_step_plan_is_bit_identical_to_python_schedule(tmp_path, planned):
    load, hists, _ = planned
    eager, he = _run(tmp_path, "eager", mode="eager", step_plan=0)
    h = hists["three"]
    assert list(h) == NAMES and all(len(v) == 1 and np.isfinite(v).all() for v in h.values())
    assert 0.0 <= h["RegressionLayer_positive_iou"][0] <= 1.0
    assert abs(h["loss"][0] - (WEIGHTS[0] * h["ClassificationLayer_loss"][0] + WEIGHTS[1] * h["RegressionLayer_loss"][0])) \
        <= 1e-6 * abs(h["loss"][0])
    assert int(load("three")["iterations"]) == 3
    _same(load("three"), eager("three"))
    assert h == he["three"]


def test_save_load_resume_is_bit_identical(tmp_path, planned):
    """3 steps -> save -> load_model (compiled with an equal spec: asserted in the worker) -> 1 step == 3 steps and 1 step
    of one model."""
    from lisec_amd import keras_h5
    load, _, ckpt = planned
    ck = keras_h5.load_model(ckpt)
    assert ck["loss_weights"] == WEIGHTS and ck["loss"]["class_name"] == "VoxelNetIoULoss"
    assert {k: ck["loss"]["config"][k] for k in dict(PARAMS, **IOU)} == dict(PARAMS, **IOU)
    resumed, hr = _run(tmp_path, "resumed", mode="resume", step_plan=1, ckpt=ckpt)
    _same(load("four"), resumed("resumed"))
    assert list(hr["resumed"]) == NAMES and all(np.isfinite(v).all() for v in hr["resumed"].values())


def test_iou_weight_zero_trains_as_voxelnet(planned):
    load, hists, _ = planned
    _same(load("plain"), load("zero"))
    assert hists["plain"] == hists["zero"] and int(load("zero")["iterations"]) == 3


def test_evaluate_is_the_definition_on_predict():
    from lisec_amd import model_training as mt
    model = _model(mt, mt.losses.VoxelNetIoULoss(**PARAMS, **IOU), metrics=["positive_iou"])
    x, y = _data(mt, True, n=4)
    _fit(model, x, y, 0, 3)
    d = model.evaluate(x, y, verbose=0, return_dict=True)
    assert list(d) == NAMES
    cls, reg = model.predict(x)
    rows, ious = [], []
    for i in range(len(cls)):
        head = np.concatenate([cls[i].reshape(-1, 2), reg[i].reshape(-1, 14)], 1)
        rows.append(R.detection_iou_loss(head, y[0][i], y[1][i], weights=WEIGHTS, **PARAMS, **IOU)[0].astype(np.float32))
        ious.append(R.decoded_iou(*R.positives(head, y[0][i], y[1][i])[2:], "bev"))      # 'positive_iou': PositiveIoU()
    print("evaluate", d, "definition", np.mean(np.float64(rows), 0))
    # per sweep the fp32 rounding of an fp64 value (rtol 1e-6); the mean of four such values in fp64 adds nothing
    np.testing.assert_allclose([d[k] for k in NAMES[:3]], np.mean(np.float64(rows), 0), rtol=1e-6, atol=0)
    np.testing.assert_allclose(d[NAMES[3]], np.concatenate(ious).mean(), rtol=1e-12, atol=1e-15)
    with pytest.raises(NotImplementedError, match="metrics"):
        _model(mt, "voxelnet_iou", metrics=["mae"])
    with pytest.raises(ValueError, match="joint loss"):
        model.compile(optimizer="sgd", loss=[mt.losses.VoxelNetIoULoss(), "mse"])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _worker(json.loads(sys.argv[2]))
