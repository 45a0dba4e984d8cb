"""The VoxelNet detection loss in the training step: LisecNet.backward with a DetectionLossSpec against the fp64 definition
(tests/detection_loss_ref.py) on the net's own head map, and Model.fit / evaluate / save / load_model with
losses.VoxelNetLoss on the small grid of tests/test_gpu_optimizers.py."""
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

import detection_loss_ref as R  # noqa: E402
from test_gpu_optimizers import SMALL, _cloud, _data, _dump, _same, _targets  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["loss", "ClassificationLayer_loss", "RegressionLayer_loss"]
PARAMS = dict(alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0)
WEIGHTS = [2.0, 0.5]
TINY = float(np.finfo(np.float32).tiny)


def _compile(model, **kw):
    from lisec_amd import model_training as mt
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.9, nesterov=True),
                  loss=mt.losses.VoxelNetLoss(**PARAMS), loss_weights=WEIGHTS, **kw)


def _close(got, ref):
    """fp32 rounding of an fp64 value: rtol 1e-6, atol 0 (against the fp32 rounding of the oracle where it lies below
    the fp32 normal range), as in tests/test_gpu_detection_loss.py."""
    ref = np.asarray(ref, np.float64)
    want = np.where(np.abs(ref) >= TINY, ref, ref.astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-6, atol=0)


def test_backward_writes_the_oracles_head_gradient_and_loss():
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.voxelizer import Voxelizer
    model = mt.createModel(16, 32, 8, 35)
    _compile(model)
    spec, net, dev = model.loss, model.net, model.net.device
    assert isinstance(spec, mt.losses.DetectionLossSpec) and model.metrics_names == NAMES
    sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(0)).to(dev))
    y_cls, y_reg = _targets(0)
    yc, yr = (torch.from_numpy(a).to(dev) for a in (y_cls, y_reg))
    for grad_scale in (1.0, 0.5):
        net.forward(sample, training=True)
        lo = net.backward(yc, yr, loss=spec, grad_scale=grad_scale)
        torch.cuda.synchronize()
        head = net.act["head"].cpu().numpy().reshape(-1, 16)
        r_loss, r_counts, r_grad = R.detection_loss(head, y_cls, y_reg, weights=WEIGHTS, grad_scale=grad_scale, **PARAMS)
        assert r_counts.min() > 0 and np.array_equal(net.loss_counts.cpu().numpy(), r_counts)
        _close(lo.cpu().numpy(), r_loss)
        _close(net.dact["head"].cpu().numpy().reshape(-1, 16), r_grad)
        assert np.abs(net.grad.cpu().numpy()).max() > 0


# ---- Model.fit / save / load_model (worker processes: the step-plan knob is read once per process) ---------------------
def _worker(args):
    from lisec_amd import model_training as mt
    mode, step_plan = args["mode"], bool(args["step_plan"])
    np.random.seed(0)
    if mode == "resume":
        model = mt.load_model(args["ckpt"])
        assert model.loss == mt.losses.compile_loss(mt.losses.VoxelNetLoss(**PARAMS), loss_weights=WEIGHTS)[0]
    else:
        model = mt.createModel(16, 32, 8, 35)
        _compile(model)
    assert model.metrics_names == NAMES
    x, y = _data(mt, step_plan)
    epochs = 2 if mode == "fit6" else 1
    hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=epochs, steps_per_epoch=3, shuffle=False)
    assert (getattr(model, "_captured", None) is not None) == step_plan
    assert list(hist.history) == NAMES
    if mode == "save":
        model.save(args["ckpt"])
    _dump(model, args["out"])
    with open(args["out"] + ".json", "w") as f:
        json.dump(hist.history, f)


def _run(tmp, tag, **args):
    out = str(tmp / f"{tag}.npz")
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out + ".json") as f:
        hist = json.load(f)
    return dict(np.load(out)), hist


@pytest.fixture(scope="module")
def six_planned_steps(tmp_path_factory):
    """Two epochs of three steps from the recorded plan: the run both comparisons below start from."""
    return _run(tmp_path_factory.mktemp("whole"), "whole", mode="fit6", step_plan=1)


def test_fit_step_plan_is_bit_identical_to_python_schedule(tmp_path, six_planned_steps):
    plan, hp = six_planned_steps
    eager, he = _run(tmp_path, "eager", mode="fit6", step_plan=0)
    assert int(plan["iterations"]) == 6
    _same(plan, eager)
    assert hp == he and all(np.isfinite(v).all() and len(v) == 2 for v in hp.values())


def test_save_load_resume_is_bit_identical(tmp_path, six_planned_steps):
    """3 steps -> save -> load_model (compiled with an equal spec: asserted in the worker) -> 3 steps == 6 steps."""
    from lisec_amd import keras_h5
    whole, hw = six_planned_steps
    ckpt = str(tmp_path / "ckpt.h5")
    _run(tmp_path, "half", mode="save", step_plan=1, ckpt=ckpt)
    ck = keras_h5.load_model(ckpt)
    assert ck["loss_weights"] == WEIGHTS and ck["loss"]["class_name"] == "VoxelNetLoss"
    assert {k: ck["loss"]["config"][k] for k in PARAMS} == PARAMS and ck["metrics"] is None
    resumed, hr = _run(tmp_path, "resumed", mode="resume", step_plan=1, ckpt=ckpt)
    _same(whole, resumed)
    assert {k: v[1] for k, v in hw.items()} == {k: v[0] for k, v in hr.items()}


def test_evaluate_validation_and_recompile():
    """evaluate() equals the oracle on predict(); fit(validation_data=) logs the three val_ keys, each the evaluate() of
    the validation sweep; compile(loss='mse') afterwards runs the legacy kernel again."""
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd import ops
    from lisec_amd.voxelizer import Voxelizer
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    _compile(model)
    x, y = _data(mt, True, n=4)
    vx, vy = x[3:], [y[0][3:], y[1][3:]]
    hist = model.fit(x=x[:3], y=[y[0][:3], y[1][:3]], batch_size=1, verbose=0, epochs=2, shuffle=False,
                     validation_data=(vx, vy))
    assert list(hist.history) == NAMES + ["val_" + n for n in NAMES]
    for e in range(2):
        h = {k: v[e] for k, v in hist.history.items()}
        for pre in ("", "val_"):
            assert abs(h[pre + "loss"] - (WEIGHTS[0] * h[pre + "ClassificationLayer_loss"]
                                          + WEIGHTS[1] * h[pre + "RegressionLayer_loss"])) <= 1e-6 * abs(h[pre + "loss"])
    got = model.evaluate(vx, vy, verbose=0)
    assert got == [hist.history["val_" + n][1] for n in NAMES]
    d = model.evaluate(x, y, verbose=0, return_dict=True)
    assert list(d) == NAMES
    cls, reg = model.predict(x)
    rows = []
    for i in range(len(cls)):
        head = np.concatenate([cls[i].reshape(-1, 2), reg[i].reshape(-1, 14)], 1)
        rows.append(R.detection_loss(head, y[0][i], y[1][i], weights=WEIGHTS, **PARAMS)[0].astype(np.float32))
    # per sweep the fp32 rounding of an fp64 value (rtol 1e-6, derived in tests/test_gpu_detection_loss.py); the mean of
    # four such values in fp64 adds nothing
    np.testing.assert_allclose([d[k] for k in NAMES], np.mean(np.float64(rows), 0), rtol=1e-6, atol=0)
    with pytest.raises(NotImplementedError, match="metrics"):
        _compile(model, metrics=["mae"])
    with pytest.raises(ValueError, match="joint loss"):
        model.compile(optimizer="sgd", loss=[mt.losses.VoxelNetLoss(), "mse"])
    # the legacy step is untouched: 'mse' compiles to the string and lisec_rpn_loss writes the head gradient
    model.compile(optimizer="sgd", loss="mse")
    assert model.loss == "mse" and model._compile_args is None
    net, dev = model.net, model.net.device
    sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(0)).to(dev))
    yc, yr = (torch.from_numpy(a).to(dev) for a in _targets(0))
    net.forward(sample, training=True)
    lo = net.backward(yc, yr, loss=model.loss).clone()
    ref = torch.zeros_like(net.dact["head"])
    ref_lo = torch.zeros(3, dtype=torch.float32, device=dev)
    ops.rpn_loss(net.act["head"], yc, yr, net.Ho * net.Wo, 0, ref, ref_lo)
    torch.cuda.synchronize()
    assert torch.equal(net.dact["head"], ref) and torch.equal(lo, ref_lo)
    hist = model.fit(x=x[:3], y=[y[0][:3], y[1][:3]], batch_size=1, verbose=0, epochs=1, shuffle=False)
    assert list(hist.history) == NAMES and model.loss == "mse"


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _worker(json.loads(sys.argv[2]))
