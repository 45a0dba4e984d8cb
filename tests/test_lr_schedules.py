"""tf.keras 2.4 learning-rate schedules and LearningRateScheduler without a GPU: every schedule's value against an
independent fp64 transcription of the TF 2.4 formulas (shared with tests/test_gpu_lr_schedules.py), constructor
validation, Keras (de)serialization, the optimizers' handling of a schedule (spec configs, refusals, get_config), the
Keras `.h5` training_config of a schedule, and the callback's argument handling on a mock model."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from lisec_amd import _lib, keras_h5
from lisec_amd import model_training as mt
from lisec_amd.network import OptimizerSpec
from lisec_amd.params import glorot_numpy

S = mt.optimizers.schedules
H5PY_PYTHON = "/opt/conda/bin/python3.9"          # the interpreter with h5py that tests/test_hdf5_lite.py uses
PROBE = os.path.join(os.path.dirname(__file__), "golden", "h5py_probe.py")


# ---- the reference: the TF 2.4 formulas, written out again in fp64 ----------------------------------------------------
def ref_lr(name, c, s):
    """schedule(s) of the class `name` with Keras config c, s: the iteration count before the update."""
    s = np.float64(s)
    if name == "ExponentialDecay":
        p = s / c["decay_steps"]
        p = np.floor(p) if c.get("staircase") else p
        return float(c["initial_learning_rate"] * np.power(np.float64(c["decay_rate"]), p))
    if name == "PiecewiseConstantDecay":
        b, v = c["boundaries"], c["values"]
        if s <= b[0]:
            return float(v[0])
        if s > b[-1]:
            return float(v[-1])
        for lo, hi, val in zip(b[:-1], b[1:], v[1:-1]):
            if lo < s <= hi:
                return float(val)
        raise AssertionError("unreachable")
    if name == "PolynomialDecay":
        d = np.float64(c["decay_steps"])
        if c.get("cycle"):
            d = d * (1.0 if s == 0 else np.ceil(s / d))
        else:
            s = min(s, d)
        end = c.get("end_learning_rate", 1e-4)
        return float((c["initial_learning_rate"] - end) * np.power(1.0 - s / d, c.get("power", 1.0)) + end)
    if name == "InverseTimeDecay":
        p = s / c["decay_steps"]
        p = np.floor(p) if c.get("staircase") else p
        return float(c["initial_learning_rate"] / (1.0 + c["decay_rate"] * p))
    if name == "CosineDecay":
        d = np.float64(c["decay_steps"])
        a = c.get("alpha", 0.0)
        return float(c["initial_learning_rate"] * ((1 - a) * 0.5 * (1.0 + np.cos(np.pi * min(s, d) / d)) + a))
    if name == "CosineDecayRestarts":
        f = s / np.float64(c["first_decay_steps"])
        t, m, a = c.get("t_mul", 2.0), c.get("m_mul", 1.0), c.get("alpha", 0.0)
        if t == 1.0:
            i = np.floor(f)
            f = f - i
        else:
            i = np.floor(np.log(1.0 - f * (1.0 - t)) / np.log(t))
            f = (f - (1.0 - t ** i) / (1.0 - t)) / t ** i
        return float(c["initial_learning_rate"] * ((1 - a) * 0.5 * m ** i * (1.0 + np.cos(np.pi * f)) + a))
    raise KeyError(name)


def near_restart(c, s):
    """True at (or within 1e-9 of) the start of a period of CosineDecayRestarts with t_mul != 1, where floor(log/log)
    may land on either side."""
    t = c.get("t_mul", 2.0)
    if t == 1.0:
        return False
    x = np.log(1.0 - s / c["first_decay_steps"] * (1.0 - t)) / np.log(t)
    return abs(x - round(x)) < 1e-9


# one config per kind and flag (the GPU tests evaluate the same ones on the device)
CASES = {
    "exp": ("ExponentialDecay", dict(initial_learning_rate=0.1, decay_steps=100, decay_rate=0.96)),
    "exp_stair": ("ExponentialDecay", dict(initial_learning_rate=0.05, decay_steps=7, decay_rate=0.5, staircase=True)),
    "piecewise": ("PiecewiseConstantDecay", dict(boundaries=[10, 100, 1000, 5000], values=[1.0, 0.5, 0.1, 0.01, 0.001])),
    "poly": ("PolynomialDecay", dict(initial_learning_rate=0.1, decay_steps=1000, end_learning_rate=0.001, power=2.0)),
    "poly_cycle": ("PolynomialDecay", dict(initial_learning_rate=0.1, decay_steps=300, end_learning_rate=0.01, power=0.5,
                                           cycle=True)),
    "inv": ("InverseTimeDecay", dict(initial_learning_rate=0.1, decay_steps=50, decay_rate=0.5)),
    "inv_stair": ("InverseTimeDecay", dict(initial_learning_rate=0.1, decay_steps=50, decay_rate=0.5, staircase=True)),
    "cos": ("CosineDecay", dict(initial_learning_rate=0.1, decay_steps=5000, alpha=0.1)),
    "restarts1": ("CosineDecayRestarts", dict(initial_learning_rate=0.1, first_decay_steps=700, t_mul=1.0, m_mul=0.9,
                                              alpha=0.05)),
    "restarts2": ("CosineDecayRestarts", dict(initial_learning_rate=0.1, first_decay_steps=300, t_mul=2.0, m_mul=0.8)),
    "restarts15": ("CosineDecayRestarts", dict(initial_learning_rate=0.02, first_decay_steps=128, t_mul=1.5, m_mul=1.0,
                                               alpha=0.1)),
}


def make(which):
    name, c = CASES[which]
    return getattr(S, name)(**c)


def probe_steps(which):
    """Steps that exercise each schedule's edges."""
    name, c = CASES[which]
    steps = set(range(0, 40)) | {1 << 24, (1 << 24) + 1, 20_000}
    d = c.get("decay_steps", c.get("first_decay_steps"))
    if d:
        for k in range(1, 12):
            steps |= {k * d - 1, k * d, k * d + 1}
    for b in c.get("boundaries", []):
        steps |= {b - 1, b, b + 1}
    return sorted(s for s in steps if not (name == "CosineDecayRestarts" and near_restart(c, s)))


@pytest.mark.parametrize("which", list(CASES))
def test_schedule_matches_formula(which):
    name, c = CASES[which]
    sched = make(which)
    for s in probe_steps(which):
        got, want = sched(s), ref_lr(name, c, s)
        assert isinstance(got, float)
        assert math.isclose(got, want, rel_tol=1e-13, abs_tol=1e-300), (which, s, got, want)


def test_schedule_edges():
    e = S.ExponentialDecay(1.0, 10, 0.5, staircase=True)
    assert e(9) == 1.0 and e(10) == 0.5 and e(19) == 0.5 and e(20) == 0.25
    assert S.ExponentialDecay(1.0, 10, 0.5)(5) == pytest.approx(0.5 ** 0.5, rel=1e-15)
    p = S.PiecewiseConstantDecay([100, 200], [1.0, 0.5, 0.1])
    assert (p(100), p(101), p(200), p(201)) == (1.0, 0.5, 0.5, 0.1)
    poly = S.PolynomialDecay(1.0, 10, end_learning_rate=0.0, cycle=True)
    assert poly(0) == 1.0 and poly(10) == 0.0 and poly(11) == pytest.approx(1 - 11 / 20) and poly(20) == 0.0
    assert S.PolynomialDecay(1.0, 10, end_learning_rate=0.5)(50) == 0.5                   # no cycle: held at the end
    assert S.InverseTimeDecay(1.0, 10, 1.0, staircase=True)(19) == 0.5
    assert S.CosineDecay(1.0, 100, alpha=0.2)(100) == pytest.approx(0.2) and S.CosineDecay(1.0, 100)(1000) == 0.0
    r1 = S.CosineDecayRestarts(1.0, 10, t_mul=1.0, m_mul=0.5)
    assert r1(0) == 1.0 and r1(10) == 0.5 and r1(20) == 0.25 and r1(5) == pytest.approx(0.5)
    r2 = S.CosineDecayRestarts(1.0, 10, t_mul=2.0, m_mul=0.5)
    assert r2(15) == pytest.approx(0.5 * 0.5 * (1 + math.cos(math.pi * 0.25)))            # period 1: 20 steps from 10
    assert r2(0) == 1.0 and r2(5) == pytest.approx(0.5)


def test_constructor_defaults_and_validation():
    with pytest.raises(ValueError, match="1 less than"):
        S.PiecewiseConstantDecay([1, 2], [1.0, 0.5])
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([1], [1.0, 0.5, 0.1])
    with pytest.raises(TypeError):
        S.ExponentialDecay(0.1, 10)                                    # decay_rate has no default
    assert S.PolynomialDecay(0.1, 10).get_config() == {"initial_learning_rate": 0.1, "decay_steps": 10,
                                                        "end_learning_rate": 0.0001, "power": 1.0, "cycle": False,
                                                        "name": None}
    assert S.CosineDecayRestarts(0.1, 10).get_config() == {"initial_learning_rate": 0.1, "first_decay_steps": 10,
                                                            "t_mul": 2.0, "m_mul": 1.0, "alpha": 0.0, "name": None}
    assert S.CosineDecay(0.1, 10).get_config()["alpha"] == 0.0
    assert S.ExponentialDecay(0.1, 10, 0.9).get_config()["staircase"] is False
    assert S.InverseTimeDecay(0.1, 10, 0.9).get_config()["staircase"] is False
    assert issubclass(S.CosineDecay, S.LearningRateSchedule)


@pytest.mark.parametrize("which", list(CASES))
def test_config_round_trips(which):
    name, c = CASES[which]
    sched = make(which)
    cfg = sched.get_config()
    assert {k: v for k, v in cfg.items() if k in c} == c and cfg["name"] is None
    again = type(sched).from_config(cfg)
    assert again.get_config() == cfg
    ser = S.serialize(sched)
    assert ser == {"class_name": name, "config": cfg}
    back = S.deserialize(json.loads(json.dumps(ser)))                 # through JSON, as in a saved file
    assert type(back) is type(sched) and back.get_config() == json.loads(json.dumps(cfg))
    for s in (0, 3, 99, 100, 4321):
        assert back(s) == sched(s)
    with pytest.raises(ValueError, match="Unknown decay"):
        S.deserialize({"class_name": "NoSuchDecay", "config": {}})


def test_optimizers_take_a_schedule():
    sched = S.ExponentialDecay(0.1, 100, 0.5, staircase=True)
    for opt in (mt.optimizers.SGD(learning_rate=sched, momentum=0.9), mt.optimizers.SGD(lr=sched),
                mt.optimizers.Adam(learning_rate=sched), mt.optimizers.Adam(lr=sched, amsgrad=True)):
        assert opt.lr is sched
        assert opt.get_config()["learning_rate"] == {"class_name": "ExponentialDecay", "config": sched.get_config()}
        spec = opt.spec()
        assert spec.schedule is sched and spec.device_lr and spec.lr_descriptor.kind == 1
        json.dumps(opt.get_config())
    assert mt.optimizers.SGD(lr=0.05).get_config()["learning_rate"] == 0.05


def test_spec_configs_tell_schedules_apart():
    """Two different schedules never share a step plan; a rate read from the device descriptor is not part of the key."""
    scheds = [S.ExponentialDecay(0.1, 100, 0.5), S.ExponentialDecay(0.1, 100, 0.5, staircase=True),
              S.ExponentialDecay(0.1, 101, 0.5), S.InverseTimeDecay(0.1, 100, 0.5), S.CosineDecay(0.1, 100),
              S.CosineDecay(0.1, 100, alpha=0.1), S.CosineDecayRestarts(0.1, 100), S.PolynomialDecay(0.1, 100),
              S.PiecewiseConstantDecay([5], [0.1, 0.01]), S.PiecewiseConstantDecay([6], [0.1, 0.01])]
    configs = {mt.optimizers.SGD(lr=s, momentum=0.9, nesterov=True).spec().config for s in scheds}
    assert len(configs) == len(scheds)
    configs |= {mt.optimizers.Adam(lr=s).spec().config for s in scheds}
    assert len(configs) == 2 * len(scheds)
    same = [mt.optimizers.SGD(lr=S.CosineDecay(0.1, 100)).spec() for _ in range(2)]
    assert same[0] == same[1] and hash(same[0]) == hash(same[1])
    # a plain rate: the config of before; with device_lr the rate moves to the descriptor and out of the config
    sgd = mt.optimizers.SGD(lr=0.02, momentum=0.9, nesterov=True)
    assert sgd.spec().config == ("sgd", 0.02, 0.0, 0.9, True) and not sgd.spec().device_lr
    assert sgd.spec().lr_descriptor is None
    dev = sgd.spec(device_lr=True)
    assert dev.device_lr and dev.config != sgd.spec().config
    assert dev.lr_descriptor.kind == 0 and dev.lr_descriptor.initial == 0.02
    assert mt.optimizers.SGD(lr=0.5, momentum=0.9, nesterov=True).spec(device_lr=True) == dev
    assert OptimizerSpec("sgd", 0.01, 1e-6, 0.9, True).config == ("sgd", 0.01, 1e-6, 0.9, True)


def test_descriptor_fields():
    d = S.descriptor(S.PolynomialDecay(0.1, 300, end_learning_rate=0.01, power=0.5, cycle=True), decay=1e-3)
    assert (d.kind, d.flag, d.initial, d.decay_steps, d.end_learning_rate, d.power, d.decay) == \
        (3, 1, 0.1, 300.0, 0.01, 0.5, 1e-3)
    d = S.descriptor(S.CosineDecayRestarts(0.1, 70, t_mul=1.5, m_mul=0.9, alpha=0.05))
    assert (d.kind, d.decay_steps, d.t_mul, d.m_mul, d.alpha) == (6, 70.0, 1.5, 0.9, 0.05)
    d = S.descriptor(S.PiecewiseConstantDecay(list(range(1, 65)), [float(i) for i in range(65)]))
    assert d.kind == 2 and d.n_boundaries == 64 and d.boundaries[63] == 64.0 and d.values[64] == 64.0
    d = S.descriptor(0.25, 1e-6)
    assert (d.kind, d.initial, d.decay) == (0, 0.25, 1e-6)
    import ctypes
    assert ctypes.sizeof(_lib.LrSchedule) == 16 + 9 * 8 + (2 * _lib.LR_MAX_BOUNDARIES + 1) * 8


def test_custom_schedules_and_device_limits_are_refused():
    class WarmUp(S.LearningRateSchedule):
        def __call__(self, step):
            return 0.1 * min(1.0, step / 100)

        def get_config(self):
            return {}

    class MyExp(S.ExponentialDecay):                 # a subclass may change __call__: not the built-in formula either
        pass

    for cls in (WarmUp, MyExp):
        sched = cls() if cls is WarmUp else cls(0.1, 10, 0.5)
        for make_opt in (lambda: mt.optimizers.SGD(learning_rate=sched), lambda: mt.optimizers.SGD(lr=sched),
                         lambda: mt.optimizers.Adam(learning_rate=sched)):
            with pytest.raises(NotImplementedError, match=cls.__name__):
                make_opt()
    too_many = S.PiecewiseConstantDecay(list(range(65)), [0.1] * 66)
    with pytest.raises(ValueError, match="64"):
        mt.optimizers.SGD(lr=too_many)
    for bad in (S.ExponentialDecay(0.1, 0, 0.5), S.CosineDecay(0.1, -5), S.CosineDecayRestarts(0.1, 0),
                S.PolynomialDecay(0.1, 0), S.InverseTimeDecay(0.1, 0, 0.5)):
        with pytest.raises(ValueError, match="decay steps"):
            mt.optimizers.Adam(lr=bad)


# ---- Keras .h5 training_config ------------------------------------------------------------------------------------------
def _write(tmp_path, optimizer, name):
    params = glorot_numpy(seed=3)
    path = str(tmp_path / f"{name}.h5")
    keras_h5.save_model(path, params, 16, 32, 8, 35, optimizer=optimizer, iterations=0)
    return path


def _have_h5py():
    if not os.path.exists(H5PY_PYTHON):
        return False
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    return subprocess.run([H5PY_PYTHON, "-c", "import h5py"], env=env, capture_output=True).returncode == 0


@pytest.mark.parametrize("cls", ["SGD", "Adam"])
def test_keras_h5_round_trip_of_a_schedule(tmp_path, cls):
    sched = S.CosineDecayRestarts(0.01, 40, t_mul=1.5, m_mul=0.9, alpha=0.01)
    ser = S.serialize(sched)
    if cls == "Adam":
        opt = dict(class_name="Adam", lr=ser, decay=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False)
    else:
        opt = dict(lr=ser, decay=1e-4, momentum=0.9, nesterov=True)
    path = _write(tmp_path, opt, cls)
    from lisec_amd import hdf5_lite
    with hdf5_lite.File(path) as f:
        tc = json.loads(bytes(f.attrs["training_config"]).decode())["optimizer_config"]
    assert tc["class_name"] == cls and tc["config"]["learning_rate"] == ser and tc["config"]["decay"] == 1e-4
    ck = keras_h5.load_model(path)
    assert ck["optimizer"]["lr"] == ser
    back = S.deserialize(ck["optimizer"]["lr"])
    assert type(back) is S.CosineDecayRestarts and back.get_config() == sched.get_config()
    if not _have_h5py():
        return                                             # the hdf5_lite round trip above still ran; no h5py here
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    out = subprocess.run([H5PY_PYTHON, PROBE, "dump", path], env=env, capture_output=True, check=True).stdout
    desc = json.loads(out)
    tc = json.loads(desc["/"]["attrs"]["training_config"]["value"])["optimizer_config"]
    assert tc["class_name"] == cls and tc["config"]["learning_rate"] == ser


def test_float_rate_training_config_is_unchanged():
    """A number as learning rate: the training_config JSON of before, byte for byte."""
    sgd = keras_h5._training_config(dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True))
    assert json.dumps(sgd) == (
        '{"loss": ["mse", "mse"], "metrics": null, "weighted_metrics": null, "loss_weights": null, "optimizer_config": '
        '{"class_name": "SGD", "config": {"name": "SGD", "learning_rate": 0.01, "decay": 1e-06, "momentum": 0.9, '
        '"nesterov": true}}}')
    adam = keras_h5._training_config(dict(class_name="Adam", lr=0.002, decay=1e-5, beta_1=0.85, beta_2=0.995,
                                          epsilon=1e-6, amsgrad=True))
    assert json.dumps(adam) == (
        '{"loss": ["mse", "mse"], "metrics": null, "weighted_metrics": null, "loss_weights": null, "optimizer_config": '
        '{"class_name": "Adam", "config": {"name": "Adam", "learning_rate": 0.002, "decay": 1e-05, "beta_1": 0.85, '
        '"beta_2": 0.995, "epsilon": 1e-06, "amsgrad": true}}}')
    assert json.dumps(keras_h5._training_config(dict(lr=np.float32(0.5), decay=0, momentum=0, nesterov=False))) == \
        json.dumps(keras_h5._training_config(dict(lr=0.5, decay=0.0, momentum=0.0, nesterov=False)))


# ---- LearningRateScheduler on a mock model ------------------------------------------------------------------------------
class _Model:
    def __init__(self, lr):
        self.optimizer = mt.optimizers.SGD(lr=lr, momentum=0.9, nesterov=True)


def _run_epochs(cb, model, epochs):
    cb.set_model(model)
    seen = []
    for epoch in range(epochs):
        cb.on_epoch_begin(epoch, {})
        logs = {"loss": 1.0}
        cb.on_epoch_end(epoch, logs)
        seen.append(logs["lr"])
    return seen


def test_learning_rate_scheduler_arguments():
    cbs = mt.callbacks
    calls = []

    def two(epoch, lr):
        calls.append((epoch, lr))
        return lr * 0.5

    m = _Model(0.08)
    assert _run_epochs(cbs.LearningRateScheduler(two), m, 3) == [0.04, 0.02, 0.01]
    assert calls == [(0, 0.08), (1, 0.04), (2, 0.02)] and m.optimizer.lr == 0.01
    m = _Model(0.08)
    assert _run_epochs(cbs.LearningRateScheduler(lambda epoch: 0.1 / (1 + epoch)), m, 3) == [0.1, 0.05, 0.1 / 3]
    m = _Model(0.08)
    assert _run_epochs(cbs.LearningRateScheduler(lambda epoch, lr: np.float32(0.25)), m, 1) == [0.25]
    assert type(m.optimizer.lr) is float
    for bad in (lambda epoch, lr: 1, lambda epoch, lr: "0.1", lambda epoch, lr: None):
        m = _Model(0.08)
        cb = cbs.LearningRateScheduler(bad)
        cb.set_model(m)
        with pytest.raises(ValueError, match="should be float"):
            cb.on_epoch_begin(0, {})
        assert m.optimizer.lr == 0.08
    m = _Model(S.CosineDecay(0.1, 100))
    cb = cbs.LearningRateScheduler(lambda epoch, lr: lr)
    cb.set_model(m)
    with pytest.raises(ValueError, match="CosineDecay"):
        cb.on_epoch_begin(0, {})


def test_callback_base_class_hooks():
    cb = mt.callbacks.Callback()
    cb.set_model("m")
    cb.set_params({"epochs": 2})
    assert cb.model == "m" and cb.params == {"epochs": 2}
    for hook in (cb.on_train_begin, cb.on_train_end):
        hook()
        hook({})
    cb.on_epoch_begin(0)
    cb.on_epoch_end(0, {"loss": 1.0})
    assert "callbacks" in mt.Model.fit.__code__.co_varnames
