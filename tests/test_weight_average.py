"""Weight averaging without a GPU: the numpy definition (tests/weight_average_ref.py) on hand cases, the optimizer
wrappers optimizers.MovingAverage / optimizers.SWA (configs, write-through, refusals, spec configs) and the `average`
slot and nested optimizer config in the Keras .h5 and the .npz checkpoints."""
import json

import numpy as np
import pytest

import weight_average_ref as R
from lisec_amd import hdf5_lite, keras_h5
from lisec_amd import model_training as mt
from lisec_amd.network import AverageSpec, OptimizerSpec
from lisec_amd.params import TRAINABLE_KINDS, glorot_numpy, param_specs

F = np.float32
O = mt.optimizers
GRID = (16, 32, 8, 35)


# ---- the definition on hand cases ---------------------------------------------------------------------------------------
def test_c_equal_one_is_a_store():
    """decay_s = 0 (before start_step, or average_decay = 0): a <- w, where the arithmetic form gives 0 for w = 1."""
    a, w = np.array([1e8], F), np.array([1.0], F)
    assert R.ema_coefficient(3, 0.99, start_step=5) == F(1.0)
    assert R.ema_step(a, w, 3, 0.99, start_step=5)[0] == F(1.0)
    assert R.ema_step(a, w, 0, 0.0)[0] == F(1.0)
    arithmetic = a - (a - w) * F(1.0)
    assert arithmetic[0] == F(0.0)                       # 1e8 - 1 rounds to 1e8 in fp32: the store is not a detail


def test_ema_is_three_separately_rounded_operations():
    a, w = np.array([1.0, -2.5, 3e-3], F), np.array([0.5, -2.25, 1.0], F)
    c = F(1.0 - 0.99)
    want = a - ((a - w) * c).astype(F)
    got = R.ema_step(a, w, 100, 0.99)
    assert got.dtype == F and np.array_equal(R.bits(got), R.bits(want))
    assert c == R.ema_coefficient(100, 0.99) and float(c) != 1.0 - 0.99      # rounded once, from the double


def test_dynamic_decay_ramp():
    """min(0.99, (1 + k)/(10 + k)): 0.1, 2/11, ... reaches 0.99 at k = 890 ((1 + k)/(10 + k) >= 0.99 <=> k >= 890)."""
    for k, want in ((0, 0.1), (1, 2 / 11), (89, 90 / 99), (90, 91 / 100), (889, 890 / 899), (890, 0.99), (5000, 0.99)):
        assert R.ema_decay(k, 0.99, dynamic_decay=True) == want
        assert R.ema_decay(k + 7, 0.99, start_step=7, dynamic_decay=True) == want       # k counts from start_step
        assert R.ema_coefficient(k, 0.99, dynamic_decay=True) == F(1.0 - want)
    assert R.ema_decay(6, 0.99, start_step=7, dynamic_decay=True) == 0.0
    assert R.ema_decay(0, 0.05, dynamic_decay=True) == 0.05                               # the cap is average_decay


def test_swa_snapshots():
    start, period = 4, 3
    got = [R.swa_m(s, start, period) for s in range(12)]
    assert got == [-1, -1, -1, -1, 0, -1, -1, 1, -1, -1, 2, -1]
    a, w = np.array([2.0, 1.0], F), np.array([4.0, 0.0], F)
    for s in (0, 3, 5, 6, 8):
        assert np.array_equal(R.bits(R.swa_step(a, w, s, start, period)), R.bits(a))      # keeps its bits
    assert np.array_equal(R.swa_step(a, w, 4, start, period), w)                           # m = 0: a <- w
    assert np.array_equal(R.swa_step(a, w, 7, start, period), np.array([3.0, 0.5], F))    # m = 1: (a + w)/2
    got = R.swa_step(a, w, 10, start, period)                                               # m = 2: (2a + w)/3
    assert np.array_equal(R.bits(got), R.bits(((a * F(2) + w) / F(3)).astype(F)))
    assert [R.swa_m(s, 0, 1) for s in range(4)] == [0, 1, 2, 3]


def test_num_updates_folds_into_average_decay():
    assert R.fold_num_updates(0.99, None) == 0.99
    assert R.fold_num_updates(0.99, 0) == 0.1
    assert R.fold_num_updates(0.99, 90) == 91 / 100
    assert R.fold_num_updates(0.5, 90) == 0.5
    for nu in (None, 0, 5, 90, 10_000):
        assert O.MovingAverage("sgd", average_decay=0.99, num_updates=nu).average_spec().decay == R.fold_num_updates(0.99, nu)


def test_the_forbidden_forms_differ_on_the_test_inputs():
    """What tests/test_gpu_weight_average.py relies on: its inputs tell the definition from an fma, from the
    distributed form a*(1 - c) + w*c and from a reciprocal multiply.  The mirrored spelling a + (w - a)*c is the SAME
    function bit for bit (rounding to nearest is symmetric under negation), so no input can tell it apart."""
    a, w = R.make_inputs(4100, 20)
    c = R.ema_coefficient(50, 0.9)
    want = R.ema_step(a, w, 50, 0.9)
    assert not np.array_equal(R.bits(want), R.bits(R.ema_step_fma(a, w, c)))
    assert not np.array_equal(R.bits(want), R.bits(R.ema_step_reassociated(a, w, c)))
    assert np.array_equal(R.bits(want), R.bits(R.ema_step_mirrored(a, w, c)))
    # m = 2 divides by 3; at m = 3 the divisor is 4, whose reciprocal is exact, and the two forms agree on every input
    assert not np.array_equal(R.bits(R.swa_step(a, w, 4, 0, 2)), R.bits(R.swa_step_reciprocal(a, w, 2)))
    assert np.array_equal(R.bits(R.swa_step(a, w, 6, 0, 2)), R.bits(R.swa_step_reciprocal(a, w, 3)))


# ---- the wrappers ----------------------------------------------------------------------------------------------------------
def test_config_round_trip():
    sched = O.schedules.ExponentialDecay(0.01, 100, 0.5)
    for opt in (O.MovingAverage(O.SGD(lr=0.1, momentum=0.9, nesterov=True), average_decay=0.95, num_updates=7, start_step=3,
                                dynamic_decay=True, name="ema"),
                O.MovingAverage("adam"),
                O.SWA(O.Adam(learning_rate=sched, amsgrad=True), start_averaging=5, average_period=2),
                O.SWA(O.Nadam(schedule_decay=0.01)), O.SWA("sgd")):
        ser = O.serialize(opt)
        assert ser["class_name"] == type(opt).__name__
        nested = ser["config"]["optimizer"]
        assert nested == {"class_name": type(opt._optimizer).__name__, "config": opt._optimizer.get_config()}
        json.dumps(ser)                                    # plain JSON
        back = O.deserialize(json.loads(json.dumps(ser)))
        assert type(back) is type(opt) and back.get_config() == opt.get_config()
        assert back.spec() == opt.spec() and back.spec(device_lr=True) == opt.spec(device_lr=True)
    cfg = O.MovingAverage("sgd").get_config()
    assert list(cfg) == ["name", "optimizer", "sequential_update", "average_decay", "num_updates", "start_step",
                         "dynamic_decay"]
    assert (cfg["average_decay"], cfg["num_updates"], cfg["start_step"], cfg["dynamic_decay"]) == (0.99, None, 0, False)
    assert list(O.SWA("sgd").get_config()) == ["name", "optimizer", "start_averaging", "average_period"]
    assert O.SWA("sgd").get_config()["average_period"] == 10
    with pytest.raises(ValueError, match="Lookahead"):
        O.deserialize({"class_name": "Lookahead", "config": {}})
    assert O.get(opt) is opt                               # compile() takes a wrapper as it is


def test_hyper_parameters_write_through():
    inner = O.SGD(lr=0.1, decay=1e-3, momentum=0.9)
    opt = O.MovingAverage(inner)
    assert (opt.lr, opt.decay, opt.momentum, opt.nesterov) == (0.1, 1e-3, 0.9, False)
    opt.lr = 0.05                                          # what ReduceLROnPlateau / LearningRateScheduler do
    opt.momentum = 0.5
    assert inner.lr == 0.05 and inner.momentum == 0.5 and opt.spec().lr == 0.05 and opt.spec().momentum == 0.5
    inner.lr = 0.025
    assert opt.lr == 0.025 and float(opt.lr) == 0.025
    assert opt.record is inner.record and opt.hyper == inner.hyper
    opt.average_decay = 0.5                                # its own attributes stay its own
    assert not hasattr(inner, "average_decay") and opt.average_spec().decay == 0.5
    swa = O.SWA(O.Adam(learning_rate=1e-3))
    swa.lr = 2e-3
    assert swa._optimizer.lr == 2e-3 and swa.beta_1 == 0.9
    with pytest.raises(AttributeError):
        opt.no_such_attribute


def test_refusals():
    with pytest.raises(ValueError, match="wrap"):
        O.MovingAverage(O.SWA("sgd"))
    with pytest.raises(ValueError, match="wrap"):
        O.SWA(O.MovingAverage("sgd"))
    with pytest.raises(ValueError, match="sequential_update"):
        O.MovingAverage("sgd", sequential_update=False)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="average_decay"):
            O.MovingAverage("sgd", average_decay=bad)
    O.MovingAverage("sgd", average_decay=0.0)
    O.MovingAverage("sgd", average_decay=1.0)
    with pytest.raises(ValueError):
        O.MovingAverage("sgd", start_step=-1)
    with pytest.raises(ValueError):
        O.SWA("sgd", start_averaging=-1)
    with pytest.raises(ValueError, match="average_period"):
        O.SWA("sgd", average_period=0)
    for kw in (dict(start_averaging=1.5), dict(average_period=2.0), dict(average_period=True)):
        with pytest.raises(ValueError, match="integer"):
            O.SWA("sgd", **kw)
    for kw in (dict(start_step=0.5), dict(num_updates=1.0), dict(start_step="3")):
        with pytest.raises(ValueError, match="integer"):
            O.MovingAverage("sgd", **kw)
    with pytest.raises(ValueError):
        O.MovingAverage("rmsprop")                         # the strings are 'sgd' and 'adam', as for compile()
    with pytest.raises(ValueError):
        O.MovingAverage(None)
    with pytest.raises(ValueError):                        # the wrapped optimizer's own checks still run
        O.MovingAverage(O.Adam(beta_1=1.5))
    O.SWA("sgd", start_averaging=np.int64(3), average_period=np.int32(2))


def test_spec_config_joins_only_when_set():
    plain = O.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)
    assert plain.spec().config == ("sgd", 0.01, 1e-6, 0.9, True)                # the tuple it always was
    assert OptimizerSpec().config == ("sgd", 0.01, 1e-6, 0.9, True) and OptimizerSpec().average is None
    assert O.Adam().spec(device_lr=True).config == ("adam", ("device",), 0.0, 0.9, 0.999, 1e-7, False)
    ema = O.MovingAverage(plain, average_decay=0.9).spec()
    assert ema.config[:5] == plain.spec().config and ema.config != plain.spec().config and ema != plain.spec()
    assert ema.config[5] == ("average", "ema", 0.9, False, 0)
    swa = O.SWA(plain, start_averaging=2, average_period=3).spec()
    assert swa.config[5] == ("average", "swa", 2, 3) and swa != ema
    assert O.MovingAverage(plain, average_decay=0.9).spec() == ema and hash(O.MovingAverage(plain, average_decay=0.9).spec()) == hash(ema)
    assert O.MovingAverage(plain, average_decay=0.9, dynamic_decay=True).spec() != ema
    assert ema.slots == plain.spec().slots and ema.launch == plain.spec().launch  # the update itself is the wrapped one's
    d = ema.average.descriptor
    assert (d.kind, d.dynamic, d.start, d.decay) == (0, 0, 0, 0.9)
    with pytest.raises(ValueError):
        AverageSpec("ema", decay=2.0)
    with pytest.raises(ValueError):
        OptimizerSpec(average="ema")


def test_average_weights_needs_a_wrapper():
    class _Net:
        swaps = 0

        def swap_average(self):
            self.swaps += 1

    m = mt.Model.__new__(mt.Model)
    m.net, m.optimizer = _Net(), O.SGD()
    with pytest.raises(ValueError, match="MovingAverage"):
        with m.average_weights():
            pass
    assert m.net.swaps == 0
    m.optimizer = O.SWA("sgd")
    with pytest.raises(KeyError):                           # swapped back on an exception too
        with m.average_weights():
            assert m.net.swaps == 1
            raise KeyError("x")
    assert m.net.swaps == 2
    with pytest.raises(ValueError):
        O.SWA("sgd").swap_weights(mt.Model.__new__(mt.Model))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def _trainable():
    return [n for n, _, k in param_specs() if k in TRAINABLE_KINDS]


def _arrays(params, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.standard_normal(params[n].shape).astype(F) for n in _trainable()}


def _training_config(path):
    with hdf5_lite.File(path) as f:
        return json.loads(bytes(f.attrs["training_config"]).decode())


def _file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("cls", ["MovingAverage", "SWA"])
def test_h5_round_trip_of_the_average_and_the_nested_config(tmp_path, cls):
    params = glorot_numpy(seed=3)
    velocity, average = _arrays(params, 1), _arrays(params, 2)
    opt = O.MovingAverage(O.SGD(lr=0.02, decay=1e-4, momentum=0.9), average_decay=0.9, dynamic_decay=True, start_step=2) \
        if cls == "MovingAverage" else O.SWA(O.SGD(lr=0.02, decay=1e-4, momentum=0.9), start_averaging=1, average_period=2)
    own = {k: v for k, v in opt.get_config().items() if k != "optimizer"}
    inner = dict(lr=0.02, decay=1e-4, momentum=0.9, nesterov=False)
    path = str(tmp_path / "avg.h5")
    keras_h5.save_model(path, params, *GRID, optimizer=inner, iterations=7, velocity=velocity,
                        wrapper={"class_name": cls, "config": own}, average=average)
    oc = _training_config(path)["optimizer_config"]
    assert oc == O.serialize(opt)                          # the wrapper's class and nested config
    with hdf5_lite.File(path) as f:
        names = [bytes(n).decode() for n in np.asarray(f["optimizer_weights"].attrs["weight_names"]).ravel()]
    kinds = [n.rsplit("/", 1)[1] for n in names]
    nv = len(_trainable())
    assert kinds == ["iter:0"] + ["momentum:0"] * nv + ["average:0"] * nv         # behind the wrapped optimizer's kinds
    assert all(n.startswith(cls + "/") for n in names[1 + nv:]) and all(n.startswith("SGD/") for n in names[:1 + nv])
    ck = keras_h5.load_model(path)
    assert ck["iterations"] == 7 and ck["wrapper"] == {"class_name": cls, "config": own}
    assert ck["optimizer"] == inner
    for n in _trainable():
        assert np.array_equal(R.bits(ck["average"][n]), R.bits(average[n])), n
        assert np.array_equal(R.bits(ck["velocity"][n]), R.bits(velocity[n])), n
    back = getattr(O, ck["wrapper"]["class_name"])(O.SGD(**{**inner, "lr": inner["lr"]}), **ck["wrapper"]["config"])
    assert back.get_config() == opt.get_config()


def test_h5_without_a_wrapper_keeps_its_bytes(tmp_path):
    params = glorot_numpy(seed=3)
    velocity = _arrays(params, 1)
    inner = dict(lr=0.02, decay=1e-4, momentum=0.9, nesterov=False)
    a, b = str(tmp_path / "a.h5"), str(tmp_path / "b.h5")
    keras_h5.save_model(a, params, *GRID, optimizer=inner, iterations=7, velocity=velocity)
    keras_h5.save_model(b, params, *GRID, optimizer=inner, iterations=7, velocity=velocity, wrapper=None, average=None)
    assert _file_bytes(a) == _file_bytes(b)
    ck = keras_h5.load_model(a)
    assert ck["wrapper"] is None and ck["average"] is None
    assert json.dumps(keras_h5._training_config(dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True))) == (
        '{"loss": ["mse", "mse"], "metrics": null, "weighted_metrics": null, "loss_weights": null, "optimizer_config": '
        '{"class_name": "SGD", "config": {"name": "SGD", "learning_rate": 0.01, "decay": 1e-06, "momentum": 0.9, '
        '"nesterov": true}}}')


def test_h5_unknown_wrapper_is_refused_by_name(tmp_path):
    params = glorot_numpy(seed=3)
    inner = dict(lr=0.02, decay=0.0, momentum=0.0, nesterov=False)
    with pytest.raises(ValueError, match="Lookahead"):
        keras_h5.save_model(str(tmp_path / "x.h5"), params, *GRID, optimizer=inner,
                            wrapper={"class_name": "Lookahead", "config": {}})
    good, bad = str(tmp_path / "good.h5"), str(tmp_path / "bad.h5")
    keras_h5.save_model(good, params, *GRID, optimizer=inner,
                        wrapper={"class_name": "SWA", "config": {"name": "SWA", "start_averaging": 0, "average_period": 10}})
    tc = _training_config(good)
    tc["optimizer_config"]["class_name"] = "Lookahead"
    keras_h5.save_model(bad, params, *GRID)
    with hdf5_lite.File(good) as f:
        mc = bytes(f.attrs["model_config"])
    # the same file with the wrapper's class renamed: written group by group, as tests/test_regularizers.py rewrites one
    ck = keras_h5.load_model(good)
    with hdf5_lite.File(bad, "w") as f:
        f.attrs["model_config"] = mc
        f.attrs["training_config"] = json.dumps(tc).encode()
        g = f.create_group("model_weights")
        layers, _ = keras_h5.keras_layers(*GRID)
        g.attrs["layer_names"] = [L["name"].encode() for L in layers]
        for L in layers:
            lg = g.create_group(L["name"])
            lg.attrs["weight_names"] = [f"{L['name']}/{w}:0".encode() for w, _ in L["weights"]]
            for w, pname in L["weights"]:
                lg.create_dataset(f"{L['name']}/{w}:0", data=ck["params"][pname])
    with pytest.raises(ValueError, match="Lookahead"):
        keras_h5.load_model(bad)


def test_npz_round_trip_of_the_average_and_the_nested_config(tmp_path):
    params = glorot_numpy(seed=3)
    average = _arrays(params, 2)
    opt = O.MovingAverage(O.Adam(learning_rate=2e-3), average_decay=0.8, start_step=1)
    meta = dict(format="lisec_amd-npz-1", nx=16, ny=32, nz=8, maxPoints=35, iterations=5, optimizer=O.serialize(opt))
    path = str(tmp_path / "avg.npz")
    mt._npz_write(path, meta, params, average)
    meta2, params2, average2 = mt._npz_read(path)
    assert meta2 == meta and sorted(params2) == sorted(params) and sorted(average2) == sorted(average)
    for n in average:
        assert np.array_equal(R.bits(average2[n]), R.bits(average[n])), n
    back = O.deserialize(meta2["optimizer"])
    assert type(back) is O.MovingAverage and back.get_config() == opt.get_config()
    # without a wrapper: the archive's entries are those it always had
    plain = str(tmp_path / "plain.npz")
    del meta["optimizer"]
    mt._npz_write(plain, meta, params)
    assert sorted(np.load(plain).files) == sorted(["__meta__", *params])
    assert mt._npz_read(plain)[2] == {}
