"""Decoupled weight decay without a GPU: the numpy definition (tests/weight_decay_ref.py) on the shared inputs, the
optimizer classes optimizers.AdamW / SGDW / extend_with_decoupled_weight_decay (constructors, refusals, configs, spec
configs), the chunk tables of ops.decay_chunks and the optimizer dict in the Keras .h5 checkpoints."""
import json

import numpy as np
import pytest

import weight_decay_ref as R
from lisec_amd import _lib, hdf5_lite, keras_h5, lr_schedules, ops
from lisec_amd import model_training as mt
from lisec_amd.network import DecaySpec, OptimizerSpec
from lisec_amd.params import TRAINABLE_KINDS, glorot_numpy, param_specs

F = np.float32
O = mt.optimizers
GRID = (16, 32, 8, 35)
BASES = ("SGD", "Adam", "RMSprop", "Adagrad", "Adadelta", "Adamax", "Nadam")
# the coefficients of the GPU tests (tests/test_gpu_weight_decay.py)
COEFFICIENTS = sorted({float(R.coefficient(wd, s)) for wd, counts in R.cases().values() for s in counts})


# ---- the definition --------------------------------------------------------------------------------------------------------
def test_the_definition_on_hand_cases():
    w = np.array([1.0, -2.0, 0.0, -0.0, 1e-41], F)
    got = R.step(w, 0.5)
    assert np.array_equal(R.bits(got), R.bits(np.array([0.5, -1.0, 0.0, 0.0, 5e-42], F)))     # (-0) - (-0) = +0
    assert np.array_equal(R.bits(R.step(w, 0.0)), R.bits(w))                                # 0 keeps the sign of -0
    one = np.array([1.0], F)
    assert R.step(one, F(1e-8))[0] == F(1.0) and R.step(one, F(1.0))[0] == F(0.0)
    assert R.coefficient(0.1, 5) == F(0.1)
    sched = lr_schedules.PiecewiseConstantDecay([3], [0.5, 0.25])
    assert [float(R.coefficient(sched, s)) for s in (0, 3, 4)] == [0.5, 0.5, 0.25]
    assert np.array_equal(R.steps(np.array([8.0], F), sched, range(2, 5)), np.array([8.0 * 0.5 * 0.5 * 0.75], F))


def test_the_inputs_are_not_vacuous():
    """The shared inputs hold +-0, denormals, large and small magnitudes, inf and NaN, and at every coefficient of the
    GPU tests they tell the definition from the forms the kernel must not compute: the fma and w*(1 - wd)."""
    tiny = np.finfo(F).tiny
    for n in (1020, 4100):
        w = R.make_inputs(n, R.SEED)
        assert (np.signbit(w) & (w == 0)).any() and ((w == 0) & ~np.signbit(w)).any()
        assert ((np.abs(w) < tiny) & (w != 0)).any()
        assert np.isposinf(w).any() and np.isneginf(w).any() and np.isnan(w).any()
        finite = w[np.isfinite(w)]
        assert (np.abs(finite) > 1e29).any() and ((np.abs(finite) < 1e-24) & (np.abs(finite) >= tiny)).any()
        for wd in COEFFICIENTS:
            want = R.step(w, wd)
            assert not R.same(want, w)
            assert not R.same(want, R.step_fma(w, wd)), wd
            assert not R.same(want, R.step_scaled(w, wd)), wd
            p = np.multiply(F(wd), finite, dtype=F)
            assert ((np.abs(p) < tiny) & (p != 0)).any()                    # a product that is a denormal
    assert len(COEFFICIENTS) == 6 and min(COEFFICIENTS) == float(F(0.01))
    assert R.make_inputs(0, 31).shape == (0,) and R.make_inputs(4, 31).shape == (4,)
    assert R.same(np.array([np.nan, 1.0], F), np.array([-np.nan, 1.0], F))
    assert not R.same(np.array([0.0], F), np.array([-0.0], F)) and not R.same(np.array([np.nan], F), np.array([1.0], F))


# ---- the optimizer classes ---------------------------------------------------------------------------------------------------
def test_constructors_and_defaults():
    a = O.AdamW(1e-4)
    assert (a.weight_decay, a.lr, a.beta_1, a.beta_2, a.epsilon, a.amsgrad, a.name, a.decay, a.decay_var_list) == (
        1e-4, 0.001, 0.9, 0.999, 1e-7, False, "AdamW", 0.0, None)
    assert a.record is O.Adam().record and isinstance(a, O.Adam)
    s = O.SGDW(0.01)
    assert (s.weight_decay, s.lr, s.momentum, s.nesterov, s.name, s.decay) == (0.01, 0.001, 0.0, False, "SGDW", 0.0)
    assert s.record is O.SGD().record and isinstance(s, O.SGD)
    # positional order of tfa: weight_decay, learning_rate, ...
    assert O.AdamW(0.1, 0.2, 0.3, 0.4, 0.5, True).get_config() == {
        "name": "AdamW", "learning_rate": 0.2, "decay": 0.0, "beta_1": 0.3, "beta_2": 0.4, "epsilon": 0.5, "amsgrad": True,
        "weight_decay": 0.1}
    assert O.SGDW(0.1, 0.2, 0.3, True).get_config() == {
        "name": "SGDW", "learning_rate": 0.2, "decay": 0.0, "momentum": 0.3, "nesterov": True, "weight_decay": 0.1}
    # lr= and decay= as in the base classes
    assert O.AdamW(0.1, lr=0.5, decay=1e-3).get_config()["learning_rate"] == 0.5
    assert O.AdamW(0.1, lr=0.5, decay=1e-3).decay == 1e-3 and O.SGDW(0.1, lr=0.5, decay=1e-3).lr == 0.5
    # schedules for either, independently
    sched = O.schedules.CosineDecay(1e-3, 100)
    b = O.AdamW(sched, learning_rate=O.schedules.ExponentialDecay(0.1, 10, 0.5), decay_var_list=["kernel", "cls.bias"])
    assert b.weight_decay is sched and b.decay_var_list == ["kernel", "cls.bias"]
    assert O.AdamW(0.1, decay_var_list="kernel").decay_var_list == ["kernel"]
    # a plain attribute that a callback may assign
    a.weight_decay = 0.5
    assert a.spec().weight_decay.descriptor.initial == 0.5 and a.get_config()["weight_decay"] == 0.5


def test_refusals():
    for bad in (-1e-4, float("nan"), float("inf"), 1e39, "much", None, True):
        for make in (O.AdamW, O.SGDW, lambda wd: DecaySpec(wd)):
            with pytest.raises(ValueError):
                make(bad)
    assert DecaySpec(float(np.finfo(F).max)).weight_decay == float(np.finfo(F).max)

    class Mine(lr_schedules.LearningRateSchedule):
        def __call__(self, step):
            return 0.1

        def get_config(self):
            return {}

    for make in (O.AdamW, O.SGDW, DecaySpec, O.extend_with_decoupled_weight_decay(O.RMSprop)):
        with pytest.raises(NotImplementedError):
            make(Mine())
    with pytest.raises(ValueError):                                      # past the device's limits
        O.AdamW(lr_schedules.PiecewiseConstantDecay(list(range(65)), [0.1] * 66))
    with pytest.raises(ValueError):
        O.AdamW(lr_schedules.CosineDecay(0.1, 0))
    for clip in ("clipnorm", "clipvalue", "global_clipnorm"):             # clipping is still refused
        for make in (O.AdamW, O.SGDW, O.extend_with_decoupled_weight_decay(O.Adagrad)):
            with pytest.raises(NotImplementedError):
                make(1e-4, **{clip: 1.0})
    with pytest.raises(TypeError):
        O.AdamW(1e-4, no_such_keyword=1)
    with pytest.raises(TypeError):
        O.AdamW()                                                        # weight_decay has no default, as in tfa
    with pytest.raises(ValueError):
        O.SGDW(0.1, momentum=1.5)                                        # the base class's own checks
    with pytest.raises(ValueError):
        O.AdamW(0.1, beta_1=1.0)
    with pytest.raises(ValueError):
        DecaySpec(0.1, variables=[3])
    with pytest.raises(ValueError):
        OptimizerSpec("adam", weight_decay=0.1)                          # a DecaySpec or None
    for bad in (O.MovingAverage, O.AdamW, int, "Adam", None):
        with pytest.raises(ValueError):
            O.extend_with_decoupled_weight_decay(bad)
    with pytest.raises(ValueError):
        O.deserialize({"class_name": "LambW", "config": {}})
    with pytest.raises(ValueError):
        O.deserialize({"class_name": "W", "config": {}})
    with pytest.raises(ValueError):
        O.get("adamw")                                                   # optimizers.get is unchanged


@pytest.mark.parametrize("base", BASES)
def test_extend_with_decoupled_weight_decay(base):
    cls = O.extend_with_decoupled_weight_decay(getattr(O, base))
    assert cls.__name__ == base + "W" and issubclass(cls, getattr(O, base))
    assert O.extend_with_decoupled_weight_decay(getattr(O, base)) is cls             # the same class at every call
    if base in ("SGD", "Adam"):
        assert cls is getattr(O, base + "W")
    plain, opt = getattr(O, base)(), cls(0.02, decay_var_list=["kernel"])
    assert opt.name == base + "W" and opt.weight_decay == 0.02 and opt.record is plain.record
    if base != "SGD":                                                    # (SGDW has tfa's default rate, not SGD's)
        assert {k: v for k, v in opt.get_config().items() if k not in ("name", "weight_decay", "decay_var_list")} == {
            k: v for k, v in plain.get_config().items() if k != "name"}
    assert list(opt.get_config())[-2:] == ["weight_decay", "decay_var_list"]
    spec = opt.spec()
    assert spec.slots == plain.spec().slots and spec.launch[0] == OptimizerSpec(
        spec.kind, opt.lr, opt.decay, **opt.hyper).launch[0]             # the base's kernels and slots
    assert spec.weight_decay == DecaySpec(0.5, ("kernel",)) and spec.weight_decay != DecaySpec(0.5)
    back = O.deserialize(O.serialize(opt))
    assert type(back) is cls and back.get_config() == opt.get_config()
    assert "decay_var_list" not in cls(0.02).get_config()


def test_config_round_trips():
    sched = O.schedules.PiecewiseConstantDecay([10, 20], [1e-3, 1e-4, 1e-5])
    cases = [O.AdamW(1e-4), O.AdamW(sched, learning_rate=O.schedules.CosineDecay(0.01, 50), amsgrad=True, name="mine"),
             O.SGDW(5e-4, learning_rate=0.1, momentum=0.9, nesterov=True, decay_var_list=["kernel", "rpn1.bn0.gamma"]),
             O.extend_with_decoupled_weight_decay(O.Nadam)(0.01, schedule_decay=0.01)]
    for opt in cases:
        ser = O.serialize(opt)
        assert ser["class_name"] == type(opt).__name__
        json.dumps(ser)                                                  # plain data
        back = O.deserialize(ser)
        assert type(back) is type(opt) and O.serialize(back) == ser
        assert back.spec() == opt.spec() and back.spec(device_lr=True) == opt.spec(device_lr=True)
        for wrap in (O.MovingAverage(opt, average_decay=0.9), O.SWA(opt, start_averaging=2, average_period=3)):
            wser = O.serialize(wrap)
            assert wser["config"]["optimizer"] == ser
            wback = O.deserialize(wser)
            assert O.serialize(wback) == wser and type(wback._optimizer) is type(opt)
            assert wback.spec() == wrap.spec() and wrap.spec().weight_decay == opt.spec().weight_decay
            assert wrap.spec().average is not None
    assert O.serialize(cases[1])["config"]["weight_decay"] == {"class_name": "PiecewiseConstantDecay",
                                                               "config": sched.get_config()}
    # through a wrapper the attribute reads and writes the wrapped optimizer's
    wrap = O.MovingAverage(O.AdamW(1e-4))
    wrap.weight_decay = 2e-4
    assert wrap._optimizer.weight_decay == 2e-4 and wrap.weight_decay == 2e-4
    assert wrap.spec().weight_decay.descriptor.initial == 2e-4


def test_spec_config_joins_only_when_set():
    for base, kw in (("SGD", dict(momentum=0.9)), ("Adam", {}), ("RMSprop", dict(centered=True)), ("Nadam", {})):
        plain = getattr(O, base)(learning_rate=0.001, **kw)
        cls = O.extend_with_decoupled_weight_decay(getattr(O, base))
        for device_lr in (False, True):
            want = plain.spec(device_lr).config
            assert OptimizerSpec(plain.record.kind, plain.lr, plain.decay, device_lr=device_lr, **plain.hyper).config == want
            zero = cls(0.0, learning_rate=0.001, **kw).spec(device_lr)      # the constant 0: no decay at all
            assert zero.config == want and zero.weight_decay is None and zero == plain.spec(device_lr)
            some = cls(1e-4, learning_rate=0.001, **kw).spec(device_lr)
            assert some.config == want + (("weight_decay", ("device",), None),)
            assert some != plain.spec(device_lr) and hash(some) == hash(cls(0.5, learning_rate=0.001, **kw).spec(device_lr))
    # a number is data of the step; the variables and a schedule are part of its launches
    a, b = O.AdamW(1e-4).spec(), O.AdamW(0.5).spec()
    assert a == b and bytes(a.weight_decay.descriptor) != bytes(b.weight_decay.descriptor)
    assert O.AdamW(1e-4, decay_var_list=["kernel"]).spec() != a
    assert O.AdamW(1e-4, decay_var_list=["kernel"]).spec().config[-1] == ("weight_decay", ("device",), ("kernel",))
    s1, s2 = O.schedules.CosineDecay(1e-3, 100), O.schedules.CosineDecay(1e-3, 200)
    assert O.AdamW(s1).spec() != O.AdamW(s2).spec() and O.AdamW(s1).spec() == O.AdamW(O.schedules.CosineDecay(1e-3, 100)).spec()
    assert O.AdamW(s1).spec().config[-1][1][0] == "schedule"
    assert O.AdamW(O.schedules.CosineDecay(0.0, 100)).spec().weight_decay is not None      # only the NUMBER 0 is no decay
    both = O.MovingAverage(O.AdamW(1e-4)).spec().config
    assert both[-2][0] == "average" and both[-1][0] == "weight_decay"
    d = O.AdamW(O.schedules.ExponentialDecay(0.1, 10, 0.5, staircase=True)).spec().weight_decay.descriptor
    assert (d.kind, d.flag, d.initial, d.decay_steps, d.decay_rate, d.decay) == (1, 1, 0.1, 10.0, 0.5, 0.0)


# ---- the chunk tables ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    import torch
    from lisec_amd.params import ParamStore
    return ParamStore(torch.device("cpu"))


def _spans(store):
    return {n: (o, o + (int(np.prod(s)) + 3) // 4 * 4) for n, (w, o, s) in store.offsets.items() if w == "theta"}


@pytest.mark.parametrize("names", [None, ("kernel",), ("bias", "gamma", "beta"), ("cls.bias", "rpn2.conv3.kernel", "vfe1.bn.beta"),
                                   ("gamma", "up3.kernel", "mid1.bn.gamma")])
def test_decay_chunks(store, names):
    rows = ops.decay_chunks(store, names)
    spans = _spans(store)
    kind_of = {n: k for n, _, k in store.specs}
    if names is None:
        want = set(spans)
    else:
        want = {n for n in spans if n in names or kind_of[n] in names}
    offs = [r[0] for r in rows]
    assert offs == sorted(offs) and len(set(offs)) == len(offs)                      # ascending
    covered = {n: [] for n in want}
    for off, count in rows:
        assert off % 4 == 0 and count % 4 == 0 and 0 < count <= _lib.REG_CHUNK
        owner = [n for n, (a, b) in spans.items() if a <= off < b]
        assert len(owner) == 1 and owner[0] in want                                  # only the decayed variables
        assert off + count <= spans[owner[0]][1]                                     # no chunk crosses a variable
        covered[owner[0]].append((off, count))
    for n in want:                                                                   # each one whole, over its padded length
        at = spans[n][0]
        for off, count in covered[n]:
            assert off == at
            at += count
        assert at == spans[n][1] and len(covered[n]) == -(-(spans[n][1] - spans[n][0]) // _lib.REG_CHUNK)
    if names is None:
        assert sum(c for _, c in rows) == store.n_theta
    assert ops.decay_chunks(store, list(names) if names else None) == rows
    table = ops.decay_table(rows, "cpu")
    import ctypes
    assert table.numel() == len(rows) * ctypes.sizeof(_lib.DecayChunk) and ctypes.sizeof(_lib.DecayChunk) == 16
    back = np.frombuffer(table.numpy().tobytes(), dtype=np.dtype([("offset", "<i8"), ("count", "<i4"), ("reserved", "<i4")]))
    assert [(int(r["offset"]), int(r["count"])) for r in back] == rows and not back["reserved"].any()


def test_decay_chunks_refusals_and_empty(store):
    assert ops.decay_chunks(store, ()) == []
    assert ops.decay_chunks(store, "cls.bias") == ops.decay_chunks(store, ["cls.bias", "cls.bias"])      # named twice: once
    with pytest.raises(KeyError):
        ops.decay_chunks(store, ["no.such.kernel"])
    for moving in ("mid1.bn.moving_mean", "rpn1.bn0.moving_variance"):               # the moving statistics are not trained
        with pytest.raises(ValueError):
            ops.decay_chunks(store, ["kernel", moving])
    with pytest.raises(KeyError):
        ops.decay_chunks(store, ["moving_mean"])                                     # not a kind of trainable variable


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
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


def _optimizer_dict(opt):
    """What Model.save hands keras_h5.save_model for `opt`."""
    d = opt.record.as_dict(mt._serialize_rate(opt.lr), opt.decay, opt.hyper)
    d.update(class_name=type(opt).__name__, weight_decay=mt._serialize_rate(opt.weight_decay))
    if opt.decay_var_list is not None:
        d["decay_var_list"] = list(opt.decay_var_list)
    return d


@pytest.mark.parametrize("which", ["AdamW", "SGDW", "RMSpropW"])
def test_h5_round_trip_of_the_optimizer_dict(tmp_path, which):
    params = glorot_numpy(seed=3)
    sched = O.schedules.CosineDecay(1e-3, 40, alpha=0.1)
    if which == "AdamW":
        opt, slots = O.AdamW(sched, learning_rate=0.002, decay_var_list=["kernel"]), ("m", "v")
    elif which == "SGDW":
        opt, slots = O.SGDW(5e-4, learning_rate=0.02, momentum=0.9), ("velocity",)
    else:
        opt, slots = O.extend_with_decoupled_weight_decay(O.RMSprop)(0.25), ("rms",)
    given = {s: _arrays(params, 1 + i) for i, s in enumerate(slots)}
    d = _optimizer_dict(opt)
    path = str(tmp_path / "wd.h5")
    keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=7, **given)
    assert _training_config(path)["optimizer_config"] == O.serialize(opt)            # the class and its whole config
    with hdf5_lite.File(path) as f:
        names = [bytes(n).decode() for n in np.asarray(f["optimizer_weights"].attrs["weight_names"]).ravel()]
    assert all(n.startswith(which + "/") for n in names) and names[0] == which + "/iter:0"
    nv = len(_trainable())
    kinds = [n.rsplit("/", 1)[1] for n in names]
    base_kinds = [s.kind for s in opt.record.active_slots(opt.hyper)]                # the base optimizer's slot kinds
    assert kinds == ["iter:0"] + [k + ":0" for k in base_kinds for _ in range(nv)]
    ck = keras_h5.load_model(path)
    assert ck["iterations"] == 7 and ck["wrapper"] is None and ck["optimizer"] == d
    for s in slots:
        for n in _trainable():
            assert np.array_equal(R.bits(ck[s][n]), R.bits(given[s][n])), (s, n)
    back = O.deserialize(_training_config(path)["optimizer_config"])
    assert type(back) is type(opt) and back.get_config() == opt.get_config()
    # nested under an averaging wrapper
    wrap = O.MovingAverage(opt, average_decay=0.9)
    own = {k: v for k, v in wrap.get_config().items() if k != "optimizer"}
    keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=3, wrapper={"class_name": "MovingAverage", "config": own},
                        average=_arrays(params, 9), **given)
    assert _training_config(path)["optimizer_config"] == O.serialize(wrap)
    ck = keras_h5.load_model(path)
    assert ck["optimizer"] == d and ck["wrapper"]["class_name"] == "MovingAverage" and ck["average"] is not None


def test_h5_of_an_optimizer_without_decay_keeps_its_bytes(tmp_path):
    """A file of a base optimizer is byte for byte what it was: the record of <Base>W is <Base>'s, and only a dict that
    names the W class gains keys."""
    params = glorot_numpy(seed=3)
    m, v = _arrays(params, 1), _arrays(params, 2)
    plain = dict(class_name="Adam", lr=0.002, decay=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False)
    a, b = str(tmp_path / "a.h5"), str(tmp_path / "b.h5")
    keras_h5.save_model(a, params, *GRID, optimizer=plain, iterations=7, m=m, v=v)
    keras_h5.save_model(b, params, *GRID, optimizer=dict(plain, class_name="AdamW", weight_decay=0.0), iterations=7, m=m, v=v)
    assert _file_bytes(a) != _file_bytes(b)
    assert "weight_decay" not in _training_config(a)["optimizer_config"]["config"]
    assert keras_h5.load_model(a)["optimizer"] == plain
    assert json.dumps(keras_h5._training_config(dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True))) == (
        '{"loss": ["mse", "mse"], "metrics": null, "weighted_metrics": null, "loss_weights": null, "optimizer_config": '
        '{"class_name": "SGD", "config": {"name": "SGD", "learning_rate": 0.01, "decay": 1e-06, "momentum": 0.9, '
        '"nesterov": true}}}')
    assert json.dumps(keras_h5._training_config(plain)["optimizer_config"]) == (
        '{"class_name": "Adam", "config": {"name": "Adam", "learning_rate": 0.002, "decay": 0.0, "beta_1": 0.9, '
        '"beta_2": 0.999, "epsilon": 1e-07, "amsgrad": false}}')
    # a class that is neither in the table nor a <Base>W is written as SGD, as it always was
    assert keras_h5._training_config(dict(class_name="LambW", lr=0.1))["optimizer_config"]["class_name"] == "SGD"
    assert keras_h5.written_class(dict(class_name="SGDW")) == "SGDW" and keras_h5.written_class({}) == "SGD"
