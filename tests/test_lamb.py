"""LAMB without a GPU: the numpy definition (tests/lamb_ref.py) on hand cases, the tables of ops.lamb_chunks, the
optimizer class optimizers.LAMB (defaults, configs, refusals, wrappers), the spec configs of every optimizer kind and the
optimizer dict in the Keras .h5 checkpoints."""
import ctypes
import json

import numpy as np
import pytest

import lamb_ref as R
from lisec_amd import _lib, hdf5_lite, keras_h5, ops, optimizer_table
from lisec_amd import model_training as mt
from lisec_amd.network import AverageSpec, DecaySpec, OptimizerSpec
from lisec_amd.params import TRAINABLE_KINDS, glorot_numpy, param_specs

F = np.float32
O = mt.optimizers
GRID = (16, 32, 8, 35)


# ---- the definition --------------------------------------------------------------------------------------------------------
def test_the_definition_on_hand_cases():
    w = np.array([3.0, 4.0, 0.0, 0.0, 1.0, 1.0, 2.0, 2.0])
    g = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, -1.0])
    z = np.zeros(8)
    variables = [(0, 2, True, True), (2, 2, True, True), (4, 2, True, True), (6, 2, False, False)]
    th, m, v, r = R.step(w, z, z, g, variables, 0, lr=0.1, epsilon=1e-12)
    # the first step of Adam has u = sign(g): ||w|| = 5, ||u|| = sqrt(2)
    assert np.allclose(m, 0.1 * g) and np.allclose(v, 0.001 * g * g)
    assert np.isclose(r[0], 5 / np.sqrt(2)) and np.allclose(th[:2], w[:2] - 0.1 * r[0])
    assert r[1] == 1.0 and np.allclose(th[2:4], -0.1)                 # ||w|| = 0: r = 1, the plain Adam step
    assert r[2] == 1.0 and np.array_equal(th[4:6], w[4:6])             # u = 0: r = 1, nothing moves
    assert r[3] == 1.0 and np.allclose(th[6:], w[6:] - 0.1 * g[6:])    # not adapted: r = 1
    # the decay is inside u, only where the variable is decayed, and changes the ratio
    th, _, _, r = R.step(w, z, z, z, variables, 5, lr=0.1, weight_decay_rate=0.5)
    assert np.isclose(r[0], 2.0) and np.allclose(th[:2], w[:2] - 0.1 * 2.0 * 0.5 * w[:2])
    assert r[3] == 1.0 and np.array_equal(th[6:], w[6:])
    assert R.lr_t(0.1, 0.5, 4) == 0.1 / 3.0
    # floats outside every variable are copied
    th, m, v, _ = R.step(w, w, w, g, variables[:1], 0, lr=0.1)
    assert np.array_equal(th[2:], w[2:]) and np.array_equal(m[2:], w[2:]) and np.array_equal(v[2:], w[2:])


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    import torch
    from lisec_amd.params import ParamStore
    return ParamStore(torch.device("cpu"))


def _spans(store):
    return {n: (o, o + (int(np.prod(s)) + 3) // 4 * 4) for n, (w, o, s) in store.offsets.items() if w == "theta"}


LISTS = [None, (), ("bias", "gamma", "beta"), ("cls.bias", "rpn2.conv3.kernel", "vfe1.bn.beta"),
         ("gamma", "up3.kernel", "mid1.bn.gamma")]


@pytest.mark.parametrize("no_decay", LISTS)
@pytest.mark.parametrize("no_adapt", [None, (), ("kernel",), ("reg.kernel", "beta")])
def test_lamb_chunks(store, no_decay, no_adapt):
    chunks, variables = ops.lamb_chunks(store, no_decay, no_adapt)
    spans = _spans(store)
    # every trainable variable, ascending, whole over its padded length, no chunk across a variable
    assert [v[3] for v in variables] == sorted(spans, key=lambda n: spans[n][0])
    offs = [c[0] for c in chunks]
    assert offs == sorted(offs) and len(set(offs)) == len(offs)
    assert sum(c[1] for c in chunks) == store.n_theta
    at = 0
    for j, (first, n, off, name) in enumerate(variables):
        a, b = spans[name]
        assert first == at and off == a and n == -(-(b - a) // _lib.REG_CHUNK)
        pos = a
        for off_c, count, var, flags in chunks[first:first + n]:
            assert off_c == pos and var == j and count % 4 == 0 and off_c % 4 == 0 and 0 < count <= _lib.REG_CHUNK
            assert flags == chunks[first][3] and flags & ~(_lib.LAMB_DECAYED | _lib.LAMB_ADAPTED) == 0
            pos += count
        assert pos == b
        at += n
    assert at == len(chunks)
    # the lists select what decay_chunks selects; None for the adaptation list means the decay list
    undecayed = [c[:2] for c in chunks if not c[3] & _lib.LAMB_DECAYED]
    unadapted = [c[:2] for c in chunks if not c[3] & _lib.LAMB_ADAPTED]
    assert undecayed == ops.decay_chunks(store, no_decay or ())
    assert unadapted == ops.decay_chunks(store, (no_decay or ()) if no_adapt is None else no_adapt)
    as_lists = [None if x is None else list(x) for x in (no_decay, no_adapt)]
    assert ops.lamb_chunks(store, *as_lists) == (chunks, variables)
    table = ops.lamb_table(chunks, variables, "cpu")
    assert (table.n_chunks, table.n_vars) == (len(chunks), len(variables))
    assert ctypes.sizeof(_lib.LambChunk) == 24 and ctypes.sizeof(_lib.LambVar) == 8
    back = np.frombuffer(table.chunks.numpy().tobytes(), dtype=np.dtype(
        [("offset", "<i8"), ("count", "<i4"), ("var", "<i4"), ("flags", "<i4"), ("reserved", "<i4")]))
    assert [(int(r["offset"]), int(r["count"]), int(r["var"]), int(r["flags"])) for r in back] == chunks
    assert not back["reserved"].any()
    vback = np.frombuffer(table.variables.numpy().tobytes(), dtype=np.dtype([("first", "<i4"), ("n", "<i4")]))
    assert [(int(r["first"]), int(r["n"])) for r in vback] == [v[:2] for v in variables]


def test_lamb_chunks_refusals(store):
    assert ops.lamb_chunks(store, "cls.bias") == ops.lamb_chunks(store, ["cls.bias", "cls.bias"], ("cls.bias",))
    for which in (0, 1):
        args = [None, None]
        args[which] = ["no.such.kernel"]
        with pytest.raises(KeyError):
            ops.lamb_chunks(store, *args)
        args[which] = ["moving_mean"]                                    # not a kind of trainable variable
        with pytest.raises(KeyError):
            ops.lamb_chunks(store, *args)
        for moving in ("mid1.bn.moving_mean", "rpn1.bn0.moving_variance"):
            args[which] = ["kernel", moving]
            with pytest.raises(ValueError):
                ops.lamb_chunks(store, *args)
    assert ops.LAMB_BLOCKS == 2048 and len(ops.lamb_chunks(store)[0]) < ops.LAMB_BLOCKS


# ---- the optimizer class ---------------------------------------------------------------------------------------------------------
CONFIG_KEYS = ["name", "learning_rate", "weight_decay_rate", "decay", "beta_1", "beta_2", "epsilon",
               "exclude_from_weight_decay", "exclude_from_layer_adaptation"]


def test_defaults_and_config():
    a = O.LAMB()
    assert (a.lr, a.beta_1, a.beta_2, a.epsilon, a.weight_decay_rate, a.exclude_from_weight_decay,
            a.exclude_from_layer_adaptation, a.name, a.decay) == (0.001, 0.9, 0.999, 1e-6, 0.0, None, None, "LAMB", 0.0)
    assert a.get_config() == dict(zip(CONFIG_KEYS, ["LAMB", 0.001, 0.0, 0.0, 0.9, 0.999, 1e-6, None, None]))
    assert list(a.get_config()) == CONFIG_KEYS                           # tfa's order
    # positional order of tfa
    b = O.LAMB(0.1, 0.2, 0.3, 0.4, 0.5, ["bias"], ["gamma", "cls.kernel"], "mine")
    assert b.get_config() == dict(zip(CONFIG_KEYS, ["mine", 0.1, 0.5, 0.0, 0.2, 0.3, 0.4, ["bias"], ["gamma", "cls.kernel"]]))
    assert O.LAMB(lr=0.5, decay=1e-3).lr == 0.5 and O.LAMB(lr=0.5, decay=1e-3).decay == 1e-3
    assert O.LAMB(exclude_from_weight_decay="bias").exclude_from_weight_decay == ["bias"]
    assert a.record is optimizer_table.BY_KIND["lamb"] and a.record.layerwise and a.record.class_name == "LAMB"
    assert [h.name for h in a.record.hyper] == ["weight_decay_rate", "beta_1", "beta_2", "epsilon"]
    assert [s.kind for s in a.record.slots] == ["m", "v"] and a.spec().slots == ("m", "v")
    assert a.record.step == ("lamb_step_dev", "lamb_step_sched")
    assert a.spec().launch[0] == "lamb_step_dev" and a.spec(device_lr=True).launch[0] == "lamb_step_sched"
    assert not any(o.layerwise or o.lists for o in optimizer_table.OPTIMIZERS if o.kind != "lamb")
    sched = O.schedules.CosineDecay(1e-3, 100)
    c = O.LAMB(sched)
    assert c.lr is sched and c.spec().device_lr and c.get_config()["learning_rate"]["class_name"] == "CosineDecay"
    a.lr = 0.25                                                          # a plain attribute that a callback may assign
    assert a.spec(device_lr=True).lr_descriptor.initial == 0.25 and a.decay_spec() is None


def test_spec_config():
    s = O.LAMB(0.01, weight_decay_rate=0.02, exclude_from_weight_decay=["bias"]).spec()
    assert s.config == ("lamb", 0.01, 0.0, 0.02, 0.9, 0.999, 1e-6, ("bias",), None)
    assert s.lists == (("bias",), None) and s.weight_decay is None
    assert O.LAMB(0.01).spec(device_lr=True).config == ("lamb", ("device",), 0.0, 0.0, 0.9, 0.999, 1e-6, None, None)
    assert O.LAMB(exclude_from_layer_adaptation=["beta"]).spec() != O.LAMB().spec()
    assert OptimizerSpec("lamb").epsilon == 1e-6 and OptimizerSpec("lamb", epsilon=1e-3).epsilon == 1e-3
    assert OptimizerSpec("adam").lists == () and not hasattr(OptimizerSpec("adam"), "exclude_from_weight_decay")


def test_refusals():
    for bad in (dict(beta_1=1.0), dict(beta_1=-0.1), dict(beta_2=1.0), dict(beta_2=float("nan")), dict(epsilon=-1e-6),
                dict(weight_decay_rate=-0.1), dict(exclude_from_weight_decay=[3]),
                dict(exclude_from_layer_adaptation=[None])):
        with pytest.raises(ValueError):
            O.LAMB(**bad)
    for clip in ("clipnorm", "clipvalue", "global_clipnorm"):
        with pytest.raises(NotImplementedError):
            O.LAMB(**{clip: 1.0})
    with pytest.raises(TypeError):
        O.LAMB(no_such_keyword=1)
    with pytest.raises(ValueError):                                      # LAMB carries its own decay
        O.extend_with_decoupled_weight_decay(O.LAMB)
    with pytest.raises(ValueError):
        O.deserialize({"class_name": "LAMBW", "config": {"weight_decay": 0.1}})
    with pytest.raises(ValueError):
        OptimizerSpec("lamb", weight_decay=DecaySpec(0.1))
    with pytest.raises(ValueError):
        O.get("lamb")                                                    # optimizers.get is unchanged


def test_round_trips_and_wrappers():
    sched = O.schedules.PiecewiseConstantDecay([10, 20], [1e-3, 1e-4, 1e-5])
    cases = [O.LAMB(), O.LAMB(sched, weight_decay_rate=0.01, exclude_from_weight_decay=["bias", "gamma", "beta"], name="mine"),
             O.LAMB(0.02, 0.8, 0.99, 1e-5, 0.1, ["bias"], ["cls.kernel"], decay=1e-4)]
    for opt in cases:
        ser = O.serialize(opt)
        assert ser["class_name"] == "LAMB" and list(ser["config"]) == CONFIG_KEYS
        json.dumps(ser)
        back = O.deserialize(ser)
        assert type(back) is O.LAMB and O.serialize(back) == ser
        assert back.spec() == opt.spec() and back.spec(device_lr=True) == opt.spec(device_lr=True)
        for wrap, avg in ((O.MovingAverage(opt, average_decay=0.9), AverageSpec("ema", decay=0.9)),
                          (O.SWA(opt, start_averaging=2, average_period=3), AverageSpec("swa", start=2, period=3))):
            spec = wrap.spec()
            assert spec.kind == "lamb" and spec.average == avg and spec.lists == opt.spec().lists
            assert spec.config == opt.spec().config + (("average",) + avg.config,)
            wser = O.serialize(wrap)
            assert wser["config"]["optimizer"] == ser and O.serialize(O.deserialize(wser)) == wser
            assert wrap.record.layerwise and wrap.lists == opt.lists
    wrap = O.SWA(O.LAMB())
    wrap.lr = 0.5
    assert wrap._optimizer.lr == 0.5


def test_the_spec_configs_of_the_other_kinds_are_what_they_were():
    """OptimizerSpec(kind).config with default arguments, written out from the commit before LAMB."""
    want = {
        "sgd": ("sgd", 0.01, 1e-06, 0.9, True),
        "adam": ("adam", 0.01, 1e-06, 0.9, 0.999, 1e-07, False),
        "rmsprop": ("rmsprop", 0.01, 1e-06, 0.9, 0.9, 1e-07, False),
        "adagrad": ("adagrad", 0.01, 1e-06, 0.1, 1e-07),
        "adadelta": ("adadelta", 0.01, 1e-06, 0.9, 1e-07),
        "adamax": ("adamax", 0.01, 1e-06, 0.9, 0.999, 1e-07),
        "nadam": ("nadam", 0.01, 1e-06, 0.9, 0.999, 1e-07),
    }
    assert set(OptimizerSpec.KINDS) == set(want) | {"lamb"}
    for kind, config in want.items():
        assert OptimizerSpec(kind).config == config, kind
        assert OptimizerSpec(kind, weight_decay_rate=0.5, exclude_from_weight_decay=["bias"]).config == config
    assert OptimizerSpec("adam").launch == ("adam_step_dev", ("m", "v", None), ("beta_1", "beta_2", "epsilon"))
    assert O.Adam().spec().config == ("adam", 0.001, 0.0, 0.9, 0.999, 1e-07, False)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def _trainable():
    return [n for n, _, k in param_specs() if k in TRAINABLE_KINDS]


def _arrays(params, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.standard_normal(params[n].shape).astype(F) for n in _trainable()}


def _training_config(path):
    with hdf5_lite.File(path) as f:
        return json.loads(bytes(f.attrs["training_config"]).decode())


def _optimizer_dict(opt):
    """What Model.save hands keras_h5.save_model for `opt`."""
    d = opt.record.as_dict(mt._serialize_rate(opt.lr), opt.decay, opt.hyper)
    d.update(opt.lists)
    return d


@pytest.mark.parametrize("lists", [(None, None), (["bias", "gamma", "beta"], None), (["bias"], ["cls.kernel", "beta"])])
def test_h5_round_trip_of_the_optimizer_dict(tmp_path, lists):
    params = glorot_numpy(seed=3)
    opt = O.LAMB(O.schedules.CosineDecay(1e-3, 40, alpha=0.1), weight_decay_rate=0.01, epsilon=1e-5,
                 exclude_from_weight_decay=lists[0], exclude_from_layer_adaptation=lists[1])
    given = {"m": _arrays(params, 1), "v": _arrays(params, 2)}
    d = _optimizer_dict(opt)
    assert d["class_name"] == "LAMB" and d["exclude_from_weight_decay"] == lists[0]
    path = str(tmp_path / "lamb.h5")
    keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=7, **given)
    assert _training_config(path)["optimizer_config"] == O.serialize(opt)            # the class and its whole config
    with hdf5_lite.File(path) as f:
        names = [bytes(n).decode() for n in np.asarray(f["optimizer_weights"].attrs["weight_names"]).ravel()]
    nv = len(_trainable())
    assert names[0] == "LAMB/iter:0" and all(n.startswith("LAMB/") for n in names) and len(names) == 1 + 2 * nv
    assert all(n.endswith("/m:0") for n in names[1:1 + nv]) and all(n.endswith("/v:0") for n in names[1 + nv:])
    ck = keras_h5.load_model(path)
    assert ck["iterations"] == 7 and ck["wrapper"] is None and ck["optimizer"] == d
    for s in ("m", "v"):
        for n in _trainable():
            assert np.array_equal(ck[s][n].view(np.uint32), given[s][n].view(np.uint32)), (s, n)
    back = O.deserialize(_training_config(path)["optimizer_config"])
    assert type(back) is O.LAMB and back.get_config() == opt.get_config() and back.spec() == opt.spec()
    # nested under an averaging wrapper
    wrap = O.SWA(opt, start_averaging=1, average_period=2)
    own = {k: v for k, v in wrap.get_config().items() if k != "optimizer"}
    keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=3, wrapper={"class_name": "SWA", "config": own},
                        average=_arrays(params, 9), **given)
    assert _training_config(path)["optimizer_config"] == O.serialize(wrap)
    ck = keras_h5.load_model(path)
    assert ck["optimizer"] == d and ck["wrapper"]["class_name"] == "SWA" and ck["average"] is not None


def test_h5_of_the_other_optimizers_gains_no_key():
    plain = dict(class_name="Adam", lr=0.002, decay=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False)
    assert json.dumps(keras_h5._training_config(plain)["optimizer_config"]) == (
        '{"class_name": "Adam", "config": {"name": "Adam", "learning_rate": 0.002, "decay": 0.0, "beta_1": 0.9, '
        '"beta_2": 0.999, "epsilon": 1e-07, "amsgrad": false}}')
    assert json.dumps(keras_h5._training_config(dict(class_name="LAMB", lr=0.1))["optimizer_config"]) == (
        '{"class_name": "LAMB", "config": {"name": "LAMB", "learning_rate": 0.1, "decay": 0.0, "weight_decay_rate": 0.0, '
        '"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-06, "exclude_from_weight_decay": null, '
        '"exclude_from_layer_adaptation": null}}')
