"""Gradient clipping without a GPU: the numpy definition (tests/grad_clip_ref.py) on hand cases, the attributes and
optimizers.clip_gradients on every optimizer class and through the wrappers, the refusals, the configs and their round
trips, the spec configs, the optimizer dict in the Keras .h5 checkpoints and the table of the passes."""
import json

import numpy as np
import pytest

import grad_clip_ref as R
from lisec_amd import _lib, hdf5_lite, keras_h5, ops, optimizer_table
from lisec_amd import model_training as mt
from lisec_amd.network import AverageSpec, ClipSpec, DecaySpec, OptimizerSpec
from lisec_amd.params import glorot_numpy

F = np.float32
O = mt.optimizers
GRID = (16, 32, 8, 35)
KEYS = {"clipnorm": "norm", "clipvalue": "value", "global_clipnorm": "global_norm"}
BASES = [O.SGD, O.Adam, O.RMSprop, O.Adagrad, O.Adadelta, O.Adamax, O.Nadam]


def _every_optimizer():
    made = [cls() for cls in BASES] + [O.LAMB(), O.AdamW(0.01), O.SGDW(0.01, momentum=0.9)]
    made += [O.extend_with_decoupled_weight_decay(O.RMSprop)(0.02)]
    return made


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


# ---- the definition --------------------------------------------------------------------------------------------------------
def test_the_definition_on_hand_cases():
    g = np.array([3, 4, 0, 0], F)
    one = [(0, 4)]
    out, scales, norms = R.clip_by_norm(g, 5.0, one)
    assert scales[0] == F(1.0) and norms[0] == F(5.0) and np.array_equal(_bits(out), _bits(g))
    out, scales, norms = R.clip_by_norm(g, 2.5, one)
    assert scales[0] == F(0.5) and norms[0] == F(5.0) and np.array_equal(out, np.array([1.5, 2, 0, 0], F))
    out, scale, norm = R.clip_by_global_norm(np.array([3, 0, 0, 0, 9, 9, 9, 9, 4, 0, 0, 0], F), 2.5, [(0, 4), (8, 4)])
    assert scale == F(0.5) and norm == F(5.0)
    assert np.array_equal(out, np.array([1.5, 0, 0, 0, 9, 9, 9, 9, 2, 0, 0, 0], F))          # the gap keeps its floats
    # per variable: one clipped, one not
    out, scales, _ = R.clip_by_norm(np.array([3, 4, 0, 0, 0.3, 0.4, 0, 0], F), 1.0, [(0, 4), (4, 4)])
    assert scales[0] == F(0.2) and scales[1] == F(1.0) and np.array_equal(_bits(out[4:]), _bits([0.3, 0.4, 0, 0]))
    # nothing to scale, nothing to divide by
    out, scales, norms = R.clip_by_norm(np.zeros(4, F), 1.0, one)
    assert scales[0] == F(1.0) and norms[0] == 0 and not out.any()
    # an inf or a NaN in a variable: the scale is NaN, and so is the variable
    for bad in (np.inf, -np.inf, np.nan):
        out, scales, norms = R.clip_by_norm(np.array([1, bad, 0, 0], F), 1.0, one)
        assert np.isnan(scales[0]) and np.isnan(out).all() and not np.isfinite(norms[0])
    # by value: NaN, -0 and denormals keep their bits, the infinities become +-c
    tiny = np.float32(1e-45)
    g = np.array([np.nan, -0.0, tiny, -tiny, np.inf, -np.inf, 2.0, -2.0, 1.0, -1.0, 0.5, 0.0], F)
    out = R.clip_by_value(g, 1.0)
    want = np.array([np.nan, -0.0, tiny, -tiny, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 0.5, 0.0], F)
    assert np.array_equal(_bits(out), _bits(want))
    payload = np.array([0x7fc12345, 0xffc00001], np.uint32).view(F)
    assert np.array_equal(_bits(R.clip_by_value(payload, 3.0)), _bits(payload))
    assert np.array_equal(R.clip("value", g[6:], 1.0, [(0, 1)]), np.array([1, -2, 1, -1, 0.5, 0], F))
    # the scale is rounded once from float64
    S = R.sum_squares(np.array([1, 1, 1, 0], F))
    assert R.scale_of(S, 1.0)[0] == F(1.0 / np.sqrt(3.0)) and R.scale_of(S, 2.0)[0] == F(1.0)


# ---- the optimizer classes ---------------------------------------------------------------------------------------------------
def test_attributes_and_helper_on_every_class():
    for opt in _every_optimizer():
        name = type(opt).__name__
        before, spec_before = opt.get_config(), opt.spec().config
        assert (opt.clipnorm, opt.clipvalue, opt.global_clipnorm) == (None, None, None), name
        assert opt.clip_spec() is None and opt.spec().clip is None
        assert not set(before) & set(KEYS), name
        for key, kind in KEYS.items():
            assert O.clip_gradients(opt, **{key: 2}) is opt
            assert getattr(opt, key) == 2.0 and isinstance(getattr(opt, key), float)
            assert [getattr(opt, k) for k in KEYS if k != key] == [None, None]
            assert opt.clip_spec() == ClipSpec(kind, 2.0) and opt.spec().clip == ClipSpec(kind, 2.0)
            assert opt.spec(device_lr=True).clip == ClipSpec(kind, 2.0)
            assert opt.get_config() == {**before, key: 2.0}, name
            assert list(opt.get_config())[:len(before)] == list(before)
            assert opt.spec().config == spec_before + (("clip", kind, 2.0),)
            assert O.clip_gradients(opt) is opt and opt.clip_spec() is None               # all three None: cleared
            assert opt.get_config() == before and opt.spec().config == spec_before
            setattr(opt, key, 0.25)                                                       # a plain attribute
            assert opt.spec().clip == ClipSpec(kind, 0.25) and opt.get_config()[key] == 0.25
            setattr(opt, key, None)
        assert json.dumps(opt.get_config()) == json.dumps(before)                        # byte-identical when unset


def test_strings():
    a = O.clip_gradients("adam", global_clipnorm=10)
    assert type(a) is O.Adam and a.global_clipnorm == 10.0 and a.lr == 0.001
    s = O.clip_gradients("sgd", clipvalue=0.5)
    assert type(s) is O.SGD and s.clipvalue == 0.5
    with pytest.raises(ValueError):
        O.clip_gradients("lamb", clipnorm=1.0)
    with pytest.raises(ValueError):
        O.clip_gradients(None, clipnorm=1.0)


@pytest.mark.parametrize("wrap", ["MovingAverage", "SWA"])
def test_through_the_wrappers(wrap):
    inner = O.Adam(0.01)
    w = getattr(O, wrap)(inner)
    bare = getattr(O, wrap)(O.Adam(0.01))
    assert (w.clipnorm, w.clipvalue, w.global_clipnorm) == (None, None, None)
    assert O.clip_gradients(w, clipnorm=3.0) is w
    assert inner.clipnorm == 3.0 and w.clipnorm == 3.0 and "clipnorm" not in vars(w)
    assert w.spec().clip == ClipSpec("norm", 3.0) and w.spec().average is not None
    assert w.spec().config == bare.spec().config + (("clip", "norm", 3.0),)
    cfg = w.get_config()
    assert "clipnorm" not in cfg and cfg["optimizer"]["config"]["clipnorm"] == 3.0       # nested
    w.global_clipnorm = 7.0                                                                 # writes go through as well
    assert inner.global_clipnorm == 7.0
    with pytest.raises(ValueError):
        w.spec()                                                                            # two at once
    w.clipnorm = None
    assert w.spec().clip == ClipSpec("global_norm", 7.0)
    back = O.deserialize(O.serialize(w))
    assert type(back).__name__ == wrap and back.global_clipnorm == 7.0 and back.spec() == w.spec()
    assert O.serialize(back) == O.serialize(w)
    O.clip_gradients(w)
    assert inner.global_clipnorm is None and O.serialize(w) == O.serialize(bare)


BAD = [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), True, False, 1e39, "one", [1.0]]


def test_refusals():
    for bad in BAD:
        for key, kind in KEYS.items():
            opt = O.Adam()
            with pytest.raises(ValueError):
                O.clip_gradients(opt, **{key: bad})
            assert opt.clip_spec() is None                                 # nothing was assigned
            setattr(opt, key, bad)                                         # assigned directly: spec() refuses it
            with pytest.raises(ValueError):
                opt.spec()
            with pytest.raises(ValueError):
                ClipSpec(kind, bad)
    for pair in ({"clipnorm": 1.0, "clipvalue": 1.0}, {"clipnorm": 1.0, "global_clipnorm": 1.0},
                 {"clipvalue": 1.0, "global_clipnorm": 1.0}, {"clipnorm": 1.0, "clipvalue": 1.0, "global_clipnorm": 1.0}):
        opt = O.SGD()
        with pytest.raises(ValueError):
            O.clip_gradients(opt, **pair)
        assert opt.clip_spec() is None
        for k, v in pair.items():
            setattr(opt, k, v)
        with pytest.raises(ValueError):
            opt.spec()
        with pytest.raises(ValueError):
            O.deserialize({"class_name": "SGD", "config": pair})
    with pytest.raises(ValueError):
        ClipSpec("l2", 1.0)
    with pytest.raises(ValueError):
        OptimizerSpec("adam", clip=1.0)
    with pytest.raises(ValueError):
        OptimizerSpec("adam", clip=("norm", 1.0))
    # the largest float32 is a threshold; the constructor keywords stay refused
    assert ClipSpec("norm", float(np.finfo(F).max)).value == float(np.finfo(F).max)
    for cls in BASES + [O.LAMB]:
        for key in KEYS:
            with pytest.raises(NotImplementedError, match="clipping"):
                cls(**{key: 1.0})
    with pytest.raises(NotImplementedError, match="clipping"):
        O.AdamW(0.01, clipnorm=1.0)


def test_round_trips():
    sched = O.schedules.ExponentialDecay(0.01, 10, 0.5)
    for opt in _every_optimizer() + [O.Adam(sched), O.LAMB(exclude_from_weight_decay=["bias"])]:
        plain = O.serialize(opt)
        assert type(O.deserialize(plain)) is type(opt) and O.deserialize(plain).clip_spec() is None
        for key, kind in KEYS.items():
            O.clip_gradients(opt, **{key: 1.5})
            ser = O.serialize(opt)
            json.dumps(ser)
            assert ser["config"][key] == 1.5 and {k: v for k, v in ser["config"].items() if k != key} == plain["config"]
            back = O.deserialize(ser)
            assert type(back) is type(opt) and getattr(back, key) == 1.5 and O.serialize(back) == ser
            assert back.spec() == opt.spec() and back.spec().clip == ClipSpec(kind, 1.5)
        O.clip_gradients(opt)
        assert O.serialize(opt) == plain


def test_spec_config():
    base = ("adam", 0.001, 0.0, 0.9, 0.999, 1e-07, False)
    assert O.Adam().spec().config == base                                               # what it was
    assert O.Adam().get_config() == {"name": "Adam", "learning_rate": 0.001, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.999,
                                     "epsilon": 1e-7, "amsgrad": False}
    specs = {(k, v): O.clip_gradients(O.Adam(), **{k: v}).spec() for k in KEYS for v in (1.0, 2.0)}
    assert len({s.config for s in specs.values()} | {base}) == 7 and len(set(specs.values())) == 6
    for (k, v), s in specs.items():
        assert s.config == base + (("clip", KEYS[k], v),) and s != O.Adam().spec()
        assert s.launch == O.Adam().spec().launch and s.slots == ("m", "v")
    # behind the averaging and the decay, each present only when asked for
    w = O.clip_gradients(O.MovingAverage(O.AdamW(0.01), average_decay=0.9), clipvalue=0.5)
    plain = O.MovingAverage(O.AdamW(0.01), average_decay=0.9).spec().config
    assert w.spec().config == plain + (("clip", "value", 0.5),)
    assert plain[-2][0] == "average" and plain[-1][0] == "weight_decay"
    assert OptimizerSpec("sgd").config == ("sgd", 0.01, 1e-06, 0.9, True) and OptimizerSpec("sgd").clip is None
    assert OptimizerSpec("sgd", clip=ClipSpec("global_norm", 10)).config == ("sgd", 0.01, 1e-06, 0.9, True,
                                                                             ("clip", "global_norm", 10.0))
    assert ClipSpec("norm", 1) == ClipSpec("norm", 1.0) != ClipSpec("global_norm", 1.0)
    assert hash(ClipSpec("value", 2)) == hash(ClipSpec("value", 2.0)) and "value" in repr(ClipSpec("value", 2))
    assert isinstance(OptimizerSpec("lamb", clip=ClipSpec("norm", 1.0)).average, type(None))
    assert OptimizerSpec("adam", weight_decay=DecaySpec(0.1), average=AverageSpec("swa"),
                         clip=ClipSpec("norm", 1.0)).config[-1] == ("clip", "norm", 1.0)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def _training_config(path):
    with hdf5_lite.File(path) as f:
        return json.loads(bytes(f.attrs["training_config"]).decode())


def _optimizer_dict(opt):
    """What Model.save hands keras_h5.save_model for `opt` (an optimizer without a wrapper)."""
    d = opt.record.as_dict(mt._serialize_rate(opt.lr), opt.decay, opt.hyper)
    d.update(opt.lists)
    if isinstance(opt, mt._DecoupledWeightDecay):
        d.update(class_name=type(opt).__name__, weight_decay=mt._serialize_rate(opt.weight_decay))
    d.update(opt._clip_config())
    return d


def test_h5_round_trip_of_the_optimizer_config(tmp_path):
    params = glorot_numpy(seed=3)
    path = str(tmp_path / "clip.h5")
    cases = [(O.Adam(0.002), "global_clipnorm", 10.0), (O.SGD(0.1, momentum=0.9), "clipvalue", 0.5),
             (O.AdamW(0.01), "clipnorm", 1.0), (O.LAMB(), "global_clipnorm", 2.0), (O.RMSprop(), "clipnorm", 0.125)]
    for opt, key, value in cases:
        d_plain = _optimizer_dict(opt)
        plain = json.dumps(keras_h5._training_config(d_plain)["optimizer_config"])
        assert not any(k in plain for k in KEYS)
        O.clip_gradients(opt, **{key: value})
        d = _optimizer_dict(opt)
        assert d == {**d_plain, key: value}
        keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=4)
        oc = _training_config(path)["optimizer_config"]
        assert oc == O.serialize(opt) and oc["config"][key] == value
        ck = keras_h5.load_model(path)
        assert ck["optimizer"] == d and ck["wrapper"] is None
        back = O.deserialize(oc)
        assert type(back) is type(opt) and back.spec() == opt.spec() and getattr(back, key) == value
        # nested under an averaging wrapper: the key stays with the wrapped optimizer
        wrap = O.SWA(opt, start_averaging=1, average_period=2)
        own = {k: v for k, v in wrap.get_config().items() if k != "optimizer"}
        keras_h5.save_model(path, params, *GRID, optimizer=d, iterations=3, wrapper={"class_name": "SWA", "config": own})
        oc = _training_config(path)["optimizer_config"]
        assert oc == O.serialize(wrap) and key not in oc["config"] and oc["config"]["optimizer"]["config"][key] == value
        ck = keras_h5.load_model(path)
        assert ck["optimizer"] == d and ck["wrapper"]["class_name"] == "SWA"
        assert O.deserialize(oc).spec() == wrap.spec()
        # and without clipping the file's optimizer_config has the bytes it had
        O.clip_gradients(opt)
        assert json.dumps(keras_h5._training_config(_optimizer_dict(opt))["optimizer_config"]) == plain


def test_h5_without_clipping_gains_no_key():
    plain = dict(class_name="Adam", lr=0.002, decay=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False)
    assert json.dumps(keras_h5._training_config(plain)["optimizer_config"]) == (
        '{"class_name": "Adam", "config": {"name": "Adam", "learning_rate": 0.002, "decay": 0.0, "beta_1": 0.9, '
        '"beta_2": 0.999, "epsilon": 1e-07, "amsgrad": false}}')
    assert json.dumps(keras_h5._training_config(dict(plain, clipnorm=None, global_clipnorm=1))["optimizer_config"]) == (
        '{"class_name": "Adam", "config": {"name": "Adam", "learning_rate": 0.002, "decay": 0.0, "beta_1": 0.9, '
        '"beta_2": 0.999, "epsilon": 1e-07, "amsgrad": false, "global_clipnorm": 1.0}}')


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_the_table_is_every_trainable_variable():
    import torch
    from lisec_amd.params import ParamStore
    store = ParamStore(torch.device("cpu"))
    chunks, variables = ops.clip_chunks(store)
    assert (chunks, variables) == ops.lamb_chunks(store)                    # one cutter: LAMB's, without exclusions
    spans = {n: (o, o + (int(np.prod(s)) + 3) // 4 * 4) for n, (w, o, s) in store.offsets.items() if w == "theta"}
    assert [v[3] for v in variables] == sorted(spans, key=lambda n: spans[n][0])
    assert sum(c[1] for c in chunks) == store.n_theta
    at = 0
    for j, (first, n, off, name) in enumerate(variables):
        a, b = spans[name]
        assert first == at and off == a and n == -(-(b - a) // _lib.REG_CHUNK)
        pos = a
        for off_c, count, var, _ in chunks[first:first + n]:
            assert off_c == pos and var == j and count % 4 == 0 and off_c % 4 == 0 and 0 < count <= _lib.REG_CHUNK
            pos += count
        assert pos == b
        at += n
    assert at == len(chunks)
    table = ops.lamb_table(chunks, variables, "cpu")
    assert (table.n_chunks, table.n_vars) == (len(chunks), len(variables)) and table.names == [v[3] for v in variables]
    # the early part and the closing part of a split update see adjacent rows that add up to everything
    mid = variables[len(variables) // 2][2]
    (f0, n0), (f1, n1) = table.chunks.span(0, mid), table.chunks.span(mid, store.n_theta)
    (v0, m0), (v1, m1) = table.variables.span(0, mid), table.variables.span(mid, store.n_theta)
    assert (f0, f1, n0 + n1) == (0, n0, len(chunks)) and (v0, v1, m0 + m1) == (0, m0, len(variables))
    assert variables[v1][0] == f1
    assert set(optimizer_table.BY_CLASS) >= {"SGD", "Adam", "LAMB"}
