"""tf.keras 2.4 RMSprop, Adagrad, Adadelta, Adamax and Nadam without a GPU: the fp64 reference of their update rules
(shared with tests/test_gpu_keras_optimizers.py) pinned against torch.optim where the two conventions coincide, the
optimizer objects of model_training, and the Keras `.h5` layout of their state (training_config, optimizer_weights)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from lisec_amd import hdf5_lite, keras_h5
from lisec_amd import model_training as mt
from lisec_amd.network import OptimizerSpec
from lisec_amd.params import glorot_numpy, param_specs, TRAINABLE_KINDS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
H5PY_PYTHON = "/opt/conda/bin/python3.9"          # the interpreter with h5py that tests/test_hdf5_lite.py uses
PROBE = os.path.join(GOLDEN, "h5py_probe.py")


# ---- the reference: fp64 arithmetic on fp32 inputs; hyper-parameters and per-step scalars as the kernels get them ------
def _f(x):
    return float(np.float32(x))


def _lr_t(lr, decay, it):
    return lr / (1.0 + decay * it)


def keras_rmsprop(theta, rms, mom, mg, g, it, lr, decay, rho, momentum, epsilon, centered):
    """One RMSprop step; mom is None without momentum, mg None unless centered.  Returns (theta, rms, mom, mg)."""
    th, g = theta.astype(np.float64), g.astype(np.float64)
    r, eps, lr_t = _f(rho), _f(epsilon), _lr_t(lr, decay, it)
    rms = rms.astype(np.float64)
    if momentum == 0:                                  # TF's Python path: epsilon outside the square root
        rms = r * rms + (1.0 - r) * g * g
        den = rms
        if centered:
            mg = r * mg.astype(np.float64) + (1.0 - r) * g
            den = rms - mg * mg
        return th - lr_t * g / (np.sqrt(den) + eps), rms, None, mg
    rms = rms + (g * g - rms) * (1.0 - r)              # ResourceApply(Centered)RMSProp: epsilon inside it
    den = rms + eps
    if centered:
        mg = mg.astype(np.float64)
        mg = mg + (g - mg) * (1.0 - r)
        den = rms - mg * mg + eps
    mom = _f(momentum) * mom.astype(np.float64) + lr_t * g / np.sqrt(den)
    return th - mom, rms, mom, mg


def keras_adagrad(theta, acc, g, it, lr, decay, epsilon):
    th, g = theta.astype(np.float64), g.astype(np.float64)
    acc = acc.astype(np.float64) + g * g
    return th - _lr_t(lr, decay, it) * g / (np.sqrt(acc) + _f(epsilon)), acc


def keras_adadelta(theta, ag, av, g, it, lr, decay, rho, epsilon):
    th, g = theta.astype(np.float64), g.astype(np.float64)
    r, eps = _f(rho), _f(epsilon)
    ag = ag.astype(np.float64) * r + g * g * (1.0 - r)
    av = av.astype(np.float64)
    u = np.sqrt(av + eps) / np.sqrt(ag + eps) * g
    return th - u * _lr_t(lr, decay, it), ag, av * r + u * u * (1.0 - r)


def keras_adamax(theta, m, v, g, it, lr, decay, beta_1, beta_2, epsilon):
    """b1^t in fp32 as TF."""
    th, g = theta.astype(np.float64), g.astype(np.float64)
    b1, b2, eps = _f(beta_1), _f(beta_2), _f(epsilon)
    b1p = float(np.float32(b1) ** np.float32(it + 1))
    m = m.astype(np.float64) + (g - m) * (1.0 - b1)
    v = np.maximum(b2 * v.astype(np.float64), np.abs(g))
    return th - _lr_t(lr, decay, it) / (1.0 - b1p) * (m / (v + eps)), m, v


def nadam_scalars(cache, it, beta_1, beta_2, schedule_decay, f32=True):
    """(mu_t, mu_t1, P, P1, b2^t) of the step after `it` iterations, from the momentum_cache `cache` -- in fp32 as TF
    computes them, or in fp64 (f32=False, torch's convention)."""
    S = np.float32 if f32 else np.float64
    b1, b2, d = S(beta_1), S(beta_2), S(schedule_decay)
    t, t1 = S(it + 1), S(it + 2)
    mu_t = b1 * (S(1) - S(0.5) * S(0.96) ** (d * t))
    mu_t1 = b1 * (S(1) - S(0.5) * S(0.96) ** (d * t1))
    p = S(cache) * mu_t
    return mu_t, mu_t1, p, p * mu_t1, b2 ** t


def keras_nadam(theta, m, v, cache, g, it, lr, beta_1, beta_2, epsilon, schedule_decay, f32=True):
    """One Nadam step (lr is not decayed).  Returns (theta, m, v, cache) -- cache: the new momentum_cache, P."""
    th, g = theta.astype(np.float64), g.astype(np.float64)
    mu_t, mu_t1, p, p1, b2p = nadam_scalars(cache, it, beta_1, beta_2, schedule_decay, f32)
    S = np.float32 if f32 else np.float64
    b1, b2 = float(S(beta_1)), float(S(beta_2))
    omp, omp1, omv, om_mu = (float(S(1) - x) for x in (p, p1, b2p, mu_t))
    m = b1 * m.astype(np.float64) + (1.0 - b1) * g
    v = b2 * v.astype(np.float64) + (1.0 - b2) * g * g
    mbar = om_mu * (g / omp) + float(mu_t1) * (m / omp1)
    return th - lr * mbar / (np.sqrt(v / omv) + float(S(epsilon))), m, v, float(p)


# ---- the reference against torch.optim --------------------------------------------------------------------------------
# hyper-parameters exact in fp32 (the reference rounds them to fp32 as the kernels receive them; torch keeps doubles)
N = 1000


def _problem(seed):
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(N).astype(np.float32)
    grads = [rng.standard_normal(N).astype(np.float32) * (1 + k) for k in range(6)]
    return theta, grads


def _torch_run(theta, grads, make):
    p = torch.nn.Parameter(torch.from_numpy(theta.astype(np.float64)))
    opt = make([p])
    for g in grads:
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
    return p.detach().numpy()


@pytest.mark.parametrize("momentum,centered", [(0.0, False), (0.0, True), (0.5, False), (0.5, True)])
def test_rmsprop_reference_matches_torch(momentum, centered):
    """eps = 0 and a constant rate: torch's buffer is Keras' momentum / lr, its eps sits outside the root either way."""
    theta, grads = _problem(1)
    want = _torch_run(theta, grads, lambda ps: torch.optim.RMSprop(ps, lr=2 ** -7, alpha=0.875, eps=0.0,
                                                                   momentum=momentum, centered=centered))
    th, rms = theta, np.zeros(N)
    mom = np.zeros(N) if momentum else None
    mg = np.zeros(N) if centered else None
    for it, g in enumerate(grads):
        th, rms, mom, mg = keras_rmsprop(th, rms, mom, mg, g, it, 2 ** -7, 0.0, 0.875, momentum, 0.0, centered)
        assert (mom is None) == (momentum == 0) and (mg is None) == (not centered)
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("epsilon", [0.0, 2 ** -10])
def test_adagrad_reference_matches_torch(epsilon):
    theta, grads = _problem(2)
    want = _torch_run(theta, grads, lambda ps: torch.optim.Adagrad(ps, lr=2 ** -5, lr_decay=2 ** -3, eps=epsilon,
                                                                   initial_accumulator_value=0.25))
    th, acc = theta, np.full(N, 0.25)
    for it, g in enumerate(grads):
        th, acc = keras_adagrad(th, acc, g, it, 2 ** -5, 2 ** -3, epsilon)
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("epsilon", [2 ** -20, 2 ** -6])
def test_adadelta_reference_matches_torch(epsilon):
    theta, grads = _problem(3)
    want = _torch_run(theta, grads, lambda ps: torch.optim.Adadelta(ps, lr=0.5, rho=0.875, eps=epsilon))
    th, ag, av = theta, np.zeros(N), np.zeros(N)
    for it, g in enumerate(grads):
        th, ag, av = keras_adadelta(th, ag, av, g, it, 0.5, 0.0, 0.875, epsilon)
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=1e-12)


def test_adamax_reference_matches_torch():
    """eps = 0: torch adds eps to |g| inside the max, Keras to the max."""
    theta, grads = _problem(4)
    want = _torch_run(theta, grads, lambda ps: torch.optim.Adamax(ps, lr=2 ** -6, betas=(0.875, 0.9375), eps=0.0))
    th, m, v = theta, np.zeros(N), np.zeros(N)
    for it, g in enumerate(grads):
        th, m, v = keras_adamax(th, m, v, g, it, 2 ** -6, 0.0, 0.875, 0.9375, 0.0)
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("epsilon", [0.0, 1e-7])
def test_nadam_reference_matches_torch(epsilon):
    """torch.optim.NAdam(momentum_decay=schedule_decay) with fp64 scalars (its mu_product is fp64 under a float64
    default dtype); the reference with TF's fp32 scalars stays within fp32 rounding of it."""
    theta, grads = _problem(5)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        want = _torch_run(theta, grads, lambda ps: torch.optim.NAdam(ps, lr=2 ** -7, betas=(0.875, 0.9375), eps=epsilon,
                                                                     momentum_decay=0.004))
    finally:
        torch.set_default_dtype(old)
    for f32, tol in ((False, 1e-12), (True, 1e-6)):
        th, m, v, cache = theta, np.zeros(N), np.zeros(N), 1.0
        for it, g in enumerate(grads):
            th, m, v, cache = keras_nadam(th, m, v, cache, g, it, 2 ** -7, 0.875, 0.9375, epsilon, 0.004, f32=f32)
        np.testing.assert_allclose(th, want, rtol=tol, atol=tol)


def test_nadam_cache_is_the_product_of_the_momentum_schedule():
    cache = 1.0
    for it in range(4):
        cache = float(nadam_scalars(cache, it, 0.9, 0.999, 0.004)[2])
    mus = [0.9 * (1 - 0.5 * 0.96 ** (0.004 * t)) for t in range(1, 5)]
    assert abs(cache - np.prod(mus)) <= 1e-6 * abs(cache)


# ---- optimizer objects ------------------------------------------------------------------------------------------------
def test_defaults_get_config_and_slots():
    O = mt.optimizers
    r = O.RMSprop()
    assert (r.lr, r.decay, r.rho, r.momentum, r.epsilon, r.centered) == (0.001, 0.0, 0.9, 0.0, 1e-7, False)
    assert r.get_config() == {"name": "RMSprop", "learning_rate": 0.001, "decay": 0.0, "rho": 0.9, "momentum": 0.0,
                              "epsilon": 1e-7, "centered": False}
    assert list(r.get_config()) == ["name", "learning_rate", "decay", "rho", "momentum", "epsilon", "centered"]
    assert r.spec().slots == ("rms",)
    assert O.RMSprop(momentum=0.9).spec().slots == ("rms", "momentum")
    assert O.RMSprop(centered=True).spec().slots == ("rms", "mg")
    assert O.RMSprop(momentum=0.9, centered=True).spec().slots == ("rms", "momentum", "mg")
    a = O.Adagrad()
    assert (a.lr, a.decay, a.initial_accumulator_value, a.epsilon) == (0.001, 0.0, 0.1, 1e-7)
    assert list(a.get_config().items()) == [("name", "Adagrad"), ("learning_rate", 0.001), ("decay", 0.0),
                                            ("initial_accumulator_value", 0.1), ("epsilon", 1e-7)]
    assert a.spec().slots == ("accumulator",)
    d = O.Adadelta()
    assert (d.lr, d.rho, d.epsilon) == (0.001, 0.95, 1e-7) and d.spec().slots == ("accum_grad", "accum_var")
    assert list(d.get_config().items()) == [("name", "Adadelta"), ("learning_rate", 0.001), ("decay", 0.0),
                                            ("rho", 0.95), ("epsilon", 1e-7)]
    x = O.Adamax()
    assert (x.lr, x.beta_1, x.beta_2, x.epsilon) == (0.001, 0.9, 0.999, 1e-7) and x.spec().slots == ("m", "v")
    assert list(x.get_config().items()) == [("name", "Adamax"), ("learning_rate", 0.001), ("decay", 0.0),
                                            ("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7)]
    n = O.Nadam()
    assert (n.lr, n.decay, n.beta_1, n.beta_2, n.epsilon) == (0.001, 0.004, 0.9, 0.999, 1e-7)
    assert n.spec().slots == ("m", "v")
    assert list(n.get_config().items()) == [("name", "Nadam"), ("learning_rate", 0.001), ("decay", 0.004),
                                            ("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7)]
    assert O.Nadam(schedule_decay=0.01).decay == 0.01 and O.Nadam(decay=0.02).decay == 0.02
    # the legacy spelling lr= and a rate given positionally
    assert O.RMSprop(lr=0.01).lr == 0.01 and O.Adagrad(0.02).lr == 0.02 and O.Nadam(lr=0.5).lr == 0.5
    for o in (r, a, d, x, n):
        assert O.get(o) is o
    with pytest.raises(ValueError, match="RMSprop()"):
        O.get("rmsprop")


def test_argument_validation():
    O = mt.optimizers
    bad = [lambda: O.RMSprop(rho=1.0), lambda: O.RMSprop(rho=-0.1), lambda: O.RMSprop(momentum=-0.5),
           lambda: O.RMSprop(momentum=1.5), lambda: O.RMSprop(epsilon=-1.0), lambda: O.Adagrad(initial_accumulator_value=-1),
           lambda: O.Adagrad(epsilon=-1.0), lambda: O.Adadelta(rho=1.0), lambda: O.Adamax(beta_1=1.0),
           lambda: O.Adamax(beta_2=-0.1), lambda: O.Nadam(beta_2=1.0), lambda: O.Nadam(epsilon=-1e-7)]
    for make in bad:
        with pytest.raises(ValueError):
            make()
    with pytest.raises(TypeError):
        O.Adadelta(no_such_argument=1)


def test_distinct_configs_and_spec_kinds():
    O = mt.optimizers
    opts = [O.RMSprop(), O.RMSprop(momentum=0.9), O.RMSprop(centered=True), O.RMSprop(momentum=0.9, centered=True),
            O.RMSprop(rho=0.8), O.Adagrad(), O.Adagrad(initial_accumulator_value=0.2), O.Adadelta(), O.Adadelta(rho=0.9),
            O.Adamax(), O.Adamax(beta_2=0.99), O.Nadam(), O.Nadam(schedule_decay=0.01), O.Adam(), O.SGD()]
    configs = {o.spec().config for o in opts}
    assert len(configs) == len(opts)
    assert O.Adamax().spec().config != O.Nadam(schedule_decay=0.0).spec().config
    assert [o.spec().kind for o in opts[::4]] == ["rmsprop", "rmsprop", "adadelta", "nadam"]
    # a rate from the device descriptor leaves the config; Nadam's descriptor carries no decay
    dev = O.Nadam(learning_rate=0.002).spec(device_lr=True)
    assert dev.device_lr and dev.lr_descriptor.kind == 0 and dev.lr_descriptor.initial == 0.002
    assert dev.lr_descriptor.decay == 0.0
    assert O.Adagrad(decay=1e-3).spec(device_lr=True).lr_descriptor.decay == 1e-3
    # the SGD and Adam configs of before
    assert OptimizerSpec("sgd", 0.01, 1e-6, 0.9, True).config == ("sgd", 0.01, 1e-6, 0.9, True)
    assert O.Adam().spec().config == ("adam", 0.001, 0.0, 0.9, 0.999, 1e-7, False)


def test_schedules_and_nadam():
    O, S = mt.optimizers, mt.optimizers.schedules
    sched = S.ExponentialDecay(0.01, 100, 0.5)
    for cls in (O.RMSprop, O.Adagrad, O.Adadelta, O.Adamax):
        spec = cls(learning_rate=sched).spec()
        assert spec.device_lr and spec.lr_descriptor.kind == 1
    with pytest.raises(ValueError, match="Nadam"):
        O.Nadam(learning_rate=sched)
    with pytest.raises(ValueError, match="Nadam"):
        OptimizerSpec("nadam", sched, 0.004)


@pytest.mark.parametrize("kw", ["clipnorm", "clipvalue", "global_clipnorm"])
def test_gradient_clipping_is_still_refused(kw):
    for cls in (mt.optimizers.RMSprop, mt.optimizers.Adagrad, mt.optimizers.Adadelta, mt.optimizers.Adamax,
                mt.optimizers.Nadam):
        with pytest.raises(NotImplementedError, match="clipping"):
            cls(**{kw: 1.0})
        cls(**{kw: None})


# ---- Keras .h5 layout of the optimizer state --------------------------------------------------------------------------
CONFIGS = {
    "rmsprop": dict(class_name="RMSprop", lr=0.002, decay=1e-5, rho=0.85, momentum=0.0, epsilon=1e-6, centered=False),
    "rmsprop_cm": dict(class_name="RMSprop", lr=0.001, decay=0.0, rho=0.9, momentum=0.8, epsilon=1e-7, centered=True),
    "adagrad": dict(class_name="Adagrad", lr=0.01, decay=1e-4, initial_accumulator_value=0.2, epsilon=1e-7),
    "adadelta": dict(class_name="Adadelta", lr=1.0, decay=0.0, rho=0.9, epsilon=1e-6),
    "adamax": dict(class_name="Adamax", lr=0.002, decay=1e-6, beta_1=0.85, beta_2=0.995, epsilon=1e-7),
    "nadam": dict(class_name="Nadam", lr=0.002, decay=0.005, beta_1=0.9, beta_2=0.999, epsilon=1e-7),
}
KINDS = {"rmsprop": ("rms",), "rmsprop_cm": ("rms", "momentum", "mg"), "adagrad": ("accumulator",),
         "adadelta": ("accum_grad", "accum_var"), "adamax": ("m", "v"), "nadam": ("m", "v")}
CONFIG_KEYS = {"RMSprop": ["rho", "momentum", "epsilon", "centered"], "Adagrad": ["initial_accumulator_value", "epsilon"],
               "Adadelta": ["rho", "epsilon"], "Adamax": ["beta_1", "beta_2", "epsilon"],
               "Nadam": ["beta_1", "beta_2", "epsilon"]}


def _write(tmp_path, which):
    params = glorot_numpy(seed=3)
    rng = np.random.default_rng(4)
    trainable = [n for n, _, k in param_specs() if k in TRAINABLE_KINDS]
    shapes = {n: s for n, s, _ in param_specs()}
    slots = {k: {n: rng.standard_normal(shapes[n]).astype(np.float32) for n in trainable} for k in KINDS[which]}
    path = str(tmp_path / f"{which}.h5")
    keras_h5.save_model(path, params, 16, 32, 8, 35, optimizer=CONFIGS[which], iterations=37, momentum_cache=0.625,
                        **slots)
    return path, params, slots


@pytest.mark.parametrize("which", list(CONFIGS))
def test_keras_h5_round_trip_of_optimizer_state(tmp_path, which):
    path, params, slots = _write(tmp_path, which)
    cfg = CONFIGS[which]
    cls = cfg["class_name"]
    with hdf5_lite.File(path) as f:
        tc = json.loads(bytes(f.attrs["training_config"]).decode())["optimizer_config"]
        og = f["optimizer_weights"]
        names = [bytes(n).decode() for n in np.asarray(og.attrs["weight_names"]).ravel()]
        it = og[f"{cls}/iter:0"][()]
        assert int(it) == 37 and np.asarray(it).dtype == np.int64
        if cls == "Nadam":
            c = og["Nadam/momentum_cache:0"][()]
            assert np.asarray(c).dtype == np.float32 and np.asarray(c).shape == () and float(c) == 0.625
        stored = {n: og[n][()] for n in names[1:] if not n.endswith("momentum_cache:0")}
    assert tc["class_name"] == cls
    assert list(tc["config"]) == ["name", "learning_rate", "decay"] + CONFIG_KEYS[cls]
    assert tc["config"] == dict(name=cls, learning_rate=cfg["lr"], decay=cfg["decay"],
                                **{k: cfg[k] for k in CONFIG_KEYS[cls]})
    # Keras' order: iter, (Nadam) momentum_cache, then one slot kind for every trainable variable, then the next kind
    layers, _ = keras_h5.keras_layers(16, 32, 8, 35)
    to_param = {f"{L['name']}/{w}": p for L in layers for w, p in L["weights"]}
    variables = [f"{L['name']}/{w}" for L in layers for w, _ in L["weights"] if w in ("kernel", "bias", "gamma", "beta")]
    head = [f"{cls}/iter:0"] + (["Nadam/momentum_cache:0"] if cls == "Nadam" else [])
    assert names == head + [f"{cls}/{var}/{k}:0" for k in KINDS[which] for var in variables]
    for n, a in stored.items():
        var, kind = n[len(cls) + 1:].rsplit("/", 1)
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, slots[kind[:-2]][to_param[var]])
    ck = keras_h5.load_model(path)
    assert ck["iterations"] == 37 and ck["optimizer"] == cfg
    assert ck["momentum_cache"] == (0.625 if cls == "Nadam" else None)
    for k in keras_h5.SLOT_KEYS:
        assert (ck[k] is not None) == (k in KINDS[which]), k
    for k in KINDS[which]:
        assert set(ck[k]) == set(slots[k])
        for n in slots[k]:
            np.testing.assert_array_equal(ck[k][n], slots[k][n])
    for n in params:
        np.testing.assert_array_equal(ck["params"][n], params[n])


def test_rmsprop_momentum_is_not_sgd_velocity(tmp_path):
    """The same Keras slot name, two meanings: SGD's "momentum" reads back as velocity, RMSprop's as its own buffer."""
    path, _, slots = _write(tmp_path, "rmsprop_cm")
    ck = keras_h5.load_model(path)
    assert ck["velocity"] is None and ck["momentum"] is not None
    params = glorot_numpy(seed=3)
    sgd = str(tmp_path / "sgd.h5")
    keras_h5.save_model(sgd, params, 16, 32, 8, 35, optimizer=dict(lr=0.01, decay=0.0, momentum=0.9, nesterov=False),
                        iterations=2, velocity=slots["momentum"])
    ck = keras_h5.load_model(sgd)
    assert ck["momentum"] is None and ck["velocity"] is not None


def test_float_rate_training_config_of_sgd_and_adam_is_unchanged():
    sgd = keras_h5._training_config(dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True))
    assert json.dumps(sgd["optimizer_config"]) == ('{"class_name": "SGD", "config": {"name": "SGD", "learning_rate": 0.01, '
                                                   '"decay": 1e-06, "momentum": 0.9, "nesterov": true}}')


def _have_h5py():
    if not os.path.exists(H5PY_PYTHON):
        return False
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    return subprocess.run([H5PY_PYTHON, "-c", "import h5py"], env=env, capture_output=True).returncode == 0


@pytest.mark.parametrize("which", ["rmsprop_cm", "nadam"])
def test_file_reads_with_h5py(tmp_path, which):
    path, _, slots = _write(tmp_path, which)
    if not _have_h5py():
        return                                             # the hdf5_lite round trip above still ran; no h5py here
    import hashlib
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    desc = json.loads(subprocess.run([H5PY_PYTHON, PROBE, "dump", path], env=env, capture_output=True, check=True).stdout)
    cls = CONFIGS[which]["class_name"]
    names = desc["/optimizer_weights"]["attrs"]["weight_names"]["value"]
    assert names[0] == f"{cls}/iter:0"
    tc = json.loads(desc["/"]["attrs"]["training_config"]["value"])
    assert tc["optimizer_config"]["class_name"] == cls
    ck = keras_h5.load_model(path)
    layers, _ = keras_h5.keras_layers(16, 32, 8, 35)
    to_param = {f"{L['name']}/{w}": p for L in layers for w, p in L["weights"]}
    for n in names[1:]:
        d = desc["/optimizer_weights/" + n]
        assert d["dtype"] == "<f4"
        if n.endswith("momentum_cache:0"):
            continue
        var, kind = n[len(cls) + 1:].rsplit("/", 1)
        a = ck[kind[:-2]][to_param[var]]
        assert d["sha"] == hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
