"""tf.keras 2.4 SGD / Adam / AMSGrad without a GPU: the numpy reference of the update formulas (shared with
tests/test_gpu_optimizers.py) pinned against torch.optim, the optimizer objects of model_training, and the Keras `.h5`
layout of every optimizer's state (training_config, optimizer_weights) through lisec_amd.hdf5_lite."""
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


# ---- the reference: fp64 arithmetic on fp32 inputs; hyper-parameters as the kernels receive them ----------------------
def _f(x):
    return float(np.float32(x))


def keras_sgd(theta, v, g, it, lr, decay, momentum, nesterov):
    """One SGD step (ResourceApplyGradientDescent / ResourceApplyKerasMomentum); it: iterations before the step.
    Returns (theta, v); v is None without momentum."""
    th, g = theta.astype(np.float64), g.astype(np.float64)
    lr_t = lr / (1.0 + decay * it)
    if momentum == 0:
        return th - lr_t * g, None
    m = _f(momentum)
    v = m * v.astype(np.float64) - lr_t * g
    return (th + m * v - lr_t * g if nesterov else th + v), v


def keras_adam(theta, m, v, vhat, g, it, lr, decay, beta_1, beta_2, epsilon, amsgrad):
    """One Adam step (ResourceApplyAdam; amsgrad: vhat <- max(vhat, v) takes v's place).  b1^t, b2^t in fp32 as TF.
    Returns (theta, m, v, vhat); vhat is None without amsgrad."""
    th, g = theta.astype(np.float64), g.astype(np.float64)
    b1, b2, eps = _f(beta_1), _f(beta_2), _f(epsilon)
    t = np.float32(it + 1)
    b1p, b2p = float(np.float32(b1) ** t), float(np.float32(b2) ** t)
    lr_t = lr / (1.0 + decay * it)
    alpha = lr_t * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    m = m.astype(np.float64) + (g - m) * (1.0 - b1)
    v = v.astype(np.float64) + (g * g - v) * (1.0 - b2)
    if amsgrad:
        vhat = np.maximum(vhat.astype(np.float64), v)
        return th - alpha * m / (np.sqrt(vhat) + eps), m, v, vhat
    return th - alpha * m / (np.sqrt(v) + eps), m, v, None


# ---- the reference against torch.optim (eps = 0 / constant lr: the two conventions coincide) --------------------------
@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_reference_matches_torch(amsgrad):
    rng = np.random.default_rng(1)
    n = 1000
    theta = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) * (1 + k) for k in range(6)]
    p = torch.nn.Parameter(torch.from_numpy(theta.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=0.01, betas=(0.9, 0.999), eps=0.0, amsgrad=amsgrad)
    th, m, v = theta.astype(np.float64), np.zeros(n), np.zeros(n)
    vhat = np.zeros(n) if amsgrad else None
    # torch takes betas in double: give the reference the same (no fp32 rounding of b1, b2, b^t)
    for it, g in enumerate(grads):
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        t = it + 1
        alpha = 0.01 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        m = m + (g - m) * (1 - 0.9)
        v = v + (g.astype(np.float64) ** 2 - v) * (1 - 0.999)
        if amsgrad:
            vhat = np.maximum(vhat, v)
        th = th - alpha * m / np.sqrt(vhat if amsgrad else v)
    np.testing.assert_allclose(th, p.detach().numpy(), rtol=1e-12, atol=1e-12)
    # ... and the reference as the GPU tests use it (fp32 hyper-parameters) stays within fp32 rounding of that
    th2, m2, v2 = theta.astype(np.float64), np.zeros(n), np.zeros(n)
    vh2 = np.zeros(n) if amsgrad else None
    for it, g in enumerate(grads):
        th2, m2, v2, vh2 = keras_adam(th2, m2, v2, vh2, g, it, 0.01, 0.0, 0.9, 0.999, 0.0, amsgrad)
    np.testing.assert_allclose(th2, th, rtol=0, atol=1e-6)


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True), (0.5, True)])
def test_sgd_reference_matches_torch(momentum, nesterov):
    rng = np.random.default_rng(2)
    n = 1000
    theta = rng.standard_normal(n).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(theta.astype(np.float64)))
    opt = torch.optim.SGD([p], lr=0.05, momentum=_f(momentum), nesterov=nesterov)
    th, v = theta.astype(np.float64), np.zeros(n)
    for it in range(6):
        g = rng.standard_normal(n).astype(np.float32)
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        th, v = keras_sgd(th, v, g, it, 0.05, 0.0, momentum, nesterov)
        assert (v is None) == (momentum == 0)
    np.testing.assert_allclose(th, p.detach().numpy(), rtol=1e-12, atol=1e-12)


def test_decayed_learning_rate_and_adam_defaults():
    """lr_t = lr / (1 + decay*it) with `it` the count BEFORE the step; the first Adam step moves a variable by
    lr*s/(s + eps), s = sqrt(1 - b2)|g|: about lr, less for gradients near eps/sqrt(1 - b2) (the last one)."""
    g = np.array([2.0, -3.0, 0.5, 1e-3], np.float32)
    th, _ = keras_sgd(np.zeros(4, np.float32), None, g, 10, 0.1, 0.5, 0.0, False)
    np.testing.assert_allclose(th, -(0.1 / 6.0) * g.astype(np.float64), rtol=1e-15)
    th, m, v, _ = keras_adam(np.zeros(4, np.float32), np.zeros(4), np.zeros(4), None, g, 0, 0.001, 0.0, 0.9, 0.999, 1e-7,
                             False)
    s = np.sqrt(1.0 - _f(0.999)) * np.abs(g.astype(np.float64))
    np.testing.assert_allclose(th, -0.001 * np.sign(g) * s / (s + _f(1e-7)), rtol=1e-6)
    assert abs(th[3]) < 0.999 * 0.001


# ---- optimizer objects ------------------------------------------------------------------------------------------------
def test_optimizer_objects_defaults_aliases_and_strings():
    s = mt.optimizers.SGD()
    assert (s.lr, s.decay, s.momentum, s.nesterov) == (0.01, 0.0, 0.0, False)
    assert s.spec() == OptimizerSpec("sgd", 0.01, 0.0, 0.0, False) and s.spec().slots == ()
    s = mt.optimizers.SGD(lr=0.02, decay=1e-6, momentum=0.9)                          # no longer NotImplementedError
    assert s.spec().slots == ("velocity",) and not s.nesterov
    assert mt.optimizers.SGD(learning_rate=0.3).lr == 0.3
    a = mt.optimizers.Adam()
    assert (a.lr, a.decay, a.beta_1, a.beta_2, a.epsilon, a.amsgrad) == (0.001, 0.0, 0.9, 0.999, 1e-7, False)
    assert a.spec().slots == ("m", "v")
    assert mt.optimizers.Adam(lr=0.01).lr == 0.01 and mt.optimizers.Adam(0.02).lr == 0.02
    assert mt.optimizers.Adam(amsgrad=True).spec().slots == ("m", "v", "vhat")
    assert a.get_config() == {"name": "Adam", "learning_rate": 0.001, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.999,
                              "epsilon": 1e-7, "amsgrad": False}
    assert isinstance(mt.optimizers.get("adam"), mt.optimizers.Adam)
    assert isinstance(mt.optimizers.get("SGD"), mt.optimizers.SGD) and mt.optimizers.get("sgd").momentum == 0.0
    assert mt.optimizers.get(a) is a
    with pytest.raises(ValueError):
        mt.optimizers.get("rmsprop")
    with pytest.raises(ValueError):
        mt.optimizers.SGD(momentum=-0.1)
    with pytest.raises(ValueError):
        mt.optimizers.Adam(beta_1=1.0)
    # every hyper-parameter is part of the spec's config (the step-plan key)
    configs = {mt.optimizers.SGD(momentum=0.9, nesterov=True).spec().config, mt.optimizers.SGD(momentum=0.9).spec().config,
               mt.optimizers.SGD().spec().config, mt.optimizers.Adam().spec().config,
               mt.optimizers.Adam(amsgrad=True).spec().config, mt.optimizers.Adam(epsilon=1e-8).spec().config}
    assert len(configs) == 6


@pytest.mark.parametrize("kw", ["clipnorm", "clipvalue", "global_clipnorm"])
def test_gradient_clipping_is_refused(kw):
    for cls in (mt.optimizers.SGD, mt.optimizers.Adam):
        with pytest.raises(NotImplementedError, match="clipping"):
            cls(**{kw: 1.0})
        cls(**{kw: None})                                  # Keras' own default: accepted
    with pytest.raises(TypeError):
        mt.optimizers.Adam(no_such_argument=1)


# ---- Keras .h5 layout of the optimizer state --------------------------------------------------------------------------
CONFIGS = {
    "sgd": dict(lr=0.05, decay=1e-4, momentum=0.0, nesterov=False),
    "momentum": dict(lr=0.01, decay=1e-6, momentum=0.8, nesterov=False),
    "adam": dict(class_name="Adam", lr=0.002, decay=1e-5, beta_1=0.85, beta_2=0.995, epsilon=1e-6, amsgrad=False),
    "amsgrad": dict(class_name="Adam", lr=0.001, decay=0.0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=True),
}
KINDS = {"sgd": (), "momentum": ("momentum",), "adam": ("m", "v"), "amsgrad": ("m", "v", "vhat")}


def _write(tmp_path, which):
    params = glorot_numpy(seed=3)
    rng = np.random.default_rng(4)
    trainable = [n for n, _, k in param_specs() if k in TRAINABLE_KINDS]
    shapes = {n: s for n, s, _ in param_specs()}
    slots = {k: {n: rng.standard_normal(shapes[n]).astype(np.float32) for n in trainable}
             for k in ("velocity", "m", "v", "vhat")}
    kw = {}
    for k in KINDS[which]:
        key = "velocity" if k == "momentum" else k
        kw[key] = slots[key]
    path = str(tmp_path / f"{which}.h5")
    keras_h5.save_model(path, params, 16, 32, 8, 35, optimizer=CONFIGS[which], iterations=37, **kw)
    return path, params, slots


@pytest.mark.parametrize("which", list(CONFIGS))
def test_keras_h5_round_trip_of_optimizer_state(tmp_path, which):
    path, params, slots = _write(tmp_path, which)
    cfg = CONFIGS[which]
    cls = cfg.get("class_name", "SGD")
    with hdf5_lite.File(path) as f:
        tc = json.loads(bytes(f.attrs["training_config"]).decode())["optimizer_config"]
        names = [bytes(n).decode() for n in np.asarray(f["optimizer_weights"].attrs["weight_names"]).ravel()]
        assert int(f["optimizer_weights"][f"{cls}/iter:0"][()]) == 37
    assert tc["class_name"] == cls
    if cls == "Adam":
        assert tc["config"] == {"name": "Adam", "learning_rate": cfg["lr"], "decay": cfg["decay"], "beta_1": cfg["beta_1"],
                                "beta_2": cfg["beta_2"], "epsilon": cfg["epsilon"], "amsgrad": cfg["amsgrad"]}
    else:
        assert tc["config"] == {"name": "SGD", "learning_rate": cfg["lr"], "decay": cfg["decay"],
                                "momentum": cfg["momentum"], "nesterov": cfg["nesterov"]}
    # Keras' order: iter, then one slot kind for every trainable variable, then the next kind
    layers, _ = keras_h5.keras_layers(16, 32, 8, 35)
    variables = [f"{L['name']}/{w}" for L in layers for w, _ in L["weights"] if w in ("kernel", "bias", "gamma", "beta")]
    n_var = len([n for n, _, k in param_specs() if k in TRAINABLE_KINDS])
    assert len(variables) == n_var
    assert names == [f"{cls}/iter:0"] + [f"{cls}/{var}/{k}:0" for k in KINDS[which] for var in variables]
    ck = keras_h5.load_model(path)
    assert ck["iterations"] == 37 and ck["optimizer"] == cfg
    for k in ("velocity", "m", "v", "vhat"):
        kept = ("momentum" if k == "velocity" else k) in KINDS[which]
        assert (ck[k] is not None) == kept, k
        if kept:
            assert set(ck[k]) == set(slots[k])
            for n in slots[k]:
                np.testing.assert_array_equal(ck[k][n], slots[k][n])
    for n in params:
        np.testing.assert_array_equal(ck["params"][n], params[n])


def test_keras_h5_reader_matches_slots_by_name(tmp_path):
    """A file whose optimizer_weights list the slots in another order reads back the same (matched by name)."""
    path, _, slots = _write(tmp_path, "amsgrad")
    shuffled = str(tmp_path / "shuffled.h5")
    with hdf5_lite.File(path) as src, hdf5_lite.File(shuffled, "w") as dst:
        for k in ("keras_version", "backend", "model_config", "training_config"):
            dst.attrs[k] = src.attrs[k]
        g = dst.create_group("model_weights")
        for k in ("layer_names", "backend", "keras_version"):
            g.attrs[k] = src["model_weights"].attrs[k]
        for lname in [bytes(n).decode() for n in src["model_weights"].attrs["layer_names"]]:
            lg = g.create_group(lname)
            wn = [bytes(w).decode() for w in np.asarray(src["model_weights"][lname].attrs["weight_names"]).ravel()]
            lg.attrs["weight_names"] = [w.encode() for w in wn]
            for w in wn:
                lg.create_dataset(w, data=src["model_weights"][lname][w][()])
        names = [bytes(n).decode() for n in np.asarray(src["optimizer_weights"].attrs["weight_names"]).ravel()]
        rev = names[::-1]
        og = dst.create_group("optimizer_weights")
        og.attrs["weight_names"] = [n.encode() for n in rev]
        for n in rev:
            og.create_dataset(n, data=src["optimizer_weights"][n][()])
    ck = keras_h5.load_model(shuffled)
    assert ck["iterations"] == 37
    for k in ("m", "v", "vhat"):
        for n in slots[k]:
            np.testing.assert_array_equal(ck[k][n], slots[k][n])


def test_save_model_keeps_its_sgd_nesterov_signature(tmp_path):
    """save_model(..., optimizer=dict(lr, decay, momentum, nesterov), iterations, velocity) as before; without the
    velocity a momentum optimizer writes no optimizer_weights (as before), SGD without momentum needs no slot."""
    params = glorot_numpy(seed=5)
    path = str(tmp_path / "nov.h5")
    keras_h5.save_model(path, params, 16, 32, 8, 35, optimizer=dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True),
                        iterations=3)
    ck = keras_h5.load_model(path)
    assert ck["optimizer"] == dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True) and ck["velocity"] is None
    assert ck["iterations"] == 0


def _have_h5py():
    if not os.path.exists(H5PY_PYTHON):
        return False
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    return subprocess.run([H5PY_PYTHON, "-c", "import h5py"], env=env, capture_output=True).returncode == 0


@pytest.mark.parametrize("which", ["adam", "amsgrad"])
def test_adam_file_reads_with_h5py(tmp_path, which):
    path, _, slots = _write(tmp_path, which)
    if not _have_h5py():
        return                                             # the hdf5_lite round trip above still ran; no h5py here
    import hashlib
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    out = subprocess.run([H5PY_PYTHON, PROBE, "dump", path], env=env, capture_output=True, check=True).stdout
    desc = json.loads(out)
    og = desc["/optimizer_weights"]
    names = og["attrs"]["weight_names"]["value"]
    assert names[0] == "Adam/iter:0" and len(names) == 1 + len(KINDS[which]) * len(slots["m"])
    assert names[1].endswith("/m:0") and names[-1].endswith("/vhat:0" if which == "amsgrad" else "/v:0")
    tc = json.loads(desc["/"]["attrs"]["training_config"]["value"])
    assert tc["optimizer_config"]["class_name"] == "Adam"
    assert tc["optimizer_config"]["config"]["amsgrad"] == (which == "amsgrad")
    ck = keras_h5.load_model(path)
    layers, _ = keras_h5.keras_layers(16, 32, 8, 35)
    to_param = {f"{L['name']}/{w}": p for L in layers for w, p in L["weights"]}
    for n in names[1:]:
        var, kind = n[len("Adam/"):].rsplit("/", 1)
        a = ck[kind[:-2]][to_param[var]]
        d = desc["/optimizer_weights/" + n]
        assert d["dtype"] == "<f4" and d["sha"] == hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
