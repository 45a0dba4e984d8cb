"""tf.keras 2.4 losses, loss_weights and metrics of Model.compile without a GPU: an fp64 numpy transcription of every
loss, metric and loss gradient (shared with tests/test_gpu_losses.py), pinned against torch.nn.functional and torch
autograd of the same formulas; compile()'s argument parsing, metric names and refusals; (de)serialization; and the
training_config that keras_h5.save_model writes."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lisec_amd import keras_h5, losses
from lisec_amd import model_training as mt
from lisec_amd.params import glorot_numpy

EPS = 1e-7
H5PY_PYTHON = "/opt/conda/bin/python3.9"          # the interpreter with h5py that tests/test_hdf5_lite.py uses
PROBE = os.path.join(os.path.dirname(__file__), "golden", "h5py_probe.py")
K = losses


# ---- the reference: Keras 2.4's formulas in fp64 ------------------------------------------------------------------------
def ref_elem(term, p, t):
    """(value, d value / d p) per element of a loss / elementwise metric term (kind, from_logits, param, label_smoothing),
    TF's gradient conventions: d|x| = sign(x), sign(0) = 0; Maximum passes the gradient to x where x >= y; clip_by_value
    where min <= x <= max; where_v2 takes the branch its condition picks."""
    kind, logits, prm, ls = term
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    e = p - t
    with np.errstate(all="ignore"):
        if kind == K.MSE:
            return e * e, 2 * e
        if kind == K.MAE:
            return np.abs(e), np.sign(e)
        if kind == K.MAPE:
            d = np.maximum(np.abs(t), EPS)
            return 100 * np.abs((t - p) / d), -100 * np.sign(t - p) / d
        if kind == K.MSLE:
            a = np.maximum(p, EPS)
            diff = np.log1p(a) - np.log1p(np.maximum(t, EPS))
            return diff * diff, np.where(p >= EPS, 2 * diff / (a + 1), 0.0)
        if kind == K.HUBER:
            ae = np.abs(e)
            return (np.where(ae <= prm, 0.5 * e * e, 0.5 * prm * prm + prm * (ae - prm)),
                    np.where(ae <= prm, e, prm * np.sign(e)))
        if kind == K.LOGCOSH:
            z = -2 * e
            return e + np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - np.log(2.0), np.tanh(e)
        if kind == K.BCE:
            ts = t * (1 - ls) + 0.5 * ls
            if logits:
                # nn.sigmoid_cross_entropy_with_logits: where(p >= 0, p, 0) - p t + log1p(exp(where(p >= 0, -p, p)))
                return np.maximum(p, 0) - p * ts + np.log1p(np.exp(-np.abs(p))), 1 / (1 + np.exp(-p)) - ts
            o = np.clip(p, EPS, 1 - EPS)
            inside = (p >= EPS) & (p <= 1 - EPS)
            return (-(ts * np.log(o + EPS) + (1 - ts) * np.log(1 - o + EPS)),
                    np.where(inside, -(ts / (o + EPS) - (1 - ts) / (1 - o + EPS)), 0.0))
        if kind == K.POISSON:
            return p - t * np.log(p + EPS), 1 - t / (p + EPS)
        if kind == K.SIGMOID_CE_CLAMPED:
            tt = np.clip(t, 0, 1)
            return np.maximum(p, 0) - p * tt + np.log1p(np.exp(-np.abs(p))), 1 / (1 + np.exp(-p)) - tt
        if kind == K.SMOOTH_L1:
            ae = np.abs(e)
            return np.where(ae < 1, 0.5 * e * e, ae - 0.5), np.where(ae < 1, e, np.sign(e))
        if kind == K.BINARY_ACCURACY:
            return (t == (p > np.float32(prm)).astype(np.float64)).astype(np.float64), None
    raise ValueError(kind)


def ref_metric(term, p, t):
    """The per-sweep value of a metric on one output (p, t: (M, C))."""
    if term[0] == K.CATEGORICAL_ACCURACY:
        return float(np.mean(np.argmax(p, -1) == np.argmax(t, -1)))
    return float(np.mean(ref_elem(term, p, t)[0]))


def ref_head_loss(spec, head, yc, yr, grad_scale=1.0):
    """fp64 (loss_out [total, cls, reg], metrics in metrics_names order, dhead (M,16)) of a LossSpec."""
    head = np.asarray(head, np.float64).reshape(-1, 16)
    outs = [(head[:, :2], np.asarray(yc, np.float64).reshape(-1, 2)), (head[:, 2:], np.asarray(yr, np.float64).reshape(-1, 14))]
    vals, grads, mets = [], [], []
    for o, (p, t) in enumerate(outs):
        v, g = ref_elem(spec.losses[o], p, t)
        vals.append(v.mean())
        grads.append(grad_scale * spec.weights[o] * g / v.size)
        mets += [ref_metric(m, p, t) for m in spec.metrics[o]]
    total = spec.weights[0] * vals[0] + spec.weights[1] * vals[1]
    return np.array([total, vals[0], vals[1]]), np.array(mets), np.concatenate(grads, 1)


# ---- torch forms of the same formulas (autograd is the independent differentiation) ------------------------------------
def torch_elem(term, p, t):
    kind, logits, prm, ls = term
    e = p - t
    eps = torch.tensor(EPS, dtype=p.dtype)
    if kind == K.MSE:
        return e * e
    if kind == K.MAE:
        return torch.abs(e)
    if kind == K.MAPE:
        return 100 * torch.abs((t - p) / torch.clamp(torch.abs(t), min=EPS))
    if kind == K.MSLE:
        a = torch.where(p >= eps, p, eps)
        return (torch.log(a + 1) - torch.log(torch.clamp(t, min=EPS) + 1)) ** 2
    if kind == K.HUBER:
        ae = torch.abs(e)
        return torch.where(ae <= prm, 0.5 * e ** 2, 0.5 * prm ** 2 + prm * (ae - prm))
    if kind == K.LOGCOSH:
        return e + F.softplus(-2 * e) - np.log(2.0)
    if kind == K.BCE:
        ts = t * (1 - ls) + 0.5 * ls
        if logits:
            cond = p >= 0
            return torch.where(cond, p, torch.zeros_like(p)) - p * ts + torch.log1p(torch.exp(torch.where(cond, -p, p)))
        inside = (p >= EPS) & (p <= 1 - EPS)
        o = torch.where(inside, p, torch.clamp(p, EPS, 1 - EPS).detach())
        return -(ts * torch.log(o + EPS) + (1 - ts) * torch.log(1 - o + EPS))
    if kind == K.POISSON:
        return p - t * torch.log(p + EPS)
    raise ValueError(kind)


HUBER_D = 0.5
TERMS = {"mse": (K.MSE, 0, 0.0, 0.0), "mae": (K.MAE, 0, 0.0, 0.0), "mape": (K.MAPE, 0, 0.0, 0.0),
         "msle": (K.MSLE, 0, 0.0, 0.0), "huber": (K.HUBER, 0, HUBER_D, 0.0), "logcosh": (K.LOGCOSH, 0, 0.0, 0.0),
         "bce": (K.BCE, 0, 0.0, 0.0), "bce_ls": (K.BCE, 0, 0.0, 0.2), "bce_logits": (K.BCE, 1, 0.0, 0.0),
         "bce_logits_ls": (K.BCE, 1, 0.0, 0.1), "poisson": (K.POISSON, 0, 0.0, 0.0)}


def edge_data(seed=0, n=400):
    """Random pairs plus the edge cases: e == 0, |e| == delta, negative p, |t| < eps, p outside [eps, 1-eps], labels 2, -1."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 1.5, n).astype(np.float32)
    t = rng.choice([0.0, 1.0, 2.0, -1.0, 0.3], n).astype(np.float32)
    t[: n // 4] = rng.normal(0, 1, n // 4)
    extra_p = [0.7, 1.5, -1.0, 0.25, -0.3, -2e-8, 3e-8, 1.2, 1 - 1e-8, 0.0, 5e-8, 2.0, 0.5, -0.5]
    extra_t = [0.7, 1.0, -0.5, 0.75, 1.0, 0.4, 1e-8, 2.0, 1.0, 1.0, -5e-9, -1.0, 0.0, 0.0]
    return np.concatenate([p, np.float32(extra_p)]), np.concatenate([t, np.float32(extra_t)])


def test_edge_data_holds_the_edge_cases():
    p, t = edge_data()
    e = p.astype(np.float64) - t
    assert (e == 0).any() and (np.abs(e) == HUBER_D).any() and (p < 0).any() and (np.abs(t) < EPS).any()
    assert ((p < EPS) | (p > 1 - EPS)).any() and (t == 2).any() and (t == -1).any()


@pytest.mark.parametrize("name", sorted(TERMS))
def test_reference_matches_torch_autograd_of_the_formula(name):
    term = TERMS[name]
    p, t = edge_data(1)
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    v = torch_elem(term, pt, torch.from_numpy(t.astype(np.float64)))
    v.sum().backward()
    rv, rg = ref_elem(term, p, t)
    np.testing.assert_allclose(rv, v.detach().numpy(), rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(rg, pt.grad.numpy(), rtol=1e-12, atol=1e-12, equal_nan=True)


def _functional(name, p, t):
    if name == "mse":
        return F.mse_loss(p, t)
    if name == "mae":
        return F.l1_loss(p, t)
    if name == "huber":
        return F.huber_loss(p, t, delta=HUBER_D)
    if name == "bce_logits":
        return F.binary_cross_entropy_with_logits(p, t)
    if name == "poisson":
        return F.poisson_nll_loss(p, t, log_input=False, eps=EPS, full=False)


@pytest.mark.parametrize("name", ["mse", "mae", "huber", "bce_logits", "poisson"])
def test_reference_mean_and_gradient_match_torch_functional(name):
    p, t = edge_data(2)
    if name == "poisson":
        p = np.abs(p) + np.float32(0.01)             # torch and Keras agree where log(p + eps) is defined
    if name == "mae":
        p[t == p] += np.float32(0.5)                 # F.l1_loss differentiates |0| as 0 too; keep the sign test elsewhere
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    tt = torch.from_numpy(t.astype(np.float64))
    v = _functional(name, pt, tt)
    v.backward()
    rv, rg = ref_elem(TERMS[name], p, t)
    np.testing.assert_allclose(rv.mean(), v.item(), rtol=1e-12)
    np.testing.assert_allclose(rg / rv.size, pt.grad.numpy(), rtol=1e-10, atol=1e-15)


def test_reference_gradient_conventions():
    """sign(0) = 0, the quadratic branch at |e| == delta, no gradient outside the BCE clip / below eps for msle."""
    v, g = ref_elem(TERMS["mae"], np.float32([1.0]), np.float32([1.0]))
    assert g[0] == 0
    v, g = ref_elem(TERMS["huber"], np.float32([1.5, -0.5]), np.float32([1.0, 0.0]))
    assert np.allclose(g, [0.5, -0.5]) and np.allclose(v, [0.125, 0.125])
    _, g = ref_elem(TERMS["bce"], np.float32([1.2, -0.1, 0.0]), np.float32([1.0, 0.0, 1.0]))
    assert (g == 0).all()
    _, g = ref_elem(TERMS["msle"], np.float32([-1.0, 0.0]), np.float32([0.5, 0.5]))
    assert (g == 0).all()
    _, g = ref_elem(TERMS["bce_logits"], np.float32([0.0]), np.float32([1.0]))
    assert g[0] == -0.5                               # sigmoid(0) - t: TF's where-form of the logits loss
    v, _ = ref_elem((K.BINARY_ACCURACY, 0, 0.0, 0.0), np.float32([0.1, -0.1, 3.0, 0.0]), np.float32([1, 0, 2, 0]))
    assert list(v) == [1, 1, 0, 1]
    assert ref_metric((K.CATEGORICAL_ACCURACY, 0, 0, 0), np.float64([[1, 1], [0, 2]]), np.float64([[2, 2], [1, 0]])) == 0.5


# ---- compile() arguments ------------------------------------------------------------------------------------------------
def test_legacy_spellings_keep_the_legacy_step():
    for loss in (["mse", "mse"], ("MSE", "mse"), "mse", "mean_squared_error", K.MeanSquaredError(),
                 {"ClassificationLayer": "mse", "RegressionLayer": K.MeanSquaredError()}):
        assert K.compile_loss(loss) == ("mse", [])
    for loss in ("smoothl1_ce", ["smoothl1_ce"], ["cross_entropy", "smooth_l1"], ["Cross_Entropy", "Smooth_L1"]):
        assert K.compile_loss(loss) == ("smoothl1_ce", [])
    assert K.compile_loss(["mse", "mse"], metrics=[]) == ("mse", [])


def test_legacy_spelling_with_weights_or_metrics_goes_through_head_loss():
    spec, names = K.compile_loss(["mse", "mse"], loss_weights=[1.0, 1.0])
    assert isinstance(spec, K.LossSpec) and spec.losses == (TERMS["mse"], TERMS["mse"]) and names == []
    spec, names = K.compile_loss("smoothl1_ce", metrics=["mae"])
    assert spec.losses == ((K.SIGMOID_CE_CLAMPED, 0, 0.0, 0.0), (K.SMOOTH_L1, 0, 0.0, 0.0))
    assert names == ["ClassificationLayer_mae", "RegressionLayer_mae"]


def test_every_loss_form():
    bce, hub = K.BinaryCrossentropy(from_logits=True, label_smoothing=0.1), K.Huber(delta=0.5)
    want = ((K.BCE, 1, 0.0, 0.1), (K.HUBER, 0, 0.5, 0.0))
    for loss in ([bce, hub], (bce, hub), {"RegressionLayer": hub, "ClassificationLayer": bce}):
        spec, _ = K.compile_loss(loss, loss_weights=[2.0, 0.5])
        assert spec.losses == want and spec.weights == (2.0, 0.5)
    names = {"mae": K.MAE, "mean_absolute_error": K.MAE, "mape": K.MAPE, "mean_absolute_percentage_error": K.MAPE,
             "msle": K.MSLE, "mean_squared_logarithmic_error": K.MSLE, "huber": K.HUBER, "logcosh": K.LOGCOSH,
             "log_cosh": K.LOGCOSH, "binary_crossentropy": K.BCE, "poisson": K.POISSON}
    for n, kind in names.items():
        spec, _ = K.compile_loss(n)
        assert spec.losses[0][0] == spec.losses[1][0] == kind
    assert K.compile_loss("huber")[0].losses[0] == (K.HUBER, 0, 1.0, 0.0)
    for cls, kind in ((K.MeanAbsoluteError, K.MAE), (K.MeanAbsolutePercentageError, K.MAPE),
                      (K.MeanSquaredLogarithmicError, K.MSLE), (K.LogCosh, K.LOGCOSH), (K.Poisson, K.POISSON),
                      (K.BinaryCrossentropy, K.BCE), (K.Huber, K.HUBER)):
        assert K.compile_loss(["mse", cls()])[0].losses[1][0] == kind


def test_loss_weights_list_and_dict():
    assert K.compile_loss("mae", loss_weights=[3, 0.25])[0].weights == (3.0, 0.25)
    assert K.compile_loss("mae", loss_weights={"RegressionLayer": 4.0})[0].weights == (1.0, 4.0)
    assert K.compile_loss("mae", loss_weights={"ClassificationLayer": 2, "RegressionLayer": 0.5})[0].weights == (2.0, 0.5)


def test_metric_forms_names_and_order():
    M = mt.metrics
    _, names = K.compile_loss("mse", metrics=["mae", "accuracy"])
    assert names == ["ClassificationLayer_mae", "ClassificationLayer_accuracy", "RegressionLayer_mae",
                     "RegressionLayer_accuracy"]
    spec, names = K.compile_loss("mse", metrics=[[M.BinaryAccuracy(threshold=0.0), "acc"], ["mse", M.MeanAbsoluteError()]])
    assert names == ["ClassificationLayer_binary_accuracy", "ClassificationLayer_acc", "RegressionLayer_mse",
                     "RegressionLayer_mean_absolute_error"]
    assert spec.metrics == (((K.BINARY_ACCURACY, 0, 0.0, 0.0), (K.CATEGORICAL_ACCURACY, 0, 0.0, 0.0)),
                            ((K.MSE, 0, 0.0, 0.0), (K.MAE, 0, 0.0, 0.0)))
    spec, names = K.compile_loss("mse", metrics={"RegressionLayer": "mae",
                                                 "ClassificationLayer": [M.BinaryCrossentropy(from_logits=True),
                                                                         "binary_accuracy", M.MeanSquaredError()]})
    assert names == ["ClassificationLayer_binary_crossentropy", "ClassificationLayer_binary_accuracy",
                     "ClassificationLayer_mean_squared_error", "RegressionLayer_mae"]
    assert spec.metrics[0][0] == (K.BCE, 1, 0.0, 0.0) and spec.metrics[0][1] == (K.BINARY_ACCURACY, 0, 0.5, 0.0)
    for s in ("mse", "mae", "mape", "msle", "logcosh", "binary_crossentropy", "poisson", "binary_accuracy",
              "categorical_accuracy"):
        assert K.compile_loss("mse", metrics=[s])[1] == [f"ClassificationLayer_{s}", f"RegressionLayer_{s}"]
    assert K.compile_loss("mse", metrics=["binary_crossentropy"])[0].metrics[0][0] == (K.BCE, 0, 0.0, 0.0)
    assert K.compile_loss("mse", metrics=[M.BinaryAccuracy(name="hit")])[1][0] == "ClassificationLayer_hit"


def test_refusals():
    with pytest.raises(ValueError):
        K.compile_loss("nope")
    with pytest.raises(ValueError):
        K.compile_loss({"ClassificationLayer": "mse", "Regression": "mse"})
    with pytest.raises(ValueError):
        K.compile_loss(["mse", "mse", "mse"])
    with pytest.raises(ValueError):
        K.compile_loss("mse", loss_weights=[1.0])
    with pytest.raises(ValueError):
        K.compile_loss("mse", loss_weights={"Other": 1.0})
    with pytest.raises(ValueError):
        K.compile_loss("mse", metrics=["nope"])
    with pytest.raises(ValueError):
        K.compile_loss("mse", metrics={"Other": ["mae"]})
    with pytest.raises(ValueError):
        K.compile_loss("mse", metrics=[["mae"], ["mae"], ["mae"]])
    with pytest.raises(ValueError):
        K.compile_loss("mse", metrics=["mae", "mse", "mape", "msle", "poisson"])
    for loss in ("hinge", "squared_hinge", "categorical_crossentropy", "sparse_categorical_crossentropy", "kld",
                 "cosine_similarity", K.Hinge(), K.CategoricalCrossentropy(), K.KLDivergence(), K.CosineSimilarity(),
                 lambda y_true, y_pred: y_pred, None, ["mse", None], {"ClassificationLayer": "mse"}):
        with pytest.raises(NotImplementedError):
            K.compile_loss(loss)

    class Mine(K.MeanSquaredError):
        pass

    with pytest.raises(NotImplementedError):
        K.compile_loss(Mine())
    for m in ("categorical_crossentropy", "hinge", "top_k_categorical_accuracy", "auc", lambda a, b: a):
        with pytest.raises(NotImplementedError):
            K.compile_loss("mse", metrics=[m])
    with pytest.raises(NotImplementedError):
        K.compile_loss("mse", weighted_metrics=["mae"])
    with pytest.raises(TypeError):
        K.compile_loss("mse", metrics="mae")
    assert K.compile_loss("mse", weighted_metrics=None) == ("mse", [])
    with pytest.raises(ValueError):
        K.Huber(delta=0)
    with pytest.raises(ValueError):
        mt.optimizers.get("rmsprop")


def test_serialize_round_trips():
    for obj in (K.MeanSquaredError(), K.MeanAbsoluteError(), K.MeanAbsolutePercentageError(),
                K.MeanSquaredLogarithmicError(), K.Huber(delta=0.25), K.LogCosh(), K.Poisson(),
                K.BinaryCrossentropy(from_logits=True, label_smoothing=0.1)):
        ser = K.serialize(obj)
        assert ser["config"]["reduction"] == "auto" and ser["config"]["name"] == obj.name
        back = K.deserialize(json.loads(json.dumps(ser)))
        assert type(back) is type(obj) and back.get_config() == obj.get_config() and back.term() == obj.term()
        assert K.get(ser).term() == obj.term()
    assert K.serialize(K.Huber(0.5)) == {"class_name": "Huber", "config": {"reduction": "auto", "name": "huber_loss",
                                                                             "delta": 0.5}}
    assert K.serialize("mae") == "mae" and K.deserialize("mae") == "mae"
    M = mt.metrics
    for obj in (M.BinaryAccuracy(threshold=0.0), M.BinaryCrossentropy(from_logits=True, label_smoothing=0.2),
                M.MeanAbsoluteError(), M.MeanSquaredError()):
        ser = M.serialize(obj)
        back = M.deserialize(json.loads(json.dumps(ser)))
        assert type(back) is type(obj) and back.get_config() == obj.get_config() and back.term() == obj.term()
    assert M.serialize(M.BinaryAccuracy(threshold=0.0)) == {
        "class_name": "BinaryAccuracy", "config": {"name": "binary_accuracy", "dtype": "float32", "threshold": 0.0}}
    with pytest.raises(ValueError):
        K.deserialize({"class_name": "Nope", "config": {}})
    with pytest.raises(ValueError):
        M.deserialize({"class_name": "Nope", "config": {}})


def test_spec_is_hashable_and_descriptor_holds_it():
    a, _ = K.compile_loss([K.BinaryCrossentropy(from_logits=True), K.Huber(0.5)], loss_weights=[2, 0.5],
                          metrics=[["binary_accuracy"], ["mae", "accuracy"]])
    b, _ = K.compile_loss({"ClassificationLayer": "binary_crossentropy", "RegressionLayer": K.Huber(0.5)},
                          loss_weights=[2, 0.5], metrics=[["binary_accuracy"], ["mae", "accuracy"]])
    assert a != b
    c, _ = K.compile_loss([K.BinaryCrossentropy(from_logits=True), K.Huber(0.5)], loss_weights={"ClassificationLayer": 2,
                          "RegressionLayer": 0.5}, metrics={"ClassificationLayer": "binary_accuracy",
                                                            "RegressionLayer": ["mae", "acc"]})
    assert a == c and hash(a) == hash(c) and a.n_metrics == 3
    d = a.descriptor()
    assert (d.loss[0].kind, d.loss[0].from_logits, d.loss[1].kind, d.loss[1].param) == (K.BCE, 1, K.HUBER, 0.5)
    assert list(d.weight) == [2.0, 0.5] and list(d.n_metrics) == [1, 2]
    assert (d.metric[0][0].kind, d.metric[0][0].param, d.metric[1][1].kind) == (K.BINARY_ACCURACY, 0.5,
                                                                                K.CATEGORICAL_ACCURACY)


def test_model_training_exposes_the_modules_and_compile_signature():
    import inspect
    assert mt.losses is losses and mt.metrics.BinaryAccuracy
    params = list(inspect.signature(mt.Model.compile).parameters)
    assert params == ["self", "optimizer", "loss", "metrics", "loss_weights", "weighted_metrics"]


# ---- training_config ----------------------------------------------------------------------------------------------------
SGD = dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)


def _write(tmp_path, name, **kw):
    path = str(tmp_path / f"{name}.h5")
    keras_h5.save_model(path, glorot_numpy(seed=3), 16, 32, 8, 35, optimizer=SGD, iterations=0, **kw)
    return path


def _have_h5py():
    if not os.path.exists(H5PY_PYTHON):
        return False
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    return subprocess.run([H5PY_PYTHON, "-c", "import h5py"], env=env, capture_output=True).returncode == 0


def test_default_training_config_file_is_byte_identical(tmp_path):
    a, b = _write(tmp_path, "a"), _write(tmp_path, "b", loss=None, loss_weights=None, metrics=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    ck = keras_h5.load_model(a)
    assert ck["loss"] == ["mse", "mse"] and ck["loss_weights"] is None and ck["metrics"] is None


def test_training_config_of_keras_losses_and_metrics(tmp_path):
    M = mt.metrics
    loss = [K.BinaryCrossentropy(from_logits=True), "huber"]
    metrics = {"ClassificationLayer": [M.BinaryAccuracy(threshold=0.0)], "RegressionLayer": ["mae", M.MeanSquaredError()]}
    path = _write(tmp_path, "k", loss=loss, loss_weights=[2.0, 0.5], metrics=metrics)
    want_loss = [{"class_name": "BinaryCrossentropy", "config": {"reduction": "auto", "name": "binary_crossentropy",
                                                                 "from_logits": True, "label_smoothing": 0}}, "huber"]
    want_metrics = {"ClassificationLayer": [{"class_name": "BinaryAccuracy", "config": {
        "name": "binary_accuracy", "dtype": "float32", "threshold": 0.0}}], "RegressionLayer": [
        "mae", {"class_name": "MeanSquaredError", "config": {"name": "mean_squared_error", "dtype": "float32"}}]}
    from lisec_amd import hdf5_lite
    with hdf5_lite.File(path) as f:
        tc = json.loads(bytes(f.attrs["training_config"]).decode())
    assert list(tc) == ["loss", "metrics", "weighted_metrics", "loss_weights", "optimizer_config"]
    assert tc["loss"] == want_loss and tc["metrics"] == want_metrics and tc["loss_weights"] == [2.0, 0.5]
    assert tc["weighted_metrics"] is None
    ck = keras_h5.load_model(path)
    assert ck["loss"] == want_loss and ck["metrics"] == want_metrics and ck["loss_weights"] == [2.0, 0.5]
    # what load_model re-compiles from it
    spec, names = K.compile_loss(mt._deserialize_nested(ck["loss"], K.deserialize), ck["loss_weights"],
                                 mt._deserialize_nested(ck["metrics"], mt.metrics.deserialize))
    assert spec == K.compile_loss(loss, [2.0, 0.5], metrics)[0]
    assert names == ["ClassificationLayer_binary_accuracy", "RegressionLayer_mae", "RegressionLayer_mean_squared_error"]
    if not _have_h5py():
        return                                             # the hdf5_lite round trip above still ran; no h5py here
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    out = subprocess.run([H5PY_PYTHON, PROBE, "dump", path], env=env, capture_output=True, check=True).stdout
    desc = json.loads(out)
    tc = json.loads(desc["/"]["attrs"]["training_config"]["value"])
    assert tc["loss"] == want_loss and tc["metrics"] == want_metrics and tc["loss_weights"] == [2.0, 0.5]
