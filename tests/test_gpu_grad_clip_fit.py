"""Gradient clipping in the training step on the small grid of the optimizer tests (createModel(16, 32, 8, 35)): one eager
step against the numpy definition (tests/grad_clip_ref.py) followed by the optimizer's own reference, on the step's own
gradient, at a threshold that clips and at one that does not; gradient_norms(); the recorded plans against the Python
schedule; a mini-batch; AdamW, LAMB and an averaging wrapper; save / load_model in the middle of a run; the plan sizes."""
import numpy as np
import pytest

import grad_clip_ref as R
from test_gpu_batch_fit import PARENT_LAUNCHES, _tuning
from test_gpu_optimizers import _data, _make_opt, _targets  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
EAGER, RECORDED, PIPELINED = "step_plan=0", "pipeline_voxels=0", ""
KEYS = {"value": "clipvalue", "norm": "clipnorm", "global_norm": "global_clipnorm"}
# thresholds for the runs that cannot measure first: far below what these gradients have (asserted where they are used)
FIXED = {"value": 1e-4, "norm": 0.01, "global_norm": 0.05}
# what a clipping kind adds to the plan of an Adam step (two update launches: the early part and the rest).  value: one
# launch in front of each part; norm: three in front of each; global_norm: the early update is not made (one launch
# less) and the one update has the partials, the finish and the apply pass in front of it
CLIP_LAUNCHES = {"value": 2, "norm": 6, "global_norm": 2}


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _model(regularized=False):
    from lisec_amd import model_training as mt
    kw = dict(kernel_regularizer=mt.regularizers.l2(1e-4)) if regularized else {}
    return mt.createModel(16, 32, 8, 35, **kw)


def _clipped(opt, kind=None, c=None):
    from lisec_amd import model_training as mt
    return opt if kind is None else mt.optimizers.clip_gradients(opt, **{KEYS[kind]: c})


def _spans(net):
    """[(offset, padded count)] of the trainable variables, as the chunk table has them, and their names."""
    p = net.params
    names = p.trainable_names()
    return [(p.offsets[n][1], (int(np.prod(p.offsets[n][2])) + 3) // 4 * 4) for n in names], names


def _measure(kind, g, spans):
    """What the threshold of a kind is compared with, on the gradient g: the largest element, the largest norm of a
    variable, the norm of everything."""
    if kind == "value":
        return float(np.abs(g).max())
    sums = [R.sum_squares(g[o:o + n]) for o, n in spans]
    return float(np.sqrt(max(sums))) if kind == "norm" else float(np.sqrt(np.sum(sums)))


def _eager_step(opt_name, regularized, kind=None, c=None):
    """The step as fit() splits it (the early update of the RPN tail at backward's hook, then the rest) at iteration 4
    from non-zero slots, the same ones at every call."""
    import torch
    from lisec_amd import model_training as mt
    with _tuning(EAGER):
        model = _model(regularized)
        o = _clipped(_make_opt(opt_name), kind, c)
        model.compile(optimizer=o, loss=['mse', 'mse'])
        net, spec = model.net, o.spec()
        net.iterations = 4
        torch.manual_seed(3)
        for name in spec.slots:
            net.slot(name).copy_(torch.rand_like(net.params.theta) * 1e-3)
        theta0 = net.params.theta.cpu().numpy().copy()
        slots0 = [net.slot(name).cpu().numpy().copy() for name in spec.slots]
        x, y = _data(mt, False, n=1)
        yc, yr = (torch.from_numpy(a[0]).to(net.device) for a in y)
        net.forward(x[0].sample, training=True)
        net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
        pending = net._early is not None
        net.apply_gradients(opt=spec)
        torch.cuda.synchronize()
        assert net.iterations == 5 and net._iter_dev.cpu().tolist() == [5, 0]
        return dict(model=model, net=net, o=o, spec=spec, theta0=theta0, slots0=slots0, pending=pending,
                    grad=net.grad.cpu().numpy().copy(), theta=_bits(net.params.theta),
                    slots=[_bits(net.slot(name)) for name in spec.slots])


_BASE = {}


def _base(opt_name, regularized):
    """The same step without clipping, once per (optimizer, regularizer): net.grad after it is the gradient the update
    used -- backward()'s own, plus the penalty term where the net has a regularizer --, which is what a clipped step clips."""
    key = (opt_name, regularized)
    if key not in _BASE:
        r = _eager_step(opt_name, regularized)
        assert r["pending"] and np.abs(r["grad"]).max() > 0
        r["spans"], r["names"] = _spans(r["net"])
        for k in ("grad", "theta0", "theta"):
            r[k].setflags(write=False)
        del r["model"], r["net"]
        _BASE[key] = r
    return _BASE[key]


def _reference_step(o, theta0, slots0, g, it):
    from test_optimizer_semantics import keras_adam, keras_sgd
    if o.record.kind == "sgd":
        th, v = keras_sgd(theta0, slots0[0] if slots0 else None, g, it, o.lr, o.decay, o.momentum, o.nesterov)
        return th, ([v] if slots0 else [])
    th, m, v, _ = keras_adam(theta0, slots0[0], slots0[1], None, g, it, o.lr, o.decay, o.beta_1, o.beta_2, o.epsilon, False)
    return th, [m, v]


@pytest.mark.parametrize("regularized", [False, True], ids=["plain", "l2"])
@pytest.mark.parametrize("kind", list(KEYS))
@pytest.mark.parametrize("opt_name", ["adam", "momentum"])
def test_one_eager_step_is_the_definition_then_the_optimizer(opt_name, kind, regularized):
    base = _base(opt_name, regularized)
    g, spans = base["grad"], base["spans"]
    measured = _measure(kind, g, spans)
    assert np.isfinite(measured) and measured > 0
    # half of what was measured: the step clips
    c = float(F(0.5 * measured))
    r = _eager_step(opt_name, regularized, kind, c)
    net = r["net"]
    assert r["pending"] == (kind != "global_norm")            # the global norm needs every gradient: no early update
    assert np.array_equal(r["theta0"].view(np.uint32), base["theta0"].view(np.uint32))
    clipped = R.clip(kind, g, c, spans)
    assert not np.array_equal(clipped, g)
    th, ref_slots = _reference_step(r["o"], r["theta0"], r["slots0"], clipped, 4)
    got = net.params.theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    print(kind, "measured", measured, "c", c, "theta: max err", float(err.max()))
    assert err.max() <= 1e-6, float(err.max())
    assert not np.array_equal(r["theta"], base["theta"])
    for name, s_ref in zip(r["spec"].slots, ref_slots):
        s_got = net.slot(name).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())
    # net.grad holds the clipped gradient.  By value: the definition's bits.  By a norm: the scale may differ from the
    # definition's by 1 float32 ulp (1.2e-7) and the product's rounding by another; one denormal step where it is tiny
    if kind == "value":
        assert np.array_equal(r["grad"].view(np.uint32), clipped.view(np.uint32))
        with pytest.raises(RuntimeError):
            net.gradient_norms()
    else:
        np.testing.assert_allclose(r["grad"], clipped, rtol=3e-7, atol=2e-45)
        norms = net.gradient_norms()
        if kind == "norm":
            want = R.clip_by_norm(g, c, spans)[2]
            assert list(norms) == base["names"]
            np.testing.assert_allclose(np.array(list(norms.values())), want.astype(np.float64), rtol=1e-6, atol=0)
        else:
            assert list(norms) == ["global"]
            assert abs(norms["global"] - measured) <= 1e-6 * measured
    # twice what was measured: nothing is clipped, and the variables are the unclipped step's, bit for bit
    r = _eager_step(opt_name, regularized, kind, float(F(2.0 * measured)))
    assert np.array_equal(r["theta"], base["theta"])
    assert all(np.array_equal(a, b) for a, b in zip(r["slots"], base["slots"]))
    assert np.array_equal(r["grad"].view(np.uint32), g.view(np.uint32))


# ---- fit() ---------------------------------------------------------------------------------------------------------------------
def _adam(kind=None, wrap=None):
    from lisec_amd import model_training as mt
    O = mt.optimizers
    o = {None: lambda: O.Adam(learning_rate=1e-3, decay=1e-3), "adamw": lambda: O.AdamW(0.01, learning_rate=1e-3),
         "lamb": lambda: O.LAMB(learning_rate=1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=["bias", "gamma", "beta"]),
         "ema": lambda: O.MovingAverage(O.Adam(learning_rate=1e-3, decay=1e-3), average_decay=0.9)}[wrap]()
    return _clipped(o, kind, FIXED.get(kind))


def _variables(model):
    net = model.net
    return dict(theta=_bits(net.params.theta), state=_bits(net.params.state), iter_dev=np.array(net._iter_dev.cpu().tolist()),
                grad=_bits(net.grad), **{"slot_" + k: _bits(net.slot(k)) for k in model.optimizer.spec().slots})


def _same(a, b):
    assert set(a) == set(b) and "theta" in a and "slot_m" in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _global_norm(grad_bits):
    return float(np.sqrt(R.sum_squares(grad_bits.view(F))))


_RUNS = {}


def _run(kind, tuning, n=3):
    """n sweeps, one epoch, from the default initial weights with Adam and the kind's fixed threshold; run once."""
    key = (kind, tuning, n)
    if key in _RUNS:
        return _RUNS[key]
    from lisec_amd import model_training as mt
    with _tuning(tuning):
        eager = tuning == EAGER
        model = _model()
        model.compile(optimizer=_adam(kind), loss=['mse', 'mse'])
        x, y = _data(mt, not eager, n=n)
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False)
        assert (model._captured is None) == eager
        r = dict(variables=_variables(model))
        if kind in ("norm", "global_norm"):
            r["norms"] = model.net.gradient_norms()
        step = None if eager else model._captured[1]
        if step is not None:
            r["launches"], r["kind"] = step.launches, type(step).__name__
            step.close()
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("kind", list(KEYS))
def test_recorded_plans_leave_the_bits_of_the_python_schedule(kind):
    eager, recorded, pipelined = _run(kind, EAGER), _run(kind, RECORDED), _run(kind, PIPELINED)
    assert recorded["kind"] == "RecordedStep" and pipelined["kind"] == "PipelinedStep"
    assert eager["variables"]["iter_dev"].tolist() == [3, 0]
    _same(eager["variables"], recorded["variables"])
    _same(eager["variables"], pipelined["variables"])
    # the last update clipped, so the runs above compared clipped steps
    g = eager["variables"]["grad"].view(F)
    if kind == "value":
        assert np.abs(g).max() == F(FIXED[kind])
    else:
        assert eager["norms"] == recorded["norms"] == pipelined["norms"]
        print(kind, "largest norm", max(eager["norms"].values()))
        assert max(eager["norms"].values()) > FIXED[kind]
    if kind == "global_norm":
        assert abs(_global_norm(eager["variables"]["grad"]) - FIXED[kind]) <= 1e-6 * FIXED[kind]
    assert not np.array_equal(eager["variables"]["theta"], _run(None, EAGER)["variables"]["theta"])


def test_the_plan_sizes():
    """Adam without clipping records the plan it always did (PARENT_LAUNCHES, also after clipped models have run in the
    process); each kind adds what CLIP_LAUNCHES derives."""
    sizes = {kind: _run(kind, RECORDED)["launches"] for kind in list(KEYS) + [None]}
    print("plan sizes:", sizes, "parent", PARENT_LAUNCHES)
    assert sizes[None] == PARENT_LAUNCHES
    for kind, more in CLIP_LAUNCHES.items():
        assert sizes[kind] == PARENT_LAUNCHES + more, kind


def test_batch_of_three_clips_the_mean_gradient_once():
    """fit(batch_size=3) over three sweeps, eager: one update, on the clipped MEAN gradient -- the definition applied to
    the mean that the same batch leaves without clipping -- and the recorded plan gives the same bits."""
    import torch
    from lisec_amd import model_training as mt

    def fit(kind, tuning):
        with _tuning(tuning):
            model = _model()
            model.compile(optimizer=_adam(kind), loss=['mse', 'mse'])
            theta0 = model.net.params.theta.cpu().numpy().copy()
            x, y = _data(mt, tuning != EAGER, n=3)
            model.fit(x=x, y=y, batch_size=3, verbose=0, epochs=1, shuffle=False)
            torch.cuda.synchronize()
            assert model.net.iterations == 1
            out = _variables(model)
            if model._captured is not None:
                model._captured[1].close()
            return model, theta0, out

    _, _, plain = fit(None, EAGER)
    model, theta0, got = fit("global_norm", EAGER)
    mean = plain["grad"].view(F)
    spans, _ = _spans(model.net)
    c = FIXED["global_norm"]
    clipped, scale, norm = R.clip_by_global_norm(mean, c, spans)
    assert norm > c and abs(model.net.gradient_norms()["global"] - float(norm)) <= 1e-6 * float(norm)
    np.testing.assert_allclose(got["grad"].view(F), clipped, rtol=3e-7, atol=2e-45)
    z = np.zeros_like(theta0)
    th, _ = _reference_step(model.optimizer, theta0, [z, z], clipped, 0)
    err = np.abs(got["theta"].view(F).astype(np.float64) - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, float(err.max())
    _, _, planned = fit("global_norm", PIPELINED)
    _same(got, planned)


@pytest.mark.parametrize("wrap", ["adamw", "lamb", "ema"])
def test_the_other_optimizers_take_a_clipped_step(wrap):
    from lisec_amd import model_training as mt
    model = _model()
    model.compile(optimizer=_adam("global_norm", wrap), loss=['mse', 'mse'])
    theta0 = _bits(model.net.params.theta)
    x, y = _data(mt, True, n=1)
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False)
    c, net = FIXED["global_norm"], model.net
    assert model.optimizer.spec().clip.config == ("global_norm", c) and net.iterations == 1
    theta = _bits(net.params.theta)
    assert np.isfinite(theta.view(F)).all() and not np.array_equal(theta, theta0)
    assert net.gradient_norms()["global"] > c
    assert abs(_global_norm(_bits(net.grad)) - c) <= 1e-6 * c                       # what the update was made with
    if wrap == "lamb":
        assert len(net.trust_ratios()) == len(net.params.trainable_names())
    if wrap == "ema":
        assert not np.array_equal(_bits(net.average), theta)
    model._captured[1].close()


def test_save_load_resume(tmp_path):
    """One epoch of three updates -> save -> load_model -> one more epoch: theta, the slots and the count of the
    uninterrupted two epochs, bit for bit; the model comes back compiled with the clipping it was saved with."""
    from lisec_amd import model_training as mt
    x, y = _data(mt, True, n=3)
    path = str(tmp_path / "half.h5")

    def fresh():
        m = _model()
        m.compile(optimizer=_adam("global_norm"), loss=['mse', 'mse'])
        return m

    def fit(m, epochs):
        m.fit(x=x, y=y, batch_size=1, verbose=0, epochs=epochs, shuffle=False)

    whole = fresh()
    fit(whole, 2)
    want = _variables(whole)
    assert want["iter_dev"].tolist() == [6, 0]
    half = fresh()
    fit(half, 1)
    half.save(path)
    resumed = mt.load_model(path)
    assert type(resumed.optimizer) is mt.optimizers.Adam and resumed.net.iterations == 3
    assert resumed.optimizer.global_clipnorm == FIXED["global_norm"] and resumed.optimizer.clipnorm is None
    assert resumed.optimizer.get_config() == half.optimizer.get_config()
    assert resumed.optimizer.spec() == half.optimizer.spec() and resumed.optimizer.spec().clip is not None
    fit(resumed, 1)
    got = _variables(resumed)
    _same(got, want)
    assert resumed.net.gradient_norms() == whole.net.gradient_norms()
    for m in (whole, half, resumed):
        if m._captured is not None:
            m._captured[1].close()


def test_no_norms_before_a_clipped_update():
    model = _model()
    with pytest.raises(RuntimeError):
        model.net.gradient_norms()
