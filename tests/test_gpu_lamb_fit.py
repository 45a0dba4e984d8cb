"""optimizers.LAMB in the training step on the small grid of the optimizer tests (createModel(16, 32, 8, 35)): one step
against the fp64 definition (tests/lamb_ref.py) on the step's own gradient, the recorded plans against the Python
schedule, a mini-batch, save / load_model in the middle of a run, the averaging wrappers, a rate assigned by a callback,
trust_ratios(), and the plan of a model compiled with Adam afterwards."""
import numpy as np
import pytest

import lamb_ref as R
from test_gpu_batch_fit import PARENT_LAUNCHES, _tuning
from test_gpu_optimizers import _data, _targets  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
EAGER, RECORDED, PIPELINED = "step_plan=0", "pipeline_voxels=0", ""
NO_DECAY = ["bias", "gamma", "beta"]
# What LAMB adds to the plan of a step over Adam's two update launches: three launches (moments, ratios, apply) in the
# place of each.
LAMB_LAUNCHES = 4


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _floats(b):
    return b.view(np.float32)


def _opt(name="lamb"):
    from lisec_amd import model_training as mt
    O = mt.optimizers
    return {"lamb": lambda: O.LAMB(learning_rate=1e-3, decay=1e-3, weight_decay_rate=0.01, exclude_from_weight_decay=NO_DECAY),
            "ema_lamb": lambda: O.MovingAverage(_opt("lamb"), average_decay=0.9),
            "swa_lamb": lambda: O.SWA(_opt("lamb"), start_averaging=1, average_period=2),
            "adam": lambda: O.Adam(learning_rate=1e-3, decay=1e-3)}[name]()


def _model(regularized=False):
    from lisec_amd import model_training as mt
    kw = dict(kernel_regularizer=mt.regularizers.l2(1e-4)) if regularized else {}
    return mt.createModel(16, 32, 8, 35, **kw)


def _variables(model):
    net = model.net
    out = dict(theta=_bits(net.params.theta), state=_bits(net.params.state), iter_dev=np.array(net._iter_dev.cpu().tolist()),
               **{"slot_" + k: _bits(net.slot(k)) for k in model.optimizer.spec().slots})
    if model.optimizer.record.layerwise:
        ratios = net.trust_ratios()
        out["ratios"] = np.array([ratios[n] for n in net.params.trainable_names()], F).view(np.uint32)
    return out


def _same(a, b):
    keys = [k for k in a if k in b and (k in ("theta", "state", "iter_dev", "ratios") or k.startswith("slot_"))]
    assert "theta" in keys and "slot_m" in keys
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def _rows(model, opt):
    """lamb_ref's [(offset, count, decayed, adapted)] of the network's trainable variables, from the optimizer's lists."""
    p = model.net.params
    kinds = {n: k for n, _, k in p.specs}
    no_decay = opt.exclude_from_weight_decay or []
    no_adapt = no_decay if opt.exclude_from_layer_adaptation is None else opt.exclude_from_layer_adaptation
    rows = []
    for n in p.trainable_names():
        _, off, shape = p.offsets[n]
        # over the padded length, as the chunk table has it: the padding floats of theta and grad are 0 and add nothing
        # to a norm, but the test that starts from random slots has random m and v there too
        rows.append((off, (int(np.prod(shape)) + 3) // 4 * 4, not (n in no_decay or kinds[n] in no_decay),
                     not (n in no_adapt or kinds[n] in no_adapt)))
    return rows


_RUNS = {}


def _run(name, tuning, B=1, epochs=1):
    """Five sweeps per epoch from the default initial weights; run once and shared."""
    key = (name, tuning, B, epochs)
    if key in _RUNS:
        return _RUNS[key]
    from lisec_amd import model_training as mt
    with _tuning(tuning):
        eager = tuning == EAGER
        model = _model()
        model.compile(optimizer=_opt(name), loss=['mse', 'mse'])
        x, y = _data(mt, not eager, n=5)
        model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=epochs, shuffle=False)
        assert (model._captured is None) == eager
        r = _variables(model)
        if "_" in name:
            r["average"] = _bits(model.net.average)
        step = None if eager else model._captured[1]
        if step is not None:
            r["launches"], r["kind"] = step.launches, type(step).__name__
            step.close()
    _RUNS[key] = r
    return r


def _check_step(theta0, m0, v0, grad, rows, it, opt, net):
    import torch
    f32 = lambda x: float(F(x))                                          # the entries take these as C floats
    th, mm, vv, r = R.step(theta0, m0, v0, grad, rows, it, opt.lr, opt.decay, f32(opt.beta_1), f32(opt.beta_2),
                           f32(opt.epsilon), f32(opt.weight_decay_rate))
    torch.cuda.synchronize()
    got = net.params.theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    ratios = net.trust_ratios()
    got_r = np.array([ratios[n] for n in net.params.trainable_names()], np.float64)
    print("theta: max err", float(err.max()), "ratios: max rel", float(np.max(np.abs(got_r - r) / r)),
          "range", float(got_r.min()), float(got_r.max()))
    assert err.max() <= 1e-6, float(err.max())
    for name, s_ref in (("m", mm), ("v", vv)):
        s_got = net.slot(name).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())
    np.testing.assert_allclose(got_r, r, rtol=1e-5, atol=0)
    return got_r


@pytest.mark.parametrize("regularized", [False, True], ids=["plain", "l2"])
def test_one_eager_step_matches_the_definition_on_its_own_gradient(regularized):
    """The step as fit() splits it (the early update of the RPN tail, then the rest) at iteration 4 from non-zero slots;
    net.grad after the step is the gradient the update used -- with a regularizer, the penalty term included."""
    import torch
    from lisec_amd import model_training as mt
    with _tuning(EAGER):
        model = _model(regularized)
        o = _opt()
        model.compile(optimizer=o, loss=['mse', 'mse'])
        net, spec = model.net, o.spec()
        net.iterations = 4
        for name in spec.slots:
            net.slot(name).copy_(torch.rand_like(net.params.theta) * 1e-3)
        theta0 = net.params.theta.cpu().numpy().copy()
        m0, v0 = (net.slot(name).cpu().numpy().copy() for name in ("m", "v"))
        x, y = _data(mt, False, n=1)
        yc, yr = (torch.from_numpy(a[0]).to(net.device) for a in y)
        net.forward(x[0].sample, training=True)
        net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
        assert net._early is not None                                    # the update was split
        net.apply_gradients(opt=spec)
        torch.cuda.synchronize()
        g = net.grad.cpu().numpy()
        assert np.abs(g).max() > 0 and net.iterations == 5 and net._iter_dev.cpu().tolist() == [5, 0]
        rows = _rows(model, o)
        ratios = _check_step(theta0, m0, v0, g, rows, 4, o, net)
        assert not np.array_equal(net.params.theta.cpu().numpy(), theta0)
        # one finite ratio per trainable variable, 1.0 for the excluded ones and not for (all of) the others
        assert len(net.trust_ratios()) == len(rows) == len(net.params.trainable_names())
        assert np.isfinite(ratios).all() and (ratios > 0).all()
        adapted = np.array([r[3] for r in rows])
        assert (ratios[~adapted] == 1.0).all() and (~adapted).any() and (ratios[adapted] != 1.0).any()


def test_recorded_plans_leave_the_bits_of_the_python_schedule():
    eager, recorded, pipelined = _run("lamb", EAGER, epochs=2), _run("lamb", RECORDED, epochs=2), _run("lamb", PIPELINED, epochs=2)
    assert recorded["kind"] == "RecordedStep" and pipelined["kind"] == "PipelinedStep"
    assert eager["iter_dev"].tolist() == [10, 0]
    _same(eager, recorded)
    _same(eager, pipelined)
    assert not np.array_equal(eager["theta"], _run("adam", EAGER, epochs=2)["theta"])


def test_batch_of_three_is_three_micro_steps_and_one_update():
    """fit(batch_size=3) over three sweeps: positions first, middle, last, one update -- the definition applied to the
    accumulated mean, which net.grad holds after the step; and the recorded plans give the bits of the Python schedule."""
    import torch
    from lisec_amd import model_training as mt
    with _tuning(EAGER):
        model = _model()
        o = _opt()
        model.compile(optimizer=o, loss=['mse', 'mse'])
        net, seen = model.net, []
        theta0 = net.params.theta.cpu().numpy().copy()
        inner = net.train_micro_step

        def spy(sample, yc, yr, position, **kw):
            out = inner(sample, yc, yr, position, **kw)
            seen.append((position, net.iterations))
            return out
        net.train_micro_step = spy
        x, y = _data(mt, False, n=3)
        model.fit(x=x, y=y, batch_size=3, verbose=0, epochs=1, shuffle=False)
        torch.cuda.synchronize()
        assert seen == [("first", 0), ("middle", 0), ("last", 1)]
        z = np.zeros_like(theta0)
        _check_step(theta0, z, z, net.grad.cpu().numpy(), _rows(model, o), 0, o, net)
        eager = _variables(model)
    with _tuning(PIPELINED):
        model = _model()
        model.compile(optimizer=_opt(), loss=['mse', 'mse'])
        x, y = _data(mt, True, n=3)
        model.fit(x=x, y=y, batch_size=3, verbose=0, epochs=1, shuffle=False)
        assert model._captured is not None
        _same(eager, _variables(model))
        model._captured[1].close()


def test_save_load_resume(tmp_path):
    """One epoch of three updates -> save -> load_model -> one more epoch: theta, the slots and the count of the
    uninterrupted two epochs, bit for bit; the class and the exclusion lists come back."""
    from lisec_amd import model_training as mt
    x, y = _data(mt, True, n=3)
    path = str(tmp_path / "half.h5")

    def fresh():
        m = _model()
        m.compile(optimizer=_opt(), loss=['mse', 'mse'])
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
    assert type(resumed.optimizer) is mt.optimizers.LAMB and resumed.net.iterations == 3
    assert resumed.optimizer.get_config() == half.optimizer.get_config()
    assert resumed.optimizer.exclude_from_weight_decay == NO_DECAY and resumed.optimizer.spec() == half.optimizer.spec()
    a, b = _variables(resumed), _variables(half)
    _same({k: v for k, v in a.items() if k != "ratios"}, b)             # (the ratios are not state: none before an update)
    fit(resumed, 1)
    _same(_variables(resumed), want)
    for m in (whole, half, resumed):
        if m._captured is not None:
            m._captured[1].close()


@pytest.mark.parametrize("name", ["ema_lamb", "swa_lamb"])
def test_an_averaging_wrapper_trains_the_same_bits_and_swaps(name):
    from lisec_amd import model_training as mt
    plain = _run("lamb", PIPELINED)
    wrapped = _run(name, PIPELINED)
    _same(plain, wrapped)
    assert wrapped["launches"] == plain["launches"] + 1                  # the averaging pass
    assert not np.array_equal(wrapped["average"], wrapped["theta"])
    model = _model()
    model.compile(optimizer=_opt(name), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=3)              # (three updates: SWA's last snapshot is taken after the second)
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False)
    theta, average = _bits(model.net.params.theta), _bits(model.net.average)
    assert not np.array_equal(theta, average)
    with model.average_weights():
        assert np.array_equal(_bits(model.net.params.theta), average)
    assert np.array_equal(_bits(model.net.params.theta), theta)
    model._captured[1].close()


def test_reduce_lr_on_plateau_reaches_the_kernel_without_recording_again():
    from lisec_amd import callbacks
    from lisec_amd import model_training as mt
    x, y = _data(mt, True, n=2)

    class Flat(callbacks.Callback):
        def on_epoch_begin(self, epoch, logs=None):
            self.step = (self.model._captured or (None, None))[1]

        def on_epoch_end(self, epoch, logs=None):
            logs["val_loss"] = 1.0                  # a plateau from the second epoch on
            if epoch:
                assert self.model._captured[1] is self.step

    def fit(cbs):
        m = _model()
        m.compile(optimizer=_opt(), loss=['mse', 'mse'])
        h = m.fit(x=x, y=y, batch_size=1, verbose=0, epochs=4, shuffle=False, callbacks=cbs).history
        out = _variables(m)
        m._captured[1].close()
        return h, out

    ha, a = fit([Flat(), callbacks.ReduceLROnPlateau(factor=0.5, patience=1)])
    assert ha["lr"] == [0.001, 0.001, 0.0005, 0.00025]
    rates = ha["lr"]
    _, b = fit([callbacks.LearningRateScheduler(lambda epoch, lr: rates[epoch])])
    _same(a, b)
    _, kept = fit([callbacks.LearningRateScheduler(lambda epoch, lr: 0.001)])
    assert not np.array_equal(a["theta"], kept["theta"])


def test_lists_the_network_cannot_serve_are_refused_at_compile_and_no_ratios_before_an_update():
    from lisec_amd import model_training as mt
    model = _model()
    with pytest.raises(KeyError):
        model.compile(optimizer=mt.optimizers.LAMB(exclude_from_weight_decay=["no.such.kernel"]), loss=['mse', 'mse'])
    with pytest.raises(ValueError):
        model.compile(optimizer=mt.optimizers.LAMB(exclude_from_layer_adaptation=["mid1.bn.moving_mean"]), loss=['mse', 'mse'])
    assert model.optimizer is None
    with pytest.raises(RuntimeError):
        model.net.trust_ratios()


def test_the_plan_of_adam_is_the_size_it_was():
    """A model compiled with Adam AFTER LAMB has run in the process records the plan it always did: 198 operations, the
    size of Adam's recorded step on the commit before LAMB (measured there with tests/test_gpu_weight_decay_fit.py::
    test_plan_sizes, which prints it: 'adam': 198) -- Adam's update is two launches, the early update and the rest, like
    the SGD update whose plan test_gpu_batch_fit pins at PARENT_LAUNCHES = 198.  LAMB's own plan has three launches in the
    place of each of the two."""
    _run("lamb", RECORDED)
    adam = _run("adam", RECORDED)
    lamb = _run("lamb", RECORDED)
    print("plan sizes: adam", adam["launches"], "lamb", lamb["launches"], "parent", PARENT_LAUNCHES)
    assert adam["launches"] == PARENT_LAUNCHES
    assert lamb["launches"] == PARENT_LAUNCHES + LAMB_LAUNCHES
