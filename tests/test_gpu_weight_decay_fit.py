"""optimizers.AdamW / SGDW in the training step on the small grid of the optimizer tests (createModel(16, 32, 8, 35)): the
step is the numpy decay (tests/weight_decay_ref.py) followed by the base optimizer's step, bit for bit; excluded
variables are left alone; mini-batches decay once per update; the recorded plans leave the bits of the Python schedule and
grow by exactly the decay launches; a coefficient changed by a callback reaches a replayed plan; the weight penalty is
taken before the decay; the averaging wrappers and the checkpoints carry on."""
import numpy as np
import pytest

import weight_average_ref as RA
import weight_decay_ref as R
from test_gpu_batch_fit import PARENT_LAUNCHES, _tuning
from test_gpu_optimizers import _data, _targets  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
DECAY_LAUNCHES = 2                         # what a decay adds to the plan of a step: one pass in front of each part of the update
EAGER, RECORDED, PIPELINED = "step_plan=0", "pipeline_voxels=0", ""


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _floats(b):
    return b.view(np.float32)


def _opt(name):
    from lisec_amd import model_training as mt
    O = mt.optimizers
    return {"adam": lambda: O.Adam(learning_rate=1e-3, decay=1e-3),
            "adamw": lambda: O.AdamW(0.05, learning_rate=1e-3, decay=1e-3),
            "adamw0": lambda: O.AdamW(0.0, learning_rate=1e-3, decay=1e-3),
            "adamw_cosine": lambda: O.AdamW(O.schedules.CosineDecay(0.1, 4, alpha=0.1), learning_rate=1e-3),
            "adamw_01": lambda: O.AdamW(0.1, learning_rate=1e-3),
            "sgd": lambda: O.SGD(lr=0.01, decay=1e-3, momentum=0.9),
            "sgdw": lambda: O.SGDW(0.03, learning_rate=0.01, decay=1e-3, momentum=0.9),
            "sgdw0": lambda: O.SGDW(0.0, learning_rate=0.01, decay=1e-3, momentum=0.9),
            "sgdw_kernels": lambda: O.SGDW(0.03, learning_rate=0.01, decay=1e-3, momentum=0.9, decay_var_list=["kernel"]),
            "ema_adamw": lambda: O.MovingAverage(O.AdamW(0.05, learning_rate=1e-3, decay=1e-3), average_decay=0.9,
                                                 dynamic_decay=True)}[name]()


def _model(regularized=False):
    from lisec_amd import model_training as mt
    kw = dict(kernel_regularizer=mt.regularizers.l2(1e-4)) if regularized else {}
    return mt.createModel(16, 32, 8, 35, **kw)


def _variables(model):
    net = model.net
    return dict(theta=_bits(net.params.theta), state=_bits(net.params.state), iter_dev=np.array(net._iter_dev.cpu().tolist()),
                **{"slot_" + k: _bits(net.slot(k)) for k in model.optimizer.spec().slots})


def _same(a, b):
    """The variables of two runs (_variables' keys), bit for bit."""
    a, b = ({k: v for k, v in r.items() if k in ("theta", "state", "iter_dev", "grad", "theta0") or k.startswith("slot_")}
            for r in (a, b))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


_RUNS = {}


def _run(name, tuning, B=1):
    """Five sweeps, one epoch (B = 2: batches of two, two and one sweep), from the default initial weights; run once and
    shared.  Under the Python schedule theta is read after every update."""
    key = (name, tuning, B)
    if key in _RUNS:
        return _RUNS[key]
    from lisec_amd import _lib
    from lisec_amd import model_training as mt
    with _tuning(tuning):
        eager = tuning == EAGER
        model = _model()
        model.compile(optimizer=_opt(name), loss=['mse', 'mse'])
        net = model.net
        thetas = [_bits(net.params.theta)]
        x, y = _data(mt, not eager, n=5)
        if eager:
            inner = net.train_micro_step

            def spy(sample, yc, yr, position, **kw):
                out = inner(sample, yc, yr, position, **kw)
                if position in ("single", "last"):
                    thetas.append(_bits(net.params.theta))
                return out
            net.train_micro_step = spy
        model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=1, shuffle=False)
        assert (model._captured is None) == eager
        r = dict(_variables(model), thetas=thetas)
        if name.startswith("ema"):
            r["average"] = _bits(net.average)
        step = None if eager else model._captured[1]
        if step is not None:
            r["launches"] = step.launches
            r["micro"] = {k: _lib.load().lisec_step_plan_size(p) for k, p in step.micro.items()}
            r["kind"] = type(step).__name__
            step.close()
    _RUNS[key] = r
    return r


# ---- composition: the step is the decay, then the base optimizer's step ------------------------------------------------------
@pytest.mark.parametrize("name,base,wd", [("adamw", "adam", 0.05), ("sgdw", "sgd", 0.03)])
def test_the_step_is_the_decay_then_the_base_step(name, base, wd):
    """Net A takes one AdamW (SGDW with momentum) step, split into the early update and the rest as fit() splits it.  Net B
    holds the same variables and the same gradient: theta is read back after the backward pass, decayed in numpy,
    written back, and the plain Adam (SGD) step follows in one piece.  Theta and the slots: the same bits."""
    import torch
    from lisec_amd import model_training as mt
    with _tuning(EAGER):
        x, y = _data(mt, False, n=1)
        got = {}
        for which in ("A", "B"):
            model = _model()
            opt = _opt(name if which == "A" else base)
            model.compile(optimizer=opt, loss=['mse', 'mse'])
            net, spec = model.net, opt.spec()
            yc, yr = (torch.from_numpy(a[0]).to(net.device) for a in y)
            theta0 = _bits(net.params.theta)
            net.forward(x[0].sample, training=True)
            if which == "A":
                net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
                assert net._early is not None                        # the update was split
            else:
                net.backward(yc, yr, loss="mse")
                assert np.array_equal(_bits(net.params.theta), theta0)
                decayed = R.step(_floats(theta0), R.coefficient(wd, 0))
                assert not np.array_equal(R.bits(decayed), theta0)
                net.params.theta.copy_(torch.from_numpy(decayed))
            grad = _bits(net.grad)
            net.apply_gradients(opt=spec)
            got[which] = dict(_variables(model), grad=grad, theta0=theta0)
        assert np.array_equal(got["A"]["theta0"], got["B"]["theta0"])
        assert got["A"]["iter_dev"].tolist() == [1, 0]
        assert not np.array_equal(got["A"]["theta"], got["A"]["theta0"])
        _same(got["A"], got["B"])


# ---- exclusions, and one decay per update --------------------------------------------------------------------------------------
def _by_kind(model, theta_bits):
    """{kind: [(name, float32 array)]} of the trainable variables in a copy of theta."""
    p, out = model.net.params, {}
    kinds = {n: k for n, _, k in p.specs}
    flat = _floats(theta_bits)
    for n in p.trainable_names():
        _, off, shape = p.offsets[n]
        out.setdefault(kinds[n], []).append((n, flat[off:off + int(np.prod(shape))]))
    return out


@pytest.mark.parametrize("B,sweeps,updates", [(1, 3, 3), (2, 4, 2)])
def test_excluded_variables_and_one_decay_per_update(B, sweeps, updates):
    """SGDW(learning_rate=0, weight_decay=0.01, decay_var_list=['kernel']): after `updates` updates the kernels are the
    reference iterated that often, and biases, gamma and beta have their values (==: an update with a rate of 0 may turn
    a -0 into +0).  batch_size=2 over four sweeps: exactly two decays, not four."""
    from lisec_amd import model_training as mt
    model = _model()
    model.compile(optimizer=mt.optimizers.SGDW(learning_rate=0.0, weight_decay=0.01, decay_var_list=['kernel']),
                  loss=['mse', 'mse'])
    x, y = _data(mt, True, n=sweeps)
    before = _by_kind(model, _bits(model.net.params.theta))
    model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=1, shuffle=False)
    assert model.net.iterations == updates and model._captured is not None
    after = _by_kind(model, _bits(model.net.params.theta))
    assert sorted(before) == ["beta", "bias", "gamma", "kernel"]
    for (n, w0), (_, w1) in zip(before["kernel"], after["kernel"]):
        want = R.steps(w0, 0.01, range(updates))
        assert (w1 == want).all(), n
        assert not (R.steps(w0, 0.01, range(updates + 1)) == want).all() and not (w0 == want).all(), n
    for kind in ("bias", "gamma", "beta"):
        for (n, w0), (_, w1) in zip(before[kind], after[kind]):
            assert (w1 == w0).all(), n
    assert any((w0 != 0).any() for _, w0 in before["gamma"])                # a decay of gamma = 1 would have shown
    model._captured[1].close()


def test_a_decay_var_list_the_network_cannot_serve_is_refused_at_compile():
    from lisec_amd import model_training as mt
    model = _model()
    with pytest.raises(KeyError):
        model.compile(optimizer=mt.optimizers.AdamW(1e-4, decay_var_list=["no.such.kernel"]), loss=['mse', 'mse'])
    with pytest.raises(ValueError):
        model.compile(optimizer=mt.optimizers.AdamW(1e-4, decay_var_list=["mid1.bn.moving_mean"]), loss=['mse', 'mse'])
    assert model.optimizer is None


# ---- plans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adamw", "sgdw_kernels", "adamw_cosine"])
def test_recorded_plans_leave_the_bits_of_the_python_schedule(name):
    eager, recorded, pipelined = _run(name, EAGER), _run(name, RECORDED), _run(name, PIPELINED)
    assert recorded["kind"] == "RecordedStep" and pipelined["kind"] == "PipelinedStep"
    assert eager["iter_dev"].tolist() == [5, 0] and len(eager["thetas"]) == 6
    for plan in (recorded, pipelined):
        _same({k: v for k, v in eager.items() if k != "thetas"},
              {k: v for k, v in plan.items() if k in eager and k != "thetas"})
    base = {"adamw": "adam", "sgdw_kernels": "sgd", "adamw_cosine": "adam"}[name]
    if name != "adamw_cosine":                               # (another rate and no legacy decay: no base run to differ from)
        assert not np.array_equal(eager["theta"], _run(base, EAGER)["theta"])


def test_the_schedule_is_read_at_the_count_of_the_step():
    """Eager, theta after each update: the first update of the cosine run decays with wd_0 = 0.1 -- the run with the
    constant 0.1 has that theta -- and the second one with another coefficient."""
    cosine, constant = _run("adamw_cosine", EAGER), _run("adamw_01", EAGER)
    assert R.coefficient(_opt("adamw_cosine").weight_decay, 0) == F(0.1) != R.coefficient(_opt("adamw_cosine").weight_decay, 1)
    assert np.array_equal(cosine["thetas"][1], constant["thetas"][1])
    assert not np.array_equal(cosine["thetas"][2], constant["thetas"][2])


def test_plan_sizes():
    """A spec without decay -- also the constant 0 -- records the plan test_gpu_batch_fit pins; one with decay exactly the
    decay launches more, and a sweep that only accumulates nothing more."""
    sizes = {name: _run(name, RECORDED)["launches"] for name in ("sgd", "sgdw0", "sgdw", "sgdw_kernels", "adam", "adamw0", "adamw")}
    print("plan sizes", sizes, "parent", PARENT_LAUNCHES)
    assert sizes["sgd"] == PARENT_LAUNCHES and sizes["sgdw0"] == PARENT_LAUNCHES
    assert sizes["adamw0"] == sizes["adam"]
    assert sizes["sgdw"] == PARENT_LAUNCHES + DECAY_LAUNCHES and sizes["sgdw_kernels"] == PARENT_LAUNCHES + DECAY_LAUNCHES
    assert sizes["adamw"] == sizes["adam"] + DECAY_LAUNCHES
    _same(_run("sgdw0", RECORDED), _run("sgd", RECORDED))
    plan, plain = _run("sgdw", RECORDED, B=2), _run("sgd", RECORDED, B=2)
    print("micro plans", plan["micro"], plain["micro"])
    assert plan["micro"]["last", 0] == plain["micro"]["last", 0] + DECAY_LAUNCHES
    for position in ("first", "middle"):
        if (position, 0) in plain["micro"]:
            assert plan["micro"][position, 0] == plain["micro"][position, 0]
    _same({k: v for k, v in _run("sgdw", EAGER, B=2).items() if k != "thetas"},
          {k: v for k, v in plan.items() if k in ("theta", "state", "iter_dev", "slot_velocity")})
    assert plan["iter_dev"].tolist() == [3, 0]


# ---- callbacks -----------------------------------------------------------------------------------------------------------------
def test_a_callback_changes_the_coefficient_of_a_replayed_plan():
    """A callback halves optimizer.weight_decay after the first epoch: the plan recorded in that epoch is replayed in the
    second and decays with the new coefficient -- the bits of an eager run that does the same, not those of a run that
    keeps the coefficient."""
    from lisec_amd import model_training as mt

    def run(tuning, halve):
        with _tuning(tuning):
            model = _model()
            model.compile(optimizer=_opt("adamw"), loss=['mse', 'mse'])
            x, y = _data(mt, tuning != EAGER, n=2)
            plans = []

            class Halve(mt.callbacks.Callback):
                def on_epoch_end(self, epoch, logs=None):
                    plans.append(None if model._captured is None else model._captured[1])
                    if epoch == 0 and halve:
                        model.optimizer.weight_decay = model.optimizer.weight_decay / 2

            model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, shuffle=False, callbacks=[Halve()])
            assert model.optimizer.weight_decay == (0.025 if halve else 0.05) and model.net.iterations == 4
            if tuning != EAGER:
                assert plans[0] is not None and plans[1] is plans[0]         # replayed, not recorded again
                plans[0].close()
            return _variables(model)

    eager, plan, kept = run(EAGER, True), run(PIPELINED, True), run(PIPELINED, False)
    _same(eager, plan)
    assert not np.array_equal(plan["theta"], kept["theta"])


# ---- with regularizers ---------------------------------------------------------------------------------------------------------
def test_the_penalty_is_taken_on_the_weights_before_the_decay():
    """kernel_regularizer=l2(1e-4) and AdamW(0.1): the logged `loss` of the first step is the data loss plus the penalty of
    the UNDECAYED weights (net.penalty() before the step), not of the decayed ones (0.81 of it)."""
    import torch
    from lisec_amd import model_training as mt
    model = _model(regularized=True)
    model.compile(optimizer=mt.optimizers.AdamW(0.1, learning_rate=1e-3), loss=['mse', 'mse'])
    p0 = float(model.net.penalty().item())
    x, y = _data(mt, True, n=1)
    h = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False).history
    torch.cuda.synchronize()
    in_step = float(model.net.reg_penalty.item())                           # what the step itself summed, in two parts
    loss, data = h["loss"][0], h["ClassificationLayer_loss"][0] + h["RegressionLayer_loss"][0]
    # float32: the two losses, their sum and the fold of the penalty into it, each half an ulp of a number <= loss
    bound = 2 * float(np.spacing(F(loss)))
    print("loss", loss, "data", data, "penalty before", p0, "in the step", in_step, "bound", bound)
    assert p0 > 0 and abs(0.19 * p0) > 100 * bound                          # the two penalties are told apart
    assert abs((loss - data) - p0) <= bound
    assert abs(in_step - p0) <= 1e-12 * p0                                  # fp64 sums of the same terms in another order
    p1 = float(model.net.penalty().item())                                  # of the decayed, updated weights: about 0.81 p0
    assert abs(p1 - 0.81 * p0) < 0.01 * p0
    model._captured[1].close()


# ---- averaging -----------------------------------------------------------------------------------------------------------------
def test_the_average_sees_the_decayed_updated_variables():
    w, plain = _run("ema_adamw", EAGER), _run("adamw", EAGER)
    assert len(w["thetas"]) == 6
    for s, (a, b) in enumerate(zip(w["thetas"], plain["thetas"])):          # the training is AdamW's
        assert np.array_equal(a, b), s
    a = _floats(w["thetas"][0]).copy()
    for s, th in enumerate(w["thetas"][1:]):
        a = RA.ema_step(a, _floats(th), s, 0.9, dynamic_decay=True)
    assert np.array_equal(w["average"], RA.bits(a))
    plan = _run("ema_adamw", PIPELINED)
    assert np.array_equal(plan["average"], w["average"]) and np.array_equal(plan["theta"], w["theta"])
    assert plan["launches"] == _run("adamw", PIPELINED)["launches"] + 1     # the averaging pass


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adamw_cosine", "sgdw_kernels"])
def test_save_load_resume(tmp_path, name):
    """One epoch of three updates -> save -> load_model -> one more epoch: theta, the slots and the count of the
    uninterrupted two epochs, bit for bit; the class, weight_decay and decay_var_list come back."""
    from lisec_amd import model_training as mt
    x, y = _data(mt, True, n=3)
    path = str(tmp_path / "half.h5")

    def fresh():
        m = _model()
        m.compile(optimizer=_opt(name), loss=['mse', 'mse'])
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
    assert type(resumed.optimizer) is type(half.optimizer) and type(resumed.optimizer).__name__ in ("AdamW", "SGDW")
    assert resumed.optimizer.get_config() == half.optimizer.get_config() and resumed.net.iterations == 3
    assert resumed.optimizer.spec() == half.optimizer.spec()
    _same(_variables(resumed), _variables(half))
    fit(resumed, 1)
    _same(_variables(resumed), want)
    for m in (whole, half, resumed):
        if m._captured is not None:
            m._captured[1].close()
