"""Weight regularizers through the training step, fit, evaluate, the recorded plan and save / load_model, on the small
grid of the optimizer tests (createModel(16, 32, 8, 35, ...)).

The oracle is numpy in fp64 on the host copy of the variables:  P = sum_v l1_v*sum|w| + l2_v*sum w^2,  gradient term
2*l2*w + l1*sign(w) with sign(0) = 0.

The loss identity  loss - (w_c*cls + w_r*reg) = P  is asserted within 2^-23*|loss|.  The three logged values are
float32: `loss` before the fold is the float32 of w_c*C + w_r*R, cls and reg the float32 of C and R, and the fold rounds
once more, so the identity can be off by 2^-24*(2*|L| + |loss|) with L = w_c*C + w_r*R.  That is within the bound
whenever P >= L, so the coefficients below are chosen to make the penalty the larger part of the loss (each test
asserts that it is): Glorot kernels of this network have sum w^2 of a few thousand, BatchNormalization gammas are 1."""
import math
import os

import numpy as np
import pytest

from test_gpu_optimizers import SMALL, _cloud, _data, _targets

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _regs():
    from lisec_amd import regularizers as R
    return dict(kernel_regularizer=R.l1_l2(l1=2e-5, l2=4e-3), bias_regularizer=R.l1(1e-3), gamma_regularizer=R.l2(1e-3),
                beta_regularizer="l1")


def _penalty(model):
    """P of the model's variables as they are now: fp64 sums per variable, fsum over the variables."""
    import torch
    torch.cuda.synchronize()
    p = model.net.params
    terms = []
    for name, (l1, l2) in model.regularizers.items():
        w = p.view(name).detach().cpu().numpy().astype(np.float64)
        terms += [l1 * np.abs(w).sum(), l2 * (w * w).sum()]
    return math.fsum(terms)


def _check_identity(loss, cls, reg, wc, wr, P, what):
    rest = wc * cls + wr * reg
    print(f"{what}: loss {loss!r} = {rest!r} + P {P!r}; off by {abs(loss - rest - P) / (U * 2 * abs(loss)):.3f} of the bound")
    assert P >= rest > 0, "the bound is derived for a penalty that is the larger part of the loss"
    assert abs(loss - rest - P) <= 2 * U * abs(loss)


def test_step_arithmetic_sgd():
    import torch
    from lisec_amd import model_training as mt, ops
    from lisec_amd.voxelizer import Voxelizer
    model = mt.createModel(16, 32, 8, 35, **_regs())
    o = mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.0)
    model.compile(optimizer=o, loss=['mse', 'mse'])
    net, spec, dev = model.net, o.spec(), model.net.device
    # non-zero biases and betas, so that every kind has a gradient term
    for name, _, kind in net.params.specs:
        if kind in ("bias", "beta"):
            net.params.view(name).copy_(torch.randn_like(net.params.view(name)) * 0.05)
    net.params.touch()
    net.iterations = 2
    sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(0)).to(dev))
    yc, yr = (torch.from_numpy(a).to(dev) for a in _targets(0))
    net.forward(sample, training=True)
    net.backward(yc, yr, loss="mse")
    torch.cuda.synchronize()
    g0, theta0 = net.grad.clone(), net.params.theta.clone()
    plain_loss = net.loss_out.cpu().numpy().copy()
    P = _penalty(model)
    net.apply_gradients(opt=spec)
    torch.cuda.synchronize()
    # the gradient term, variable by variable
    g0h, g1h, w0 = g0.cpu().numpy().astype(np.float64), net.grad.cpu().numpy().astype(np.float64), theta0.cpu().numpy()
    term, bound = np.zeros_like(g0h), np.zeros_like(g0h)
    for name, (l1, l2) in model.regularizers.items():
        _, off, shape = net.params.offsets[name]
        n = int(np.prod(shape))
        w = w0[off:off + n].astype(np.float64)
        term[off:off + n] = 2.0 * l2 * w + l1 * np.sign(w)
        bound[off:off + n] = 4 * U * (np.abs(g0h[off:off + n]) + np.abs(2.0 * l2 * w) + abs(l1))
    assert set(model.regularizers) == set(net.params.trainable_names())
    err = np.abs(g1h - g0h - term)
    print(f"gradient term: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    assert np.abs(term).max() > 0 and not np.array_equal(g1h, g0h)
    # padding floats of theta stay 0 and get no gradient
    pad = np.ones(net.params.n_theta, bool)
    for name in net.params.trainable_names():
        _, off, shape = net.params.offsets[name]
        pad[off:off + int(np.prod(shape))] = False
    assert pad.sum() > 0 and not net.params.theta.cpu().numpy()[pad].any() and np.array_equal(g1h[pad], g0h[pad])
    # the update is the plain SGD entry on the regularised gradient, bit for bit
    clone, state = theta0.clone(), torch.tensor([2, 0], dtype=torch.int64, device=dev)
    ops.sgd_step_dev(clone, net.grad, None, o.lr, o.decay, 0.0, False, state, advance=True)
    torch.cuda.synchronize()
    assert torch.equal(clone, net.params.theta) and not torch.equal(theta0, net.params.theta)
    assert net.iterations == 3 and net._iter_dev.cpu().tolist() == [3, 0]
    # loss_out: the penalty folded into the total alone; reg_penalty holds it
    lo = net.loss_out.cpu().numpy()
    assert lo[1] == plain_loss[1] and lo[2] == plain_loss[2]
    assert lo[0] == np.float32(np.float64(plain_loss[0]) + net.reg_penalty.item())
    assert abs(net.reg_penalty.item() - P) <= 1e-9 * P


def _biased_model(mt, opt):
    """A model with a strong bias regularizer and non-zero biases everywhere, as a loaded reference file has them."""
    import torch
    from lisec_amd import regularizers as R
    model = mt.createModel(16, 32, 8, 35, kernel_regularizer=R.l2(4e-3), bias_regularizer=R.l1_l2(l1=0.05, l2=0.5))
    model.compile(optimizer=opt, loss=['mse', 'mse'])
    gen = torch.Generator(device="cpu").manual_seed(3)
    for name, shape, kind in model.net.params.specs:
        if kind == "bias":
            model.net.params.view(name).copy_(torch.randn(shape, generator=gen) * 0.05)
    model.net.params.touch()
    return model


def _bias_slots(net):
    """Index arrays into theta: the conv biases in front of a training-mode BatchNormalization, whose gradient slot no
    backward pass writes, and the padding floats."""
    unwritten = [n for n, _, k in net.params.specs if k == "bias" and n.startswith(("mid", "rpn"))]
    assert sorted(unwritten) == sorted(net.unwritten_grads) and len(unwritten) == 3 + 4 + 6 + 6
    idx = np.concatenate([np.arange(net.params.offsets[n][1], net.params.offsets[n][1] + net.params.offsets[n][2][0])
                          for n in unwritten])
    return idx


def test_two_steps_with_biases_no_backward_writes():
    """The gradient slots of the conv biases that feed a training-mode BatchNormalization are never written by the backward
    pass (their gradient is identically 0): after the SECOND step they must hold that step's term, not the sum of both,
    and theta must be the plain SGD update by the regularised gradient, step by step."""
    import torch
    from lisec_amd import model_training as mt, ops
    from lisec_amd.voxelizer import Voxelizer
    o = mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.0)
    model = _biased_model(mt, o)
    net, spec, dev = model.net, o.spec(), model.net.device
    slots = _bias_slots(net)
    is_unwritten = np.zeros(net.params.n_theta, bool)
    is_unwritten[slots] = True
    for step in range(2):
        sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(step)).to(dev))
        yc, yr = (torch.from_numpy(a).to(dev) for a in _targets(step))
        net.forward(sample, training=True)
        net.backward(yc, yr, loss="mse")
        torch.cuda.synchronize()
        g0, theta0 = net.grad.clone(), net.params.theta.clone()
        net.apply_gradients(opt=spec)
        torch.cuda.synchronize()
        g0h, g1h, w0 = g0.cpu().numpy().astype(np.float64), net.grad.cpu().numpy().astype(np.float64), theta0.cpu().numpy()
        g0h[is_unwritten] = 0.0                                # the true gradient there, whatever the slot still held
        term, bound = np.zeros_like(g0h), np.zeros_like(g0h)
        for name, (l1, l2) in model.regularizers.items():
            _, off, shape = net.params.offsets[name]
            n = int(np.prod(shape))
            w = w0[off:off + n].astype(np.float64)
            term[off:off + n] = 2.0 * l2 * w + l1 * np.sign(w)
            bound[off:off + n] = 4 * U * (np.abs(g0h[off:off + n]) + np.abs(2.0 * l2 * w) + abs(l1))
        err = np.abs(g1h - g0h - term)
        print(f"step {step}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}; on the unwritten "
              f"biases {float((err[slots] / bound[slots]).max()):.3f}, |term| there up to {np.abs(term[slots]).max():.3f}")
        assert np.abs(term[slots]).min() > 0.04                # every such bias has a term far above the bound
        assert np.all(err <= bound)
        clone, state = theta0.clone(), torch.tensor([step, 0], dtype=torch.int64, device=dev)
        ops.sgd_step_dev(clone, net.grad, None, o.lr, o.decay, 0.0, False, state, advance=True)
        torch.cuda.synchronize()
        assert torch.equal(clone, net.params.theta)


def test_fit_decays_the_unwritten_biases_by_one_term_per_step():
    """Three fit steps from the recorded plan (the early update of the RPN tail included): a bias with an identically zero
    gradient follows  b <- b - lr*(2*l2*b + l1*sign(b))  whatever the data.  The fp64 recurrence is met within, per step,
    one rounding of b, and 6 roundings of the lr*term product (4 for the term as asserted above, 1 for the float32 lr_t, 1
    for the product)."""
    import torch
    from lisec_amd import model_training as mt
    lr, steps = 0.01, 3
    model = _biased_model(mt, mt.optimizers.SGD(lr=lr, momentum=0.0))
    net = model.net
    slots = _bias_slots(net)
    (l1, l2), = {model.regularizers[n] for n in net.unwritten_grads}
    b = net.params.theta.cpu().numpy()[slots].astype(np.float64)
    b0, bound = b.copy(), np.zeros_like(b)
    x, y = _data(mt, True)
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=steps, shuffle=False)
    assert model._captured is not None
    torch.cuda.synchronize()
    for _ in range(steps):
        bound += U * np.abs(b) + 6 * U * lr * (np.abs(2.0 * l2 * b) + l1)
        b = b - lr * (2.0 * l2 * b + l1 * np.sign(b))
    got = net.params.theta.cpu().numpy()[slots].astype(np.float64)
    err = np.abs(got - b)
    print(f"unwritten biases after {steps} steps: worst error / bound = {float((err / bound).max()):.3f}; "
          f"one term more would move them by {lr * (2.0 * l2 * np.abs(b0) + l1).min():.2e}, the bound is {bound.max():.2e}")
    assert np.all(err <= bound)
    assert np.all(got != b0)                                   # they did decay


def _fit_once(model, mt, **kw):
    x, y = _data(mt, True, n=1)
    return model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=1, shuffle=False, **kw), x, y


@pytest.mark.parametrize("loss,weights", [(['mse', 'mse'], None), ("voxelnet", [2.0, 0.5])])
def test_fit_evaluate_and_val_loss_include_the_penalty(loss, weights):
    from lisec_amd import model_training as mt
    model = mt.createModel(16, 32, 8, 35, **_regs())
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, momentum=0.9, nesterov=True), loss=loss, loss_weights=weights)
    wc, wr = weights or (1.0, 1.0)
    P0 = _penalty(model)
    x, y = _data(mt, True, n=2)
    hist = model.fit(x=x[:1], y=[a[:1] for a in y], batch_size=1, verbose=0, epochs=1, steps_per_epoch=1, shuffle=False,
                     validation_data=(x[1:], [a[1:] for a in y])).history
    _check_identity(hist["loss"][0], hist["ClassificationLayer_loss"][0], hist["RegressionLayer_loss"][0], wc, wr, P0,
                    "fit")                                                       # P of the weights before the update
    P1 = _penalty(model)
    assert P1 != P0
    _check_identity(hist["val_loss"][0], hist["val_ClassificationLayer_loss"][0], hist["val_RegressionLayer_loss"][0],
                    wc, wr, P1, "val_loss")
    ev = model.evaluate(x, y, verbose=0, return_dict=True)
    _check_identity(ev["loss"], ev["ClassificationLayer_loss"], ev["RegressionLayer_loss"], wc, wr, P1, "evaluate")
    assert _penalty(model) == P1                                                 # evaluate changes no variable


_OPTS = {"sgd": lambda mt: mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True),
         "adam": lambda mt: mt.optimizers.Adam(learning_rate=1e-3)}
_REG_SETS = {"regs": _regs, "bare": dict,
             "none": lambda: dict(kernel_regularizer=None, bias_regularizer=None, gamma_regularizer=None,
                                  beta_regularizer=None)}
_RUNS = {}


def _three_steps(opt, step_plan, regs):
    """Three fit steps of a fresh model, from the recorded plan or from the Python schedule (the step_plan knob); run
    once per (optimizer, schedule, regularizer set) and shared between the tests below."""
    key = (opt, step_plan, regs)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from lisec_amd import _lib, model_training as mt
    os.environ["LISEC_TUNING"] = "step_plan=%d" % step_plan
    try:
        model = mt.createModel(16, 32, 8, 35, **_REG_SETS[regs]())
        model.compile(optimizer=_OPTS[opt](mt), loss=['mse', 'mse'])
        x, y = _data(mt, bool(step_plan))
        hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=3, shuffle=False)
        assert (model._captured is not None) == bool(step_plan)
        torch.cuda.synchronize()
        _RUNS[key] = dict(theta=model.net.params.theta.cpu().numpy().copy(), loss=hist.history["loss"][0],
                          iterations=model.net.iterations, regularizers=dict(model.regularizers),
                          has_penalty=hasattr(model.net, "reg_penalty"),
                          size=_lib.load().lisec_step_plan_size(model._captured[1].plans[0]) if step_plan else None)
        return _RUNS[key]
    finally:
        os.environ.pop("LISEC_TUNING", None)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_recorded_plan_and_python_schedule_leave_identical_theta(opt):
    """The early update (and with it the tail's penalty pass) runs on the side stream: Adam as well as SGD."""
    plan, eager = _three_steps(opt, 1, "regs"), _three_steps(opt, 0, "regs")
    assert np.array_equal(plan["theta"].view(np.uint32), eager["theta"].view(np.uint32))
    assert plan["loss"] == eager["loss"] and plan["iterations"] == eager["iterations"] == 3


def test_a_model_without_regularizers_records_the_plan_it_always_did():
    bare, none, reg = (_three_steps("sgd", 1, k) for k in ("bare", "none", "regs"))
    assert bare["size"] == none["size"] > 0
    assert none["regularizers"] == {} and not none["has_penalty"] and reg["has_penalty"]
    assert np.array_equal(bare["theta"].view(np.uint32), none["theta"].view(np.uint32))
    # the tail on the side stream and the head on the main stream: two calls of two launches each
    assert reg["size"] == bare["size"] + 4
    assert not np.array_equal(reg["theta"], bare["theta"]) and reg["loss"] > bare["loss"]      # the penalty did something


def test_save_and_load_model_bring_the_regularizers_back(tmp_path):
    from lisec_amd import model_training as mt
    model = mt.createModel(16, 32, 8, 35, **_regs())
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    _fit_once(model, mt)
    path = str(tmp_path / "x.h5")
    model.save(path)
    back = mt.load_model(path)
    assert back.regularizers == model.regularizers and len(back.regularizers) == len(model.net.params.trainable_names())
    assert back.net.regularizers == model.net.regularizers
    P = _penalty(back)
    assert P == _penalty(model)
    hist = _fit_once(back, mt)[0].history
    _check_identity(hist["loss"][0], hist["ClassificationLayer_loss"][0], hist["RegressionLayer_loss"][0], 1.0, 1.0, P,
                    "fit after load_model")
    # an .npz carries the variables alone
    npz = str(tmp_path / "x.npz")
    model.save(npz)
    assert mt.load_model(npz).regularizers == {}
