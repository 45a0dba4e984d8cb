"""Model.fit(batch_size=B) on the small grid of the optimizer tests (createModel(16, 32, 8, 35), 2 500-point sweeps): the
gradient of a batch is the fp32 mean of its sweeps' gradients in sweep order, bit for bit; one update follows and counts
as one iteration; BatchNormalization statistics stay per sweep; the recorded plans (RecordedStep, PipelinedStep) leave
the bits of the Python schedule; the logs are sums over sweeps; schedules count updates; a regulariser acts once per
update; a Sequence is consumed item by item; batch_size=1 records the plan it always did."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_optimizers import SMALL, _cloud, _data, _dump, _make_opt, _same, _targets  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# RecordedStep.launches of the batch-1 step on this grid (loss ['mse', 'mse'], SGD with momentum, no regularizers),
# measured on the commit before mini-batches existed: batch_size=1 must keep recording exactly this plan
PARENT_LAUNCHES = 198


class _tuning:
    """LISEC_TUNING for the calls inside (the host knobs are read when they are asked for)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("LISEC_TUNING")
        os.environ["LISEC_TUNING"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("LISEC_TUNING", None)
        else:
            os.environ["LISEC_TUNING"] = self.old


# ---- the mean gradient and the update ---------------------------------------------------------------------------------
_MEAN = {}


def _mean_step():
    """Run once, shared: per-sweep gradients of sweeps 0, 1, 2 at fixed variables on one model, then
    fit(batch_size=3, steps_per_epoch=1) of a second model from the same weights under the Python schedule."""
    if _MEAN:
        return _MEAN
    import torch
    from lisec_amd import model_training as mt
    with _tuning("step_plan=0"):
        x, y = _data(mt, False)                              # padded to 4096 points, as the recorded step pads them
        one = mt.createModel(16, 32, 8, 35)
        one.compile(optimizer=_make_opt("sgd"), loss=['mse', 'mse'])
        weights = one._snapshot_weights()
        dev, grads = one.net.device, []
        for i in range(3):
            yc, yr = (torch.from_numpy(a[i]).to(dev) for a in y)
            one.net.forward(x[i].sample, training=True)
            one.net.backward(yc, yr, loss=one.loss)
            torch.cuda.synchronize()
            grads.append(one.net.grad.cpu().numpy().copy())
        two = mt.createModel(16, 32, 8, 35)
        two._restore_weights(weights)
        o = _make_opt("sgd")                                 # SGD(lr=0.01, decay=1e-3), no momentum
        two.compile(optimizer=o, loss=['mse', 'mse'])
        hist = two.fit(x=x, y=y, batch_size=3, verbose=0, epochs=1, steps_per_epoch=1, shuffle=False)
        assert two._captured is None                         # the Python schedule
        torch.cuda.synchronize()
    _MEAN.update(grads=grads, theta0=weights[0].cpu().numpy().copy(), grad=two.net.grad.cpu().numpy().copy(),
                 theta=two.net.params.theta.cpu().numpy().copy(), iterations=two.net.iterations,
                 iter_dev=two.net._iter_dev.cpu().tolist(), state_one=one.net.params.state.cpu().numpy().copy(),
                 state_two=two.net.params.state.cpu().numpy().copy(), state0=weights[1].cpu().numpy().copy(),
                 lr=o.lr, decay=o.decay, loss=hist.history["loss"])
    return _MEAN


def test_batch_gradient_is_the_fp32_mean_in_sweep_order():
    """Fails before mini-batches existed: fit(batch_size=3) raised NotImplementedError."""
    r = _mean_step()
    g0, g1, g2 = r["grads"]
    assert all(g.dtype == np.float32 for g in r["grads"]) and np.abs(g0).max() > 0 and not np.array_equal(g0, g1)
    want = ((g0 + g1) + g2) * np.float32(1 / 3)
    assert want.dtype == np.float32
    assert np.array_equal(r["grad"].view(np.uint32), want.view(np.uint32))
    # a division instead of the multiply would show: the check is not vacuous
    assert not np.array_equal(want, ((g0 + g1) + g2) / np.float32(3))
    assert r["iterations"] == 1 and r["iter_dev"] == [1, 0]
    # the moving statistics are those after the three forwards in order, one momentum step per sweep
    assert np.array_equal(r["state_one"].view(np.uint32), r["state_two"].view(np.uint32))
    assert not np.array_equal(r["state_two"], r["state0"])


def test_batch_update_is_sgd_on_the_mean():
    """theta after the step against the fp64 SGD update by the mean gradient, to the bound of
    test_gpu_optimizers.test_one_step_matches_formula_on_its_own_gradient for one update: |err| / max(1, |theta|) <= 1e-6."""
    from test_optimizer_semantics import keras_sgd
    r = _mean_step()
    mean = r["grad"].astype(np.float64)
    th, _ = keras_sgd(r["theta0"], None, mean, 0, r["lr"], r["decay"], 0.0, False)
    got = r["theta"].astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    print(f"SGD on the batch mean: worst error {float(err.max()):.3e} (bound 1e-6)")
    assert err.max() <= 1e-6
    assert not np.array_equal(r["theta"], r["theta0"])
    # one update, not three: three updates by the sweep gradients end elsewhere by far more than the bound
    three = r["theta0"].astype(np.float64) - r["lr"] * sum(g.astype(np.float64) for g in r["grads"])
    assert (np.abs(got - three) / np.maximum(1.0, np.abs(three))).max() > 1e-4


def test_train_batch_is_the_same_step_eagerly():
    """LisecNet.train_batch on the three sweeps: the gradient, variables and moving statistics of fit(batch_size=3) under the
    Python schedule, bit for bit, and the batch's [total, class, regression] as the mean of the sweeps' losses."""
    import torch
    from lisec_amd import model_training as mt
    r = _mean_step()
    x, y = _data(mt, False)
    model = mt.createModel(16, 32, 8, 35)
    dev = model.net.device
    model._restore_weights((torch.from_numpy(r["theta0"]).to(dev), torch.from_numpy(r["state0"]).to(dev)))
    o = _make_opt("sgd")
    model.compile(optimizer=o, loss=['mse', 'mse'])
    yc, yr = (torch.from_numpy(a).to(dev) for a in y)
    out = model.net.train_batch([s.sample for s in x], yc, yr, loss=model.loss, opt=o.spec())
    torch.cuda.synchronize()
    net = model.net
    assert np.array_equal(net.grad.cpu().numpy().view(np.uint32), r["grad"].view(np.uint32))
    assert np.array_equal(net.params.theta.cpu().numpy().view(np.uint32), r["theta"].view(np.uint32))
    assert np.array_equal(net.params.state.cpu().numpy().view(np.uint32), r["state_two"].view(np.uint32))
    assert net.iterations == 1 and out.dtype == torch.float64
    assert abs(float(out[0]) - r["loss"][0]) <= 2 * U * abs(r["loss"][0])
    with pytest.raises(ValueError):
        net.train_micro_step(x[0].sample, yc[0], yr[0], "second")


# ---- recorded plans against the Python schedule (worker processes, as in test_gpu_optimizers) -------------------------------
def _worker(args):
    """n = 5 sweeps, two epochs; B = 2: batches (0, 1), (2, 3), (4) -- six updates on ten sweeps; B = 3: (0, 1, 2), (3, 4)."""
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.network import PipelinedStep, RecordedStep
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    model.compile(optimizer=_make_opt(args["opt"]), loss=['mse', 'mse'])
    x, y = _data(mt, "step_plan=0" not in args["tuning"], n=5)
    B = args.get("B", 2)
    hist = model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=2, shuffle=False)
    torch.cuda.synchronize()
    want = {"": PipelinedStep, "pipeline_voxels=0": RecordedStep, "step_plan=0": type(None)}[args["tuning"]]
    step = model._captured[1] if model._captured is not None else None
    assert type(step) is want, type(step)
    if step is not None:
        kinds = ("first", "middle", "last") if B > 2 else ("first", "last")
        assert sorted(step.micro) == sorted((p, j) for p in kinds for j in range(step.NBUF))
    _dump(model, args["out"])
    d = dict(np.load(args["out"]))
    for k, v in hist.history.items():
        d["hist_" + k] = np.array(v)
    d["acc"] = model.net._acc.cpu().numpy()
    np.savez(args["out"], **d)


_RUNS = {}


def _run(tmp_path, opt, tuning, B=2):
    if (opt, tuning, B) not in _RUNS:
        out = str(tmp_path / f"{opt}_{B}_{tuning.replace('=', '')}.npz")
        env = dict(os.environ, LISEC_TUNING=tuning)
        args = dict(opt=opt, tuning=tuning, out=out, B=B)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _RUNS[opt, tuning, B] = dict(np.load(out))
    return _RUNS[opt, tuning, B]


@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_batch_plans_are_bit_identical_to_python_schedule(tmp_path, opt):
    plan, eager = _run(tmp_path, opt, ""), _run(tmp_path, opt, "step_plan=0")
    assert int(plan["iterations"]) == 6 and plan["iter_dev"].tolist() == [6, 0]
    assert len(plan["hist_loss"]) == 2 and any(k.startswith("slot_") for k in plan)
    _same(plan, eager)                                       # theta, BN state, every slot, both counts, History, acc


def test_batch_plans_with_a_middle_sweep_are_bit_identical_to_python_schedule(tmp_path):
    """B = 3 on five sweeps: batches of 3 and 2, so the plan of a sweep in the middle of a batch (acc += grad) runs too."""
    plan, eager = _run(tmp_path, "momentum", "", B=3), _run(tmp_path, "momentum", "step_plan=0", B=3)
    assert int(plan["iterations"]) == 4 and plan["iter_dev"].tolist() == [4, 0]
    _same(plan, eager)


def test_pipelined_and_recorded_step_leave_the_same_bits(tmp_path):
    _same(_run(tmp_path, "momentum", ""), _run(tmp_path, "momentum", "pipeline_voxels=0"))


# ---- logs and schedules ---------------------------------------------------------------------------------------------------
def test_history_loss_is_the_sum_over_sweeps_divided_by_the_sweeps():
    """n = 5, B = 2, one epoch: History['loss'] against the fp64 sum of the five per-sweep fp32 losses / 5, within
    2 * 2^-24 * |loss| (one fp32 rounding per logged value, and the division)."""
    import torch
    from lisec_amd import model_training as mt
    with _tuning("step_plan=0"):
        model = mt.createModel(16, 32, 8, 35)
        model.compile(optimizer=_make_opt("momentum"), loss=['mse', 'mse'])
        x, y = _data(mt, False, n=5)
        net, seen = model.net, []
        inner = net.train_micro_step

        def spy(sample, yc, yr, position, **kw):
            out = inner(sample, yc, yr, position, **kw)
            seen.append((position, net.iterations, out.clone()))
            return out
        net.train_micro_step = spy
        hist = model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=1, shuffle=False).history
        torch.cuda.synchronize()
    assert [(p, it) for p, it, _ in seen] == [("first", 0), ("last", 1), ("first", 1), ("last", 2), ("single", 3)]
    per_sweep = np.stack([t.cpu().numpy().astype(np.float64) for _, _, t in seen])
    for col, key in enumerate(("loss", "ClassificationLayer_loss", "RegressionLayer_loss")):
        want = per_sweep[:, col].sum() / 5
        print(f"{key}: {hist[key][0]!r} against {want!r}")
        assert abs(hist[key][0] - want) <= 2 * U * abs(want)
    assert net.iterations == 3


def test_a_schedule_switches_after_updates_not_sweeps():
    """PiecewiseConstantDecay([2], [0.01, 0.001]) (Keras: values[0] while iterations <= 2), B = 2 on two sweeps: one update
    per epoch, four epochs from the recorded plans.  Updates 0, 1, 2 run at 0.01, update 3 at 0.001 -- counted in sweeps
    the rate would drop with the second update.  A callback logs the rate of the epoch's update from the schedule and
    model.net.iterations (History['lr']); the variables are checked against plain SGD by the mean gradient the update
    left in net.grad, to the one-update bound of test_gpu_optimizers (1e-6 relative to max(1, |theta|))."""
    import torch
    from lisec_amd import model_training as mt
    sched = mt.optimizers.schedules.PiecewiseConstantDecay([2], [0.01, 0.001])
    model = mt.createModel(16, 32, 8, 35)
    model.compile(optimizer=mt.optimizers.SGD(learning_rate=sched, momentum=0.0), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=2)
    net, trail = model.net, []

    class Trail(mt.callbacks.Callback):
        def on_epoch_begin(self, epoch, logs=None):
            torch.cuda.synchronize()
            self.before, self.it = net.params.theta.cpu().numpy().astype(np.float64), net.iterations

        def on_epoch_end(self, epoch, logs=None):
            torch.cuda.synchronize()
            logs["lr"] = float(sched(self.it))
            trail.append((self.before, net.grad.cpu().numpy().astype(np.float64),
                          net.params.theta.cpu().numpy().astype(np.float64), self.it, net.iterations))

    hist = model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=4, shuffle=False, callbacks=[Trail()]).history
    assert model._captured is not None
    assert hist["lr"] == [0.01, 0.01, 0.01, 0.001]
    assert [(a, b) for *_, a, b in trail] == [(0, 1), (1, 2), (2, 3), (3, 4)] and net._iter_dev.cpu().tolist() == [4, 0]
    for epoch, (before, g, after, _, _) in enumerate(trail):
        right, wrong = (0.01, 0.001) if epoch < 3 else (0.001, 0.01)
        err = np.abs(after - (before - right * g)) / np.maximum(1.0, np.abs(before))
        off = np.abs(after - (before - wrong * g)) / np.maximum(1.0, np.abs(before))
        print(f"update {epoch}: worst error at rate {right}: {float(err.max()):.3e}; at {wrong}: {float(off.max()):.3e}")
        assert err.max() <= 1e-6 and off.max() > 1e-4


# ---- regularizers ---------------------------------------------------------------------------------------------------------------
def test_a_regulariser_acts_once_per_update_and_the_loss_holds_the_penalty_once():
    """bias_regularizer=l1(1e-3), kernel_regularizer=l2(4e-3), B = 2, two consecutive batches from the recorded plans.  A
    conv bias in front of a training-mode BatchNormalization (unwritten_grads) has gradient 0 and no backward pass writes
    its slot: after the SECOND batch the slot holds l1*sign(b) of that update once -- not twice (accumulated over the
    sweeps) and not the sum of both updates -- within the bound of test_gpu_regularized_fit.test_step_arithmetic_sgd,
    4 * 2^-24 * (|g| + |2*l2*w| + |l1|) with g = 0 and l2 = 0 here.  loss - mean of the sweeps' (class + regression) = P of
    the weights before the update, within that file's bound (_check_identity)."""
    import torch
    from lisec_amd import model_training as mt
    from test_gpu_regularized_fit import _bias_slots, _check_identity, _penalty
    l1 = 1e-3
    model = mt.createModel(16, 32, 8, 35, bias_regularizer=mt.regularizers.l1(l1), kernel_regularizer=mt.regularizers.l2(4e-3))
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, momentum=0.0), loss=['mse', 'mse'])
    net = model.net
    gen = torch.Generator(device="cpu").manual_seed(3)
    for name, shape, kind in net.params.specs:
        if kind == "bias":
            net.params.view(name).copy_(torch.randn(shape, generator=gen) * 0.05)
    net.params.touch()
    slots = _bias_slots(net)
    x, y = _data(mt, True, n=2)
    P0 = _penalty(model)
    h = model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=1, shuffle=False).history
    assert model._captured is not None and net.iterations == 1
    _check_identity(h["loss"][0], h["ClassificationLayer_loss"][0], h["RegressionLayer_loss"][0], 1.0, 1.0, P0, "batch 1")
    torch.cuda.synchronize()
    b1 = net.params.theta.cpu().numpy()[slots].astype(np.float64)
    P1 = _penalty(model)
    h = model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=1, shuffle=False).history
    assert net.iterations == 2
    _check_identity(h["loss"][0], h["ClassificationLayer_loss"][0], h["RegressionLayer_loss"][0], 1.0, 1.0, P1, "batch 2")
    torch.cuda.synchronize()
    got = net.grad.cpu().numpy()[slots].astype(np.float64)
    term = l1 * np.sign(b1)
    err, bound = np.abs(got - term), 4 * U * l1
    print(f"unwritten biases after two batches: worst error / bound = {float(err.max() / bound):.3f}")
    assert np.abs(term).min() == l1 and np.all(err <= bound)
    # ... and they moved by lr * term per update (6 roundings of the product and one of b, as in that file)
    b2 = net.params.theta.cpu().numpy()[slots].astype(np.float64)
    assert np.all(np.abs(b2 - (b1 - 0.01 * term)) <= U * np.abs(b1) + 6 * U * 0.01 * l1)


# ---- a Sequence ---------------------------------------------------------------------------------------------------------------
_SEQ = r"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import augment_cases as C
from lisec_amd import Constants, augment
from lisec_amd import model_training as mt
Constants.nx, Constants.ny = 16, 32                 # the (16, 32, 8) grid of the augmentation tests
pts, bxs = C.fit_sweeps()


class Logged(augment.AugmentedSweeps):
    # what a recorded step stages, as the (seed, item, epoch) draw the item carries, with the updates made so far
    def staged(self, i):
        s = super().staged(i)
        self.log.append((s.draw, self.net.iterations))
        return s


for tuning in ("pipeline_voxels=0", ""):
    os.environ["LISEC_TUNING"] = tuning
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, momentum=0.9), loss=['mse', 'mse'])
    seq = Logged(pts, bxs, seed=11, subsample="random")
    seq.log, seq.net = [], m.net
    m.fit(x=seq, batch_size=2, verbose=0, epochs=2, shuffle=False)
    torch.cuda.synchronize()
    assert m._captured is not None and seq.epoch == 2 and m.net.iterations == 4, (seq.epoch, m.net.iterations)
    assert [d for d, _ in seq.log] == [(11, i, e) for e in range(2) for i in range(3)], seq.log
    if tuning:
        # RecordedStep stages a sweep directly in front of its replay: items 0 and 1 before the epoch's first update,
        # item 2 after it -- the batches are (0, 1) and (2)
        assert [it for _, it in seq.log] == [0, 0, 1, 2, 2, 3], seq.log
print("SEQ-OK")
"""


def test_a_sequence_is_consumed_item_by_item_in_batches(tmp_path):
    """AugmentedSweeps over 3 items, B = 2, two epochs: items (0, 1) and (2) of each epoch.  A child process: the label
    grid is a module constant."""
    script = tmp_path / "fit_sequence.py"
    script.write_text(_SEQ)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("LISEC_TUNING", None)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "SEQ-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- batch_size=1 is the step it always was ---------------------------------------------------------------------------------
def test_batch_size_one_records_the_plan_it_always_did():
    import torch
    from lisec_amd import _lib, model_training as mt
    from lisec_amd.network import RecordedStep
    with _tuning("pipeline_voxels=0"):
        model = mt.createModel(16, 32, 8, 35)
        model.compile(optimizer=_make_opt("momentum"), loss=['mse', 'mse'])
        x, y = _data(mt, True)
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=3, shuffle=False)
        one = model._captured[1]
        assert type(one) is RecordedStep and one.micro == {} and len(one.plans) == 1
        assert model.net._acc is None                        # nothing of a batch exists before a batch is asked for
        print("batch-1 plan:", one.launches, "operations")
        assert one.launches == PARENT_LAUNCHES
        # another batch size records its own plans; the batch-1 plan among them is the same one
        model.fit(x=x, y=y, batch_size=3, verbose=0, epochs=1, shuffle=False)
        two = model._captured[1]
        assert two is not one and two.launches == PARENT_LAUNCHES and len(two.plans) == 4
        size = {k: _lib.load().lisec_step_plan_size(p) for k, p in two.micro.items()}
        print("micro-step plans:", size)
        # ending a batch = the batch-1 step + one pass over the tail and one over the head of theta
        assert size["last", 0] == PARENT_LAUNCHES + 2
        assert size["first", 0] == size["middle", 0] < PARENT_LAUNCHES
        torch.cuda.synchronize()
        assert model.net.iterations == 3 + 1


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _worker(json.loads(sys.argv[2]))
