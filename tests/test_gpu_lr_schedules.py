"""Learning-rate schedules and LearningRateScheduler on the GPU: the device evaluation of the schedule descriptor
(lisec_lr_schedule_eval) against the fp64 formulas of tests/test_lr_schedules.py, the *_sched update kernels against
the optimizer formulas and against the by-value entries, then Model.fit on the small grid -- step plan against the
Python schedule, one step against the formula, save / load_model / resume, LearningRateScheduler across epochs without
recording the step again, and two data-parallel ranks."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
SMALL = dict(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)
N_MODEL = 6_491_024                       # trainable variables of the Lisec network (params.py)

KERNEL_CONFIGS = {
    "sgd": dict(kind="sgd", momentum=0.0, nesterov=False),
    "momentum": dict(kind="sgd", momentum=0.9, nesterov=False),
    "nesterov": dict(kind="sgd", momentum=0.9, nesterov=True),
    "adam": dict(kind="adam", amsgrad=False),
    "amsgrad": dict(kind="adam", amsgrad=True),
}


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _desc_buffer(lr, decay=0.0):
    """A device descriptor holding lr (a number or a schedule) and the legacy decay."""
    import torch
    from lisec_amd import _lib, lr_schedules, ops
    buf = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device=_dev())
    ops.lr_schedule_set(buf, lr_schedules.descriptor(lr, decay))
    return buf


# ---- the device function ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.0, 1e-3])
def test_schedule_eval_matches_formula(decay):
    """lr_t for it = 0 .. 20 000 and around 2**24, every kind: within 1 fp32 ulp of the fp64 formula rounded once."""
    import torch
    from lisec_amd import ops
    from test_lr_schedules import CASES, make, near_restart, ref_lr
    for which, (name, c) in CASES.items():
        buf = _desc_buffer(make(which), decay)
        for start, n in ((0, 20_001), ((1 << 24) - 1000, 2000)):
            state = torch.tensor([start, 0], dtype=torch.int64, device=_dev())
            out = torch.full((n,), -1.0, dtype=torch.float32, device=_dev())
            ops.lr_schedule_eval(buf, state, n, out)
            got = out.cpu().numpy()
            assert state.cpu().tolist() == [start, 0]                   # read, never advanced
            steps = np.arange(start, start + n)
            keep = np.array([not (name == "CosineDecayRestarts" and near_restart(c, s)) for s in steps])
            ref = np.array([ref_lr(name, c, s) / (1.0 + decay * s) for s in steps[keep]])
            ref32 = ref.astype(np.float32)
            err = np.abs(got[keep].astype(np.float64) - ref32.astype(np.float64))
            ulp = np.spacing(np.abs(ref32)).astype(np.float64)
            assert (err <= ulp).all(), (which, start, int(steps[keep][np.argmax(err / ulp)]), float((err / ulp).max()))


# ---- update kernels through the C ABI ---------------------------------------------------------------------------------
def _launch(cfg, theta, grad, slots, state, advance, desc=None, lo=0, hi=None, lr=0.01, decay=1e-3):
    """desc: the *_sched entry on that descriptor; None: the by-value entry with (lr, decay)."""
    from lisec_amd import ops
    hi = theta.numel() if hi is None else hi
    s = [t[lo:hi] for t in slots]
    v = s[0] if s else None
    if cfg["kind"] == "sgd" and desc is not None:
        ops.sgd_step_sched(theta[lo:hi], grad[lo:hi], v, desc, cfg["momentum"], cfg["nesterov"], state, advance=advance)
    elif cfg["kind"] == "sgd":
        ops.sgd_step_dev(theta[lo:hi], grad[lo:hi], v, lr, decay, cfg["momentum"], cfg["nesterov"], state, advance=advance)
    elif desc is not None:
        ops.adam_step_sched(theta[lo:hi], grad[lo:hi], s[0], s[1], s[2] if cfg["amsgrad"] else None, desc, 0.9, 0.999,
                            1e-7, state, advance=advance)
    else:
        ops.adam_step_dev(theta[lo:hi], grad[lo:hi], s[0], s[1], s[2] if cfg["amsgrad"] else None, lr, decay, 0.9, 0.999,
                          1e-7, state, advance=advance)


def _n_slots(cfg):
    if cfg["kind"] == "sgd":
        return 1 if cfg["momentum"] > 0 else 0
    return 3 if cfg["amsgrad"] else 2


@pytest.mark.parametrize("n", [N_MODEL, 1028])
@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_sched_kernels_match_formula(which, n):
    """5 steps from it = 1 under ExponentialDecay(staircase, decay_steps=3): the rate halves between it = 2 and 3."""
    import torch
    from lisec_amd import model_training as mt
    from test_optimizer_semantics import keras_adam, keras_sgd
    cfg = KERNEL_CONFIGS[which]
    sched = mt.optimizers.schedules.ExponentialDecay(0.01, 3, 0.5, staircase=True)
    decay = 1e-3
    desc = _desc_buffer(sched, decay)
    rng = np.random.default_rng(21)
    theta0 = rng.standard_normal(n).astype(np.float32)
    k = _n_slots(cfg)
    theta = torch.from_numpy(theta0).to(_dev())
    slots = [torch.zeros(n, dtype=torch.float32, device=_dev()) for _ in range(k)]
    start = 1
    state = torch.tensor([start, 0], dtype=torch.int64, device=_dev())
    th = theta0.astype(np.float64)
    ref_slots = [np.zeros(n) for _ in range(k)]
    for step in range(5):
        g = (rng.standard_normal(n) * (1 + step)).astype(np.float32)
        _launch(cfg, theta, torch.from_numpy(g).to(_dev()), slots, state, True, desc=desc)
        it = start + step
        if cfg["kind"] == "sgd":
            th, v = keras_sgd(th, ref_slots[0] if k else None, g, it, sched(it), decay, cfg["momentum"], cfg["nesterov"])
            ref_slots = [v] if k else []
        else:
            th, m, v, vh = keras_adam(th, ref_slots[0], ref_slots[1], ref_slots[2] if cfg["amsgrad"] else None, g, it,
                                      sched(it), decay, 0.9, 0.999, 1e-7, cfg["amsgrad"])
            ref_slots = [m, v] + ([vh] if cfg["amsgrad"] else [])
        assert state.cpu().tolist() == [it + 1, 0]
    got = theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, (which, float(err.max()))
    for s_got, s_ref in zip(slots, ref_slots):
        np.testing.assert_allclose(s_got.cpu().numpy().astype(np.float64), s_ref, rtol=1e-5,
                                   atol=1e-7 * np.abs(s_ref).max())


@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_constant_descriptor_is_bit_identical_to_by_value_entry(which):
    """The CONSTANT kind gives the bits of the by-value entry, legacy decay included; Nesterov also those of
    lisec_sgd_nesterov_step_dev, the kernel the reference's configuration calls."""
    import torch
    from lisec_amd import ops
    cfg = KERNEL_CONFIGS[which]
    rng = np.random.default_rng(22)
    n, k = 400_004, _n_slots(cfg)
    theta0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(_dev())
    slots0 = [torch.from_numpy(np.abs(rng.standard_normal(n)).astype(np.float32) * 0.01).to(_dev()) for _ in range(k)]
    grads = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(_dev()) for _ in range(3)]
    lr, decay = 0.0137, 1e-3
    desc = _desc_buffer(lr, decay)
    runs = []
    for mode in ("value", "sched", "nesterov_ref"):
        if mode == "nesterov_ref" and which != "nesterov":
            continue
        theta, slots = theta0.clone(), [s.clone() for s in slots0]
        state = torch.tensor([97, 0], dtype=torch.int64, device=_dev())
        for g in grads:
            if mode == "nesterov_ref":
                ops.sgd_nesterov_step_dev(theta, g, slots[0], lr, decay, 0.9, state)
            else:
                _launch(cfg, theta, g, slots, state, True, desc=desc if mode == "sched" else None, lr=lr, decay=decay)
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [100, 0]
        runs.append([theta.cpu().numpy()] + [s.cpu().numpy() for s in slots])
    assert not np.array_equal(runs[0][0], theta0.cpu().numpy())
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), which


@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_sched_part_then_rest_is_bit_identical_to_one_launch(which):
    import torch
    from lisec_amd import model_training as mt
    cfg = KERNEL_CONFIGS[which]
    desc = _desc_buffer(mt.optimizers.schedules.CosineDecayRestarts(0.01, 2, t_mul=2.0, m_mul=0.7, alpha=0.1), 1e-4)
    rng = np.random.default_rng(23)
    n, lo = N_MODEL, 388_168
    k = _n_slots(cfg)
    theta0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(_dev())
    slots0 = [torch.from_numpy(np.abs(rng.standard_normal(n)).astype(np.float32) * 0.01).to(_dev()) for _ in range(k)]
    runs = []
    for split in (False, True):
        theta, slots = theta0.clone(), [s.clone() for s in slots0]
        state = torch.tensor([5, 0], dtype=torch.int64, device=_dev())
        for step in range(3):
            g = torch.from_numpy(np.random.default_rng(200 + step).standard_normal(n).astype(np.float32)).to(_dev())
            if split:
                _launch(cfg, theta, g, slots, state, False, desc=desc, lo=lo)
                _launch(cfg, theta, g, slots, state, True, desc=desc, hi=lo)
            else:
                _launch(cfg, theta, g, slots, state, True, desc=desc)
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [8, 0]
        runs.append([theta.cpu().numpy()] + [s.cpu().numpy() for s in slots])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), which


def test_bad_arguments_are_refused_and_enqueue_nothing():
    import torch
    from lisec_amd import _lib, lr_schedules
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    dev = _dev()
    n = 40_004
    rng = np.random.default_rng(24)
    th = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    v, m, vv = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
    state = torch.tensor([3, 0], dtype=torch.int64, device=dev)
    good = lr_schedules.descriptor(0.01, 0.0)
    desc = _desc_buffer(0.01)
    torch.cuda.synchronize()
    before = (th.clone(), desc.clone())

    def bad(**fields):
        d = lr_schedules.descriptor(0.01, 0.0)
        for key, val in fields.items():
            setattr(d, key, val)
        return d
    for d in (bad(kind=7), bad(kind=-1), bad(kind=1, decay_steps=0.0), bad(kind=5, decay_steps=-3.0),
              bad(kind=6, decay_steps=float("nan")), bad(kind=2, n_boundaries=65), bad(kind=2, n_boundaries=0)):
        assert lib.lisec_lr_schedule_set(P(desc), ctypes.byref(d), st) != 0
        assert lib.lisec_last_error()
    assert lib.lisec_lr_schedule_set(None, ctypes.byref(good), st) != 0
    assert lib.lisec_lr_schedule_set(P(desc), None, st) != 0
    assert lib.lisec_sgd_step_sched(P(th), P(g), P(v), n, None, 0.9, 1, P(state), 1, st) != 0       # NULL descriptor
    assert lib.lisec_sgd_step_sched(P(th), P(g), P(v), 6, P(desc), 0.9, 1, P(state), 1, st) != 0    # n % 4
    assert lib.lisec_sgd_step_sched(P(th), P(g), None, n, P(desc), 0.9, 0, P(state), 1, st) != 0    # no slot
    assert lib.lisec_sgd_step_sched(P(th), P(g), P(v), n, P(desc), 0.9, 0, P(state), 2, st) != 0    # advance
    assert lib.lisec_adam_step_sched(P(th), P(g), P(m), P(vv), None, n, None, 0.9, 0.999, 1e-7, P(state), 1, st) != 0
    assert lib.lisec_adam_step_sched(P(th), P(g), P(m), P(vv), None, 10, P(desc), 0.9, 0.999, 1e-7, P(state), 1, st) != 0
    assert lib.lisec_adam_step_sched(P(th), P(g), P(m), P(vv), None, n, P(desc), 1.0, 0.999, 1e-7, P(state), 1, st) != 0
    assert lib.lisec_lr_schedule_eval(None, P(state), 4, P(v), st) != 0
    assert lib.lisec_lr_schedule_eval(P(desc), P(state), -1, P(v), st) != 0
    torch.cuda.synchronize()
    assert torch.equal(th, before[0]) and torch.equal(desc, before[1]) and state.cpu().tolist() == [3, 0]
    assert not v.any() and not m.any() and not vv.any()


# ---- Model.fit on the small grid (worker processes: the step-plan knob is read once per process) -----------------------
def _make_opt(name):
    from lisec_amd import model_training as mt
    S = mt.optimizers.schedules
    return {"exp_nesterov": lambda: mt.optimizers.SGD(lr=S.ExponentialDecay(0.01, 2, 0.5, staircase=True), decay=1e-3,
                                                      momentum=0.9, nesterov=True),
            "restarts_adam": lambda: mt.optimizers.Adam(learning_rate=S.CosineDecayRestarts(1e-3, 2, t_mul=2.0, m_mul=0.8,
                                                                                            alpha=0.1), decay=1e-3),
            "exp_momentum": lambda: mt.optimizers.SGD(learning_rate=S.ExponentialDecay(0.02, 2, 0.5, staircase=True),
                                                      momentum=0.9),
            "nesterov": lambda: mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True),
            "adam": lambda: mt.optimizers.Adam(learning_rate=1e-3)}[name]()


def _dump(model, path, **extra):
    import torch
    torch.cuda.synchronize()
    net = model.net
    d = dict(theta=net.params.theta.cpu().numpy(), state=net.params.state.cpu().numpy(),
             iterations=np.array(net.iterations), iter_dev=net._iter_dev.cpu().numpy())
    for name in model.optimizer.spec().slots:
        d["slot_" + name] = net.slot(name).cpu().numpy()
    d.update({k: np.asarray(v) for k, v in extra.items()})
    np.savez(path, **d)


def _worker(args):
    """One fit scenario in a fresh process; writes variables, BN state, slots, iteration count (and what the mode
    observes) to args['out']."""
    from lisec_amd import _lib
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    mode, step_plan = args["mode"], bool(args["step_plan"])
    np.random.seed(0)
    if mode == "resume":
        model = mt.load_model(args["ckpt"])
        assert model.optimizer is not None and model.optimizer.spec() == _make_opt(args["opt"]).spec()
    else:
        model = mt.createModel(16, 32, 8, 35)
        model.compile(optimizer=_make_opt(args["opt"]), loss=['mse', 'mse'])
    x, y = _data(mt, step_plan)
    fit = dict(x=x, y=y, batch_size=1, verbose=0, steps_per_epoch=3, shuffle=False)
    extra = {}
    if mode in ("fit6", "save", "resume"):
        model.fit(epochs=2 if mode == "fit6" else 1, **fit)
        assert (getattr(model, "_captured", None) is not None) == step_plan
        if mode == "save":
            model.save(args["ckpt"])
    elif mode in ("lrs", "lrs_same"):
        class Watch(mt.callbacks.Callback):
            """The recorded plan and its size at the end of every epoch."""
            seen = []

            def on_epoch_end(self, epoch, logs=None):
                cap = getattr(self.model, "_captured", None)
                if cap is not None:
                    lib = _lib.load()
                    self.seen.append((id(cap[1]), lib.lisec_step_plan_size(cap[1].plans[0])))

        rates = args.get("rates")
        sched = (lambda epoch, lr: lr) if mode == "lrs_same" else (lambda epoch, lr: rates[epoch])
        hist = model.fit(epochs=3, callbacks=[mt.callbacks.LearningRateScheduler(sched), Watch()], **fit)
        extra["hist_lr"] = hist.history["lr"]
        extra["final_lr"] = model.optimizer.lr
        if step_plan:
            assert len(Watch.seen) == 3 and len(set(Watch.seen)) == 1, Watch.seen
            assert Watch.seen[0][1] > 0
    elif mode == "manual":
        for rate in args["rates"]:                 # the same rates set by hand, one fit per epoch, no callback
            model.optimizer.lr = rate
            model.fit(epochs=1, **fit)
    elif mode == "plain3":
        model.fit(epochs=3, **fit)
    else:
        raise KeyError(mode)
    _dump(model, args["out"], **extra)


def _run(tmp_path, tag, **args):
    out = str(tmp_path / f"{tag}.npz")
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def _same(a, b, skip=()):
    a, b = ({k: v for k, v in d.items() if k not in skip} for d in (a, b))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("opt", ["exp_nesterov", "restarts_adam"])
def test_fit_step_plan_is_bit_identical_to_python_schedule(tmp_path, opt):
    plan = _run(tmp_path, "plan", mode="fit6", opt=opt, step_plan=1)
    eager = _run(tmp_path, "eager", mode="fit6", opt=opt, step_plan=0)
    assert int(plan["iterations"]) == 6 and plan["iter_dev"].tolist() == [6, 0]
    _same(plan, eager)


@pytest.mark.parametrize("opt", ["exp_nesterov", "restarts_adam"])
def test_one_step_matches_formula_on_its_own_gradient(opt):
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.voxelizer import Voxelizer
    from test_gpu_optimizers import _cloud, _targets
    from test_optimizer_semantics import keras_adam, keras_sgd
    model = mt.createModel(16, 32, 8, 35)
    o = _make_opt(opt)
    model.compile(optimizer=o, loss=['mse', 'mse'])
    net, spec, dev = model.net, o.spec(), model.net.device
    net.iterations = 4                                       # lr_t = schedule(4) / (1 + decay*4)
    for name in spec.slots:
        net.slot(name).copy_(torch.rand_like(net.params.theta) * 1e-3)
    theta0 = net.params.theta.cpu().numpy().copy()
    slots0 = [net.slot(name).cpu().numpy().copy() for name in spec.slots]
    sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(0)).to(dev))
    yc, yr = (torch.from_numpy(a).to(dev) for a in _targets(0))
    net.forward(sample, training=True)
    net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
    net.apply_gradients(opt=spec)
    torch.cuda.synchronize()
    g = net.grad.cpu().numpy()
    assert np.abs(g).max() > 0 and net.iterations == 5 and net._iter_dev.cpu().tolist() == [5, 0]
    lr4 = o.lr(4)
    assert lr4 != o.lr(0)
    if spec.kind == "sgd":
        th, v = keras_sgd(theta0, slots0[0], g, 4, lr4, o.decay, o.momentum, o.nesterov)
        ref_slots = [v]
    else:
        th, m, v, _ = keras_adam(theta0, slots0[0], slots0[1], None, g, 4, lr4, o.decay, o.beta_1, o.beta_2, o.epsilon,
                                 False)
        ref_slots = [m, v]
    got = net.params.theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, float(err.max())
    assert not np.array_equal(got, theta0)
    for name, s_ref in zip(spec.slots, ref_slots):
        s_got = net.slot(name).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())


@pytest.mark.parametrize("opt", ["exp_nesterov", "restarts_adam"])
def test_save_load_resume_continues_the_schedule(tmp_path, opt):
    """3 steps -> Model.save (the schedule in training_config) -> load_model -> 3 steps == 6 steps."""
    ckpt = str(tmp_path / "ckpt.h5")
    whole = _run(tmp_path, "whole", mode="fit6", opt=opt, step_plan=1)
    half = _run(tmp_path, "half", mode="save", opt=opt, step_plan=1, ckpt=ckpt)
    assert int(half["iterations"]) == 3
    from lisec_amd import keras_h5
    from lisec_amd import model_training as mt
    ck = keras_h5.load_model(ckpt)
    assert ck["iterations"] == 3
    assert ck["optimizer"]["lr"] == mt.optimizers.schedules.serialize(_make_opt(opt).lr)
    resumed = _run(tmp_path, "resumed", mode="resume", opt=opt, step_plan=1, ckpt=ckpt)
    _same(whole, resumed)


@pytest.mark.parametrize("opt", ["nesterov", "adam"])
def test_learning_rate_scheduler_across_epochs(tmp_path, opt):
    """Rates set by the callback reach the recorded step (one plan for the three epochs) and give the variables of an
    eager run that sets the same rates by hand; History.history['lr'] holds them."""
    rates = [0.004, 0.002, 0.0005] if opt == "nesterov" else [1e-3, 5e-4, 2.5e-4]
    lrs = _run(tmp_path, "lrs", mode="lrs", opt=opt, step_plan=1, rates=rates)
    assert lrs["hist_lr"].tolist() == rates and float(lrs["final_lr"]) == rates[-1]
    assert int(lrs["iterations"]) == 9
    manual = _run(tmp_path, "manual", mode="manual", opt=opt, step_plan=0, rates=rates)
    _same(lrs, manual, skip=("hist_lr", "final_lr"))


@pytest.mark.parametrize("opt", ["nesterov", "adam"])
def test_scheduler_keeping_the_rate_is_bit_identical_to_no_callback(tmp_path, opt):
    same = _run(tmp_path, "same", mode="lrs_same", opt=opt, step_plan=1)
    plain = _run(tmp_path, "plain", mode="plain3", opt=opt, step_plan=1)
    assert same["hist_lr"].tolist() == [_make_opt(opt).lr] * 3
    _same(same, plain, skip=("hist_lr", "final_lr"))


def _dp_worker(rank, world, port, out_dir, opt):
    import torch
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is not None and model.dp.world == 2
    model.compile(optimizer=_make_opt(opt), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=4)
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, steps_per_epoch=4, shuffle=False)
    torch.cuda.synchronize()
    _dump(model, os.path.join(out_dir, f"rank{rank}.npz"))
    model.dp.barrier()
    model.dp.close()


def test_two_ranks_keep_identical_variables_and_slots(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), "exp_momentum"), nprocs=2, join=True)
    r0, r1 = dict(np.load(tmp_path / "rank0.npz")), dict(np.load(tmp_path / "rank1.npz"))
    assert int(r0["iterations"]) == 4
    for k in r0:
        if k != "state":                                     # BN moving statistics are per replica
            assert np.array_equal(r0[k], r1[k]), k
    assert np.abs(r0["slot_velocity"]).max() > 0


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _worker(json.loads(sys.argv[2]))
