"""tf.keras RMSprop, Adagrad, Adadelta, Adamax and Nadam on the GPU: the kernels of csrc/optim_keras.hip through the C
ABI against the fp64 formulas of tests/test_keras_optimizers.py (by value and from a CONSTANT descriptor), the split
step, bad arguments, then Model.fit on the small grid -- step plan against the Python schedule, one step against the
formula on the step's own gradient, save / load_model in the middle of a run, LearningRateScheduler, and two
data-parallel ranks."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
SMALL = dict(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)
N_MODEL = 6_491_024                       # trainable variables of the Lisec network (params.py)
LR, DECAY, SD = 0.01, 1e-3, 0.004

KERNEL_CONFIGS = {
    "rmsprop": dict(kind="rmsprop", momentum=0.0, centered=False),
    "rmsprop_centered": dict(kind="rmsprop", momentum=0.0, centered=True),
    "rmsprop_momentum": dict(kind="rmsprop", momentum=0.9, centered=False),
    "rmsprop_centered_momentum": dict(kind="rmsprop", momentum=0.9, centered=True),
    "adagrad": dict(kind="adagrad"),
    "adadelta": dict(kind="adadelta"),
    "adamax": dict(kind="adamax"),
    "nadam": dict(kind="nadam"),
}


def _n_slots(cfg):
    if cfg["kind"] == "rmsprop":
        return 1 + (cfg["momentum"] > 0) + cfg["centered"]
    return 1 if cfg["kind"] == "adagrad" else 2


def _init_slots(cfg, n, dev):
    import torch
    fill = 0.1 if cfg["kind"] == "adagrad" else 0.0
    return [torch.full((n,), fill, dtype=torch.float32, device=dev) for _ in range(_n_slots(cfg))]


# ---- kernels through the C ABI ----------------------------------------------------------------------------------------
def _launch(cfg, theta, grad, slots, state, cache, advance, desc=None, lo=0, hi=None):
    """One update of theta[lo:hi]; desc: a device descriptor (the *_sched entries) instead of (LR, DECAY)."""
    from lisec_amd import ops
    hi = theta.numel() if hi is None else hi
    th, g = theta[lo:hi], grad[lo:hi]
    s = [t[lo:hi] for t in slots]
    k = cfg["kind"]
    if k == "rmsprop":
        mom = s[1] if cfg["momentum"] > 0 else None
        mg = s[-1] if cfg["centered"] else None
        if desc is None:
            ops.rmsprop_step_dev(th, g, s[0], mom, mg, LR, DECAY, 0.9, cfg["momentum"], 1e-7, state, advance=advance)
        else:
            ops.rmsprop_step_sched(th, g, s[0], mom, mg, desc, 0.9, cfg["momentum"], 1e-7, state, advance=advance)
    elif k == "adagrad":
        if desc is None:
            ops.adagrad_step_dev(th, g, s[0], LR, DECAY, 1e-7, state, advance=advance)
        else:
            ops.adagrad_step_sched(th, g, s[0], desc, 1e-7, state, advance=advance)
    elif k == "adadelta":
        if desc is None:
            ops.adadelta_step_dev(th, g, s[0], s[1], LR, DECAY, 0.95, 1e-7, state, advance=advance)
        else:
            ops.adadelta_step_sched(th, g, s[0], s[1], desc, 0.95, 1e-7, state, advance=advance)
    elif k == "adamax":
        if desc is None:
            ops.adamax_step_dev(th, g, s[0], s[1], LR, DECAY, 0.9, 0.999, 1e-7, state, advance=advance)
        else:
            ops.adamax_step_sched(th, g, s[0], s[1], desc, 0.9, 0.999, 1e-7, state, advance=advance)
    elif desc is None:
        ops.nadam_step_dev(th, g, s[0], s[1], cache, LR, 0.9, 0.999, 1e-7, SD, state, advance=advance)
    else:
        ops.nadam_step_sched(th, g, s[0], s[1], cache, desc, 0.9, 0.999, 1e-7, SD, state, advance=advance)


def _reference_step(cfg, th, ref_slots, cache, g, it):
    import test_keras_optimizers as R
    k = cfg["kind"]
    if k == "rmsprop":
        mom = ref_slots[1] if cfg["momentum"] > 0 else None
        mg = ref_slots[-1] if cfg["centered"] else None
        th, rms, mom, mg = R.keras_rmsprop(th, ref_slots[0], mom, mg, g, it, LR, DECAY, 0.9, cfg["momentum"], 1e-7,
                                           cfg["centered"])
        return th, [rms] + ([mom] if mom is not None else []) + ([mg] if mg is not None else []), cache
    if k == "adagrad":
        th, acc = R.keras_adagrad(th, ref_slots[0], g, it, LR, DECAY, 1e-7)
        return th, [acc], cache
    if k == "adadelta":
        th, ag, av = R.keras_adadelta(th, ref_slots[0], ref_slots[1], g, it, LR, DECAY, 0.95, 1e-7)
        return th, [ag, av], cache
    if k == "adamax":
        th, m, v = R.keras_adamax(th, ref_slots[0], ref_slots[1], g, it, LR, DECAY, 0.9, 0.999, 1e-7)
        return th, [m, v], cache
    th, m, v, cache = R.keras_nadam(th, ref_slots[0], ref_slots[1], cache, g, it, LR, 0.9, 0.999, 1e-7, SD)
    return th, [m, v], cache


def _desc(dev, cfg):
    import ctypes
    import torch
    from lisec_amd import _lib, lr_schedules, ops
    d = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device=dev)
    host = lr_schedules.descriptor(LR, 0.0 if cfg["kind"] == "nadam" else DECAY)
    ops.lr_schedule_set(d, host)
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("n", [N_MODEL, 1028])
@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_update_kernels_match_formula(which, n):
    """5 steps from iteration 7: the by-value kernel against the reference; the descriptor kernel with a CONSTANT
    descriptor gives its bits."""
    import torch
    cfg = KERNEL_CONFIGS[which]
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(11)
    theta0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * (1 + step)).astype(np.float32) for step in range(5)]
    start = 7
    runs = []
    for desc in (None, _desc(dev, cfg)):
        theta = torch.from_numpy(theta0).to(dev)
        slots = _init_slots(cfg, n, dev)
        cache = torch.ones(1, dtype=torch.float32, device=dev)
        state = torch.tensor([start, 0], dtype=torch.int64, device=dev)
        for step, g in enumerate(grads):
            _launch(cfg, theta, torch.from_numpy(g).to(dev), slots, state, cache, True, desc=desc)
            st = state.cpu().numpy()
            assert st[0] == start + step + 1 and st[1] == 0                # one increment per step, ticket reset
        runs.append([theta.cpu().numpy()] + [s.cpu().numpy() for s in slots] + [cache.cpu().numpy()])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), which
    th = theta0.astype(np.float64)
    ref_slots = [s.cpu().numpy().astype(np.float64) for s in _init_slots(cfg, n, dev)]
    cache = 1.0
    for step, g in enumerate(grads):
        th, ref_slots, cache = _reference_step(cfg, th, ref_slots, cache, g, start + step)
    got = runs[0][0].astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, (which, float(err.max()))
    assert not np.array_equal(runs[0][0], theta0)
    for s_got, s_ref in zip(runs[0][1:-1], ref_slots):
        np.testing.assert_allclose(s_got.astype(np.float64), s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())
    if cfg["kind"] == "nadam":
        assert abs(float(runs[0][-1][0]) - cache) <= 1e-6 * abs(cache) and cache < 0.9 ** 5
    else:
        assert float(runs[0][-1][0]) == 1.0                              # only Nadam touches the cache


@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_part_then_rest_is_bit_identical_to_one_launch(which, sched):
    """advance=0 over [lo:] (the early update under the backward), then advance=1 over [:lo]: the same bits as one launch
    over everything; the iteration count advances once per step, and so does Nadam's cache."""
    import torch
    import test_keras_optimizers as R
    cfg = KERNEL_CONFIGS[which]
    dev = torch.device("cuda", torch.cuda.current_device())
    desc = _desc(dev, cfg) if sched else None
    rng = np.random.default_rng(12)
    n, lo = N_MODEL, 388_168
    theta0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    slots0 = [torch.from_numpy(np.abs(rng.standard_normal(n)).astype(np.float32) * 0.01).to(dev)
              for _ in range(_n_slots(cfg))]
    runs = []
    for split in (False, True):
        theta, slots = theta0.clone(), [s.clone() for s in slots0]
        cache = torch.ones(1, dtype=torch.float32, device=dev)
        state = torch.tensor([41, 0], dtype=torch.int64, device=dev)
        caches = []
        for step in range(3):
            g = torch.from_numpy(np.random.default_rng(100 + step).standard_normal(n).astype(np.float32)).to(dev)
            if split:
                _launch(cfg, theta, g, slots, state, cache, False, desc=desc, lo=lo)
                _launch(cfg, theta, g, slots, state, cache, True, desc=desc, hi=lo)
            else:
                _launch(cfg, theta, g, slots, state, cache, True, desc=desc)
            caches.append(float(cache.item()))
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [44, 0]
        if cfg["kind"] == "nadam":
            want, c = [], 1.0
            for it in range(41, 44):
                c = float(R.nadam_scalars(c, it, 0.9, 0.999, SD)[2])
                want.append(c)
            np.testing.assert_allclose(caches, want, rtol=1e-6)
        runs.append([theta.cpu().numpy()] + [s.cpu().numpy() for s in slots] + [cache.cpu().numpy()])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), which


def test_bad_arguments_are_refused_and_enqueue_nothing():
    import torch
    from lisec_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 40_004
    rng = np.random.default_rng(13)
    th = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    th0 = th.clone()
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    a, b, c = (torch.zeros(n, device=dev) for _ in range(3))
    cache = torch.ones(1, dtype=torch.float32, device=dev)
    st = torch.tensor([6, 0], dtype=torch.int64, device=dev)
    desc = _desc(dev, dict(kind="adagrad"))
    lib, P, s = _lib.load(), _lib.ptr, _lib.current_stream()
    T, G, A, B, C, S, D, K = P(th), P(g), P(a), P(b), P(c), P(st), P(desc), P(cache)
    bad = [
        lib.lisec_rmsprop_step_dev(T, G, A, None, None, n, 1e-3, 0.0, 0.9, 0.9, 1e-7, 0, S, 1, s),      # momentum, no mom
        lib.lisec_rmsprop_step_dev(T, G, A, B, None, n, 1e-3, 0.0, 0.9, 0.0, 1e-7, 0, S, 1, s),         # mom, no momentum
        lib.lisec_rmsprop_step_dev(T, G, A, None, None, n, 1e-3, 0.0, 0.9, 0.0, 1e-7, 1, S, 1, s),      # centered, no mg
        lib.lisec_rmsprop_step_dev(T, G, A, None, C, n, 1e-3, 0.0, 0.9, 0.0, 1e-7, 0, S, 1, s),         # mg, not centered
        lib.lisec_rmsprop_step_dev(T, G, None, None, None, n, 1e-3, 0.0, 0.9, 0.0, 1e-7, 0, S, 1, s),   # no rms
        lib.lisec_rmsprop_step_dev(T, G, A, None, None, n, 1e-3, 0.0, 1.0, 0.0, 1e-7, 0, S, 1, s),      # rho = 1
        lib.lisec_rmsprop_step_sched(T, G, A, None, None, 10, D, 0.9, 0.0, 1e-7, 0, S, 1, s),           # n % 4
        lib.lisec_rmsprop_step_sched(T, G, A, None, None, n, None, 0.9, 0.0, 1e-7, 0, S, 1, s),         # no descriptor
        lib.lisec_adagrad_step_dev(T, G, None, n, 1e-3, 0.0, 1e-7, S, 1, s),
        lib.lisec_adagrad_step_dev(T, G, A, n, 1e-3, 0.0, -1e-7, S, 1, s),                              # epsilon < 0
        lib.lisec_adagrad_step_sched(T, G, A, n, D, 1e-7, S, 2, s),                                     # advance = 2
        lib.lisec_adadelta_step_dev(T, G, A, None, n, 1.0, 0.0, 0.95, 1e-7, S, 1, s),
        lib.lisec_adadelta_step_sched(T, G, A, B, n, D, -0.1, 1e-7, S, 1, s),                           # rho < 0
        lib.lisec_adamax_step_dev(T, G, A, B, n, 1e-3, 0.0, 1.0, 0.999, 1e-7, S, 1, s),                 # beta_1 = 1
        lib.lisec_adamax_step_sched(T, G, None, B, n, D, 0.9, 0.999, 1e-7, S, 1, s),
        lib.lisec_nadam_step_dev(T, G, A, B, None, n, 1e-3, 0.9, 0.999, 1e-7, 0.004, S, 1, s),          # no cache
        lib.lisec_nadam_step_dev(T, G, A, B, K, 6, 1e-3, 0.9, 0.999, 1e-7, 0.004, S, 1, s),
        lib.lisec_nadam_step_sched(T, G, A, B, K, n, D, 0.9, 1.5, 1e-7, 0.004, S, 1, s),                # beta_2 > 1
        lib.lisec_nadam_step_sched(T, G, A, B, K, n, D, 0.9, 0.999, 1e-7, 0.004, S, -1, s),
    ]
    assert all(r != 0 for r in bad), bad
    torch.cuda.synchronize()
    assert torch.equal(th, th0) and st.cpu().tolist() == [6, 0] and float(cache.item()) == 1.0
    assert not a.any() and not b.any() and not c.any()


# ---- Model.fit on the small grid (worker processes: the step-plan knob is read once per process) -----------------------
def _make_opt(name):
    from lisec_amd import model_training as mt
    O = mt.optimizers
    return {"rmsprop": lambda: O.RMSprop(learning_rate=1e-3, decay=1e-3),
            "rmsprop_cm": lambda: O.RMSprop(learning_rate=1e-3, decay=1e-3, momentum=0.9, centered=True),
            "adagrad": lambda: O.Adagrad(learning_rate=1e-2, decay=1e-3),
            "adadelta": lambda: O.Adadelta(learning_rate=1.0, decay=1e-3),
            "adamax": lambda: O.Adamax(learning_rate=2e-3, decay=1e-3),
            "nadam": lambda: O.Nadam(learning_rate=2e-3)}[name]()


def _dump(model, path, **extra):
    import torch
    torch.cuda.synchronize()
    net = model.net
    d = dict(theta=net.params.theta.cpu().numpy(), state=net.params.state.cpu().numpy(),
             iterations=np.array(net.iterations), iter_dev=net._iter_dev.cpu().numpy(),
             momentum_cache=net.momentum_cache.cpu().numpy(), **extra)
    for name in model.optimizer.spec().slots:
        d["slot_" + name] = net.slot(name).cpu().numpy()
    np.savez(path, **d)


def _worker(args):
    """One fit scenario in a fresh process; writes its variables, BN state, slots, iteration count and momentum_cache."""
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
    elif mode == "lrs":
        from lisec_amd import _lib

        class Watch(mt.callbacks.Callback):
            seen = []

            def on_epoch_end(self, epoch, logs=None):
                cap = getattr(self.model, "_captured", None)
                if cap is not None:
                    self.seen.append((id(cap[1]), _lib.load().lisec_step_plan_size(cap[1].plans[0])))

        rates = args["rates"]
        hist = model.fit(epochs=3, callbacks=[mt.callbacks.LearningRateScheduler(lambda epoch, lr: rates[epoch]),
                                              Watch()], **fit)
        extra["hist_lr"] = np.array(hist.history["lr"])
        assert len(Watch.seen) == 3 and len(set(Watch.seen)) == 1, Watch.seen
    elif mode == "manual":
        for rate in args["rates"]:                 # the same rates set by hand, one fit per epoch, no callback
            model.optimizer.lr = rate
            model.fit(epochs=1, **fit)
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


@pytest.mark.parametrize("opt", ["rmsprop_cm", "adagrad", "adadelta", "adamax", "nadam"])
def test_fit_step_plan_is_bit_identical_to_python_schedule(tmp_path, opt):
    plan = _run(tmp_path, "plan", mode="fit6", opt=opt, step_plan=1)
    eager = _run(tmp_path, "eager", mode="fit6", opt=opt, step_plan=0)
    assert int(plan["iterations"]) == 6 and plan["iter_dev"].tolist() == [6, 0]
    assert (float(plan["momentum_cache"][0]) < 1.0) == (opt == "nadam")
    _same(plan, eager)


@pytest.mark.parametrize("opt", ["rmsprop", "rmsprop_cm", "adagrad", "adadelta", "adamax", "nadam"])
def test_one_step_matches_formula_on_its_own_gradient(opt):
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.voxelizer import Voxelizer
    import test_keras_optimizers as R
    from test_gpu_optimizers import _cloud, _targets
    model = mt.createModel(16, 32, 8, 35)
    o = _make_opt(opt)
    model.compile(optimizer=o, loss=['mse', 'mse'])
    net, spec, dev = model.net, o.spec(), model.net.device
    if opt == "adagrad":
        assert torch.all(net.slot("accumulator") == np.float32(0.1))
    assert float(net.momentum_cache.item()) == 1.0
    net.iterations = 4                                       # lr_t and the per-step scalars at it = 4
    for name in spec.slots:                                  # a non-zero starting state
        net.slot(name).copy_(torch.rand_like(net.params.theta) * 1e-3)
    if spec.kind == "rmsprop" and o.centered:                # a reachable state: the mean square is >= the squared mean
        net.slot("rms").add_(net.slot("mg") ** 2)
    net.momentum_cache.fill_(0.75)
    theta0 = net.params.theta.cpu().numpy().copy()
    s0 = [net.slot(name).cpu().numpy().copy() for name in spec.slots]
    sample = Voxelizer(**SMALL, device=dev)(torch.from_numpy(_cloud(0)).to(dev))
    yc, yr = (torch.from_numpy(a).to(dev) for a in _targets(0))
    net.forward(sample, training=True)
    net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
    assert net._early is not None                            # the early update under the backward pass ran
    net.apply_gradients(opt=spec)
    torch.cuda.synchronize()
    g = net.grad.cpu().numpy()
    assert np.abs(g).max() > 0 and net.iterations == 5 and net._iter_dev.cpu().tolist() == [5, 0]
    cache = 0.75
    if spec.kind == "rmsprop":
        mom = s0[1] if o.momentum > 0 else None
        mg = s0[-1] if o.centered else None
        th, rms, mom, mg = R.keras_rmsprop(theta0, s0[0], mom, mg, g, 4, o.lr, o.decay, o.rho, o.momentum, o.epsilon,
                                           o.centered)
        ref = [rms] + ([mom] if mom is not None else []) + ([mg] if mg is not None else [])
    elif spec.kind == "adagrad":
        th, acc = R.keras_adagrad(theta0, s0[0], g, 4, o.lr, o.decay, o.epsilon)
        ref = [acc]
    elif spec.kind == "adadelta":
        th, ag, av = R.keras_adadelta(theta0, s0[0], s0[1], g, 4, o.lr, o.decay, o.rho, o.epsilon)
        ref = [ag, av]
    elif spec.kind == "adamax":
        th, m, v = R.keras_adamax(theta0, s0[0], s0[1], g, 4, o.lr, o.decay, o.beta_1, o.beta_2, o.epsilon)
        ref = [m, v]
    else:
        th, m, v, cache = R.keras_nadam(theta0, s0[0], s0[1], 0.75, g, 4, o.lr, o.beta_1, o.beta_2, o.epsilon, o.decay)
        ref = [m, v]
    got = net.params.theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, float(err.max())
    assert not np.array_equal(got, theta0)
    for name, s_ref in zip(spec.slots, ref):
        s_got = net.slot(name).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())
    assert abs(float(net.momentum_cache.item()) - cache) <= 1e-6 * cache


@pytest.mark.parametrize("opt", ["rmsprop_cm", "adagrad", "nadam"])
def test_save_load_resume_is_bit_identical(tmp_path, opt):
    """3 steps -> Model.save (Keras .h5) -> load_model (compiled, iteration count, slots, momentum_cache) -> 3 steps ==
    6 steps."""
    ckpt = str(tmp_path / "ckpt.h5")
    whole = _run(tmp_path, "whole", mode="fit6", opt=opt, step_plan=1)
    half = _run(tmp_path, "half", mode="save", opt=opt, step_plan=1, ckpt=ckpt)
    assert int(half["iterations"]) == 3
    from lisec_amd import keras_h5
    ck = keras_h5.load_model(ckpt)
    assert ck["iterations"] == 3 and ck["optimizer"]["class_name"] == type(_make_opt(opt)).__name__
    if opt == "nadam":
        assert ck["momentum_cache"] == float(half["momentum_cache"][0]) < 1.0
    resumed = _run(tmp_path, "resumed", mode="resume", opt=opt, step_plan=1, ckpt=ckpt)
    _same(whole, resumed)


@pytest.mark.parametrize("opt", ["nadam", "adadelta"])
def test_learning_rate_scheduler_across_epochs(tmp_path, opt):
    """Rates set by the callback reach the recorded step (one plan for the three epochs) and give the variables of an
    eager run that sets the same rates by hand."""
    rates = [2e-3, 1e-3, 2.5e-4] if opt == "nadam" else [1.0, 0.5, 0.25]
    lrs = _run(tmp_path, "lrs", mode="lrs", opt=opt, step_plan=1, rates=rates)
    assert lrs["hist_lr"].tolist() == rates and int(lrs["iterations"]) == 9
    manual = _run(tmp_path, "manual", mode="manual", opt=opt, step_plan=0, rates=rates)
    _same(lrs, manual, skip=("hist_lr",))


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
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=4, shuffle=False)
    torch.cuda.synchronize()
    _dump(model, os.path.join(out_dir, f"rank{rank}.npz"))
    model.dp.barrier()
    model.dp.close()


@pytest.mark.parametrize("opt", ["nadam", "rmsprop_cm"])
def test_two_ranks_keep_identical_variables_slots_and_cache(tmp_path, opt):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), opt), nprocs=2, join=True)
    r0, r1 = dict(np.load(tmp_path / "rank0.npz")), dict(np.load(tmp_path / "rank1.npz"))
    assert int(r0["iterations"]) == 2
    for k in r0:
        if k != "state":                                     # BN moving statistics are per replica
            assert np.array_equal(r0[k], r1[k]), k
    assert np.abs(r0["slot_" + _make_opt(opt).spec().slots[0]]).max() > 0
    assert (float(r0["momentum_cache"][0]) < 1.0) == (opt == "nadam")


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _worker(json.loads(sys.argv[2]))
