"""tf.keras SGD (no momentum / momentum / Nesterov), Adam and AMSGrad on the GPU: the update kernels of csrc/optim.hip
through the C ABI against the fp64 formulas of tests/test_optimizer_semantics.py, then Model.fit on the small grid --
step plan against the Python schedule, one step against the formula on the step's own gradient, save / load_model in
the middle of a run, re-compiling with another optimizer, and two data-parallel ranks."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

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


def _ref():
    from test_optimizer_semantics import keras_adam, keras_sgd
    return keras_sgd, keras_adam


# ---- kernels through the C ABI ----------------------------------------------------------------------------------------
def _launch(cfg, theta, grad, slots, state, advance, lo=0, hi=None, lr=0.01, decay=1e-3):
    from lisec_amd import ops
    hi = theta.numel() if hi is None else hi
    s = [t[lo:hi] for t in slots]
    if cfg["kind"] == "sgd":
        ops.sgd_step_dev(theta[lo:hi], grad[lo:hi], s[0] if s else None, lr, decay, cfg["momentum"], cfg["nesterov"], state,
                         advance=advance)
    else:
        ops.adam_step_dev(theta[lo:hi], grad[lo:hi], s[0], s[1], s[2] if cfg["amsgrad"] else None, lr, decay, 0.9, 0.999,
                          1e-7, state, advance=advance)


def _n_slots(cfg):
    if cfg["kind"] == "sgd":
        return 1 if cfg["momentum"] > 0 else 0
    return 3 if cfg["amsgrad"] else 2


@pytest.mark.parametrize("n", [N_MODEL, 1028])
@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_update_kernels_match_formula(which, n):
    import torch
    keras_sgd, keras_adam = _ref()
    cfg = KERNEL_CONFIGS[which]
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(11)
    theta0 = rng.standard_normal(n).astype(np.float32)
    k = _n_slots(cfg)
    theta = torch.from_numpy(theta0).to(dev)
    slots = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(k)]
    start = 7
    state = torch.tensor([start, 0], dtype=torch.int64, device=dev)
    th = theta0.astype(np.float64)
    ref_slots = [np.zeros(n) for _ in range(k)]
    for step in range(5):
        g = (rng.standard_normal(n) * (1 + step)).astype(np.float32)
        _launch(cfg, theta, torch.from_numpy(g).to(dev), slots, state, True)
        it = start + step
        if cfg["kind"] == "sgd":
            th, v = keras_sgd(th, ref_slots[0] if k else None, g, it, 0.01, 1e-3, cfg["momentum"], cfg["nesterov"])
            ref_slots = [v] if k else []
        else:
            th, m, v, vh = keras_adam(th, ref_slots[0], ref_slots[1], ref_slots[2] if cfg["amsgrad"] else None, g, it,
                                      0.01, 1e-3, 0.9, 0.999, 1e-7, cfg["amsgrad"])
            ref_slots = [m, v] + ([vh] if cfg["amsgrad"] else [])
        st = state.cpu().numpy()
        assert st[0] == it + 1 and st[1] == 0                       # exactly one increment per step, ticket reset
    got = theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, (which, float(err.max()))
    for s_got, s_ref in zip(slots, ref_slots):
        s_got = s_got.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())


@pytest.mark.parametrize("which", list(KERNEL_CONFIGS))
def test_part_then_rest_is_bit_identical_to_one_launch(which):
    """advance=0 over [lo:] (the early update under the backward), then advance=1 over [:lo]: the same bits as one launch
    over everything, and the iteration count advances once."""
    import torch
    cfg = KERNEL_CONFIGS[which]
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(12)
    n, lo = N_MODEL, 388_168                   # lo: a split point, a multiple of 4 (the early update starts at one)
    k = _n_slots(cfg)
    theta0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    slots0 = [torch.from_numpy(np.abs(rng.standard_normal(n)).astype(np.float32) * 0.01).to(dev) for _ in range(k)]
    runs = []
    for split in (False, True):
        theta, slots = theta0.clone(), [s.clone() for s in slots0]
        state = torch.tensor([41, 0], dtype=torch.int64, device=dev)
        for step in range(3):
            g = torch.from_numpy(np.random.default_rng(100 + step).standard_normal(n).astype(np.float32)).to(dev)
            if split:
                _launch(cfg, theta, g, slots, state, False, lo=lo)
                _launch(cfg, theta, g, slots, state, True, hi=lo)
            else:
                _launch(cfg, theta, g, slots, state, True)
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [44, 0]
        runs.append([theta.cpu().numpy()] + [s.cpu().numpy() for s in slots])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), which


def test_sgd_entry_nesterov_equals_reference_kernel_and_refuses_bad_arguments():
    """lisec_sgd_step_dev(nesterov=1) computes the bits of the reference's lisec_sgd_nesterov_step_dev (which the
    SGD-Nesterov configuration keeps calling); bad arguments return LISEC_EINVAL and enqueue nothing."""
    import torch
    from lisec_amd import _lib, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(13)
    n = 40_004
    th0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    v0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    a, va, sa = th0.clone(), v0.clone(), torch.tensor([5, 0], dtype=torch.int64, device=dev)
    b, vb, sb = th0.clone(), v0.clone(), torch.tensor([5, 0], dtype=torch.int64, device=dev)
    ops.sgd_nesterov_step_dev(a, g, va, 0.01, 1e-6, 0.9, sa)
    ops.sgd_step_dev(b, g, vb, 0.01, 1e-6, 0.9, True, sb)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(va, vb) and torch.equal(sa, sb)
    lib, P = _lib.load(), _lib.ptr
    s = _lib.current_stream()
    assert lib.lisec_sgd_step_dev(P(b), P(g), None, n, 0.01, 0.0, 0.9, 0, P(sb), 1, s) != 0       # momentum without slot
    assert lib.lisec_sgd_step_dev(P(b), P(g), P(vb), n, 0.01, 0.0, 0.0, 0, P(sb), 1, s) != 0      # slot without momentum
    assert lib.lisec_sgd_step_dev(P(b), P(g), None, 6, 0.01, 0.0, 0.0, 0, P(sb), 1, s) != 0       # n % 4
    assert lib.lisec_adam_step_dev(P(b), P(g), P(va), None, None, n, 1e-3, 0.0, 0.9, 0.999, 1e-7, P(sb), 1, s) != 0
    assert lib.lisec_adam_step_dev(P(b), P(g), P(va), P(vb), None, n, 1e-3, 0.0, 1.0, 0.999, 1e-7, P(sb), 1, s) != 0
    assert lib.lisec_adam_step_dev(P(b), P(g), P(va), P(vb), None, 10, 1e-3, 0.0, 0.9, 0.999, 1e-7, P(sb), 1, s) != 0
    torch.cuda.synchronize()
    assert torch.equal(b, a) and sb.cpu().tolist() == [6, 0]


# ---- Model.fit on the small grid (worker processes: the step-plan knob is read once per process) -----------------------
def _make_opt(name):
    from lisec_amd import model_training as mt
    return {"sgd": lambda: mt.optimizers.SGD(lr=0.01, decay=1e-3),
            "momentum": lambda: mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.9, nesterov=False),
            "adam": lambda: mt.optimizers.Adam(learning_rate=1e-3, decay=1e-3),
            "amsgrad": lambda: mt.optimizers.Adam(learning_rate=1e-3, decay=1e-3, amsgrad=True)}[name]()


def _cloud(seed, n=2500):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-4.2, 4.2, n), rng.uniform(-4.2, 4.2, n), rng.uniform(0.0, 2.1, n)], 1)
    return pts.astype(np.float32)


def _targets(seed):
    rng = np.random.default_rng(100 + seed)
    return rng.integers(0, 3, (8, 16, 2)).astype(np.float32), rng.normal(0, 1, (8, 16, 14)).astype(np.float32)


def _data(mt, step_plan, n=3):
    def cloud(s):
        # the plan pads every sweep into its 4096-point buffer with points the voxeliser drops; the Python schedule gets
        # the same padded sweeps (same K-slice plans of the row-list kernels, hence the same summation order)
        c = _cloud(s)
        if step_plan:
            return c
        out = np.full((4096, 3), 1.0e6, np.float32)
        out[:len(c)] = c
        return out
    samples = [mt.VFE_preprocessing(cloud(s), **SMALL) for s in range(n)]
    ys = [_targets(s) for s in range(n)]
    return samples, [np.stack([y[0] for y in ys]), np.stack([y[1] for y in ys])]


def _dump(model, path):
    import torch
    torch.cuda.synchronize()
    net = model.net
    d = dict(theta=net.params.theta.cpu().numpy(), state=net.params.state.cpu().numpy(),
             iterations=np.array(net.iterations), iter_dev=net._iter_dev.cpu().numpy())
    for name in model.optimizer.spec().slots:
        d["slot_" + name] = net.slot(name).cpu().numpy()
    np.savez(path, **d)


def _worker(args):
    """One fit scenario in a fresh process; writes its variables, BN state, slots and iteration count to args['out']."""
    from lisec_amd import model_training as mt
    mode, step_plan = args["mode"], bool(args["step_plan"])
    np.random.seed(0)
    if mode == "resume":
        model = mt.load_model(args["ckpt"])
        assert model.optimizer is not None and model.optimizer.spec() == _make_opt(args["opt"]).spec()
    else:
        model = mt.createModel(16, 32, 8, 35)
        model.compile(optimizer=_make_opt(args["opt"]), loss=['mse', 'mse'])
    x, y = _data(mt, step_plan)
    if mode == "recompile":
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=3, shuffle=False)
        first = getattr(model, "_captured", None)
        model.compile(optimizer=_make_opt(args["opt2"]), loss=['mse', 'mse'])
        assert model.net.iterations == 0 and not model.net.velocity.any()
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=3, shuffle=False)
        second = getattr(model, "_captured", None)
        if step_plan:
            assert first is not None and second is not None and second[1] is not first[1] and second[0] != first[0]
    else:
        epochs = 2 if mode == "fit6" else 1
        model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=epochs, steps_per_epoch=3, shuffle=False)
        assert (getattr(model, "_captured", None) is not None) == step_plan
    if mode == "save":
        model.save(args["ckpt"])
    _dump(model, args["out"])


def _run(tmp_path, tag, **args):
    out = str(tmp_path / f"{tag}.npz")
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("opt", ["adam", "momentum", "amsgrad", "sgd"])
def test_fit_step_plan_is_bit_identical_to_python_schedule(tmp_path, opt):
    plan = _run(tmp_path, "plan", mode="fit6", opt=opt, step_plan=1)
    eager = _run(tmp_path, "eager", mode="fit6", opt=opt, step_plan=0)
    assert int(plan["iterations"]) == 6 and plan["iter_dev"].tolist() == [6, 0]
    _same(plan, eager)


@pytest.mark.parametrize("opt", ["adam", "momentum", "amsgrad", "sgd"])
def test_one_step_matches_formula_on_its_own_gradient(opt):
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.voxelizer import Voxelizer
    keras_sgd, keras_adam = _ref()
    model = mt.createModel(16, 32, 8, 35)
    o = _make_opt(opt)
    model.compile(optimizer=o, loss=['mse', 'mse'])
    net, spec, dev = model.net, o.spec(), model.net.device
    net.iterations = 4                                       # lr_t and the bias corrections at it = 4
    for name in spec.slots:                                  # a non-zero starting state
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
    if spec.kind == "sgd":
        th, v = keras_sgd(theta0, slots0[0] if slots0 else None, g, 4, o.lr, o.decay, o.momentum, o.nesterov)
        ref_slots = [v] if slots0 else []
    else:
        th, m, v, vh = keras_adam(theta0, slots0[0], slots0[1], slots0[2] if o.amsgrad else None, g, 4, o.lr, o.decay,
                                  o.beta_1, o.beta_2, o.epsilon, o.amsgrad)
        ref_slots = [m, v] + ([vh] if o.amsgrad else [])
    got = net.params.theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - th) / np.maximum(1.0, np.abs(th))
    assert err.max() <= 1e-6, float(err.max())
    assert not np.array_equal(got, theta0)
    for name, s_ref in zip(spec.slots, ref_slots):
        s_got = net.slot(name).cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(s_got, s_ref, rtol=1e-5, atol=1e-7 * np.abs(s_ref).max())


@pytest.mark.parametrize("opt", ["adam", "momentum"])
def test_save_load_resume_is_bit_identical(tmp_path, opt):
    """3 steps -> Model.save (Keras .h5) -> load_model (compiled, iteration count and slots) -> 3 steps == 6 steps."""
    ckpt = str(tmp_path / "ckpt.h5")
    whole = _run(tmp_path, "whole", mode="fit6", opt=opt, step_plan=1)
    half = _run(tmp_path, "half", mode="save", opt=opt, step_plan=1, ckpt=ckpt)
    assert int(half["iterations"]) == 3
    from lisec_amd import keras_h5
    ck = keras_h5.load_model(ckpt)
    assert ck["iterations"] == 3
    assert ck["optimizer"]["lr"] == _make_opt(opt).lr
    resumed = _run(tmp_path, "resumed", mode="resume", opt=opt, step_plan=1, ckpt=ckpt)
    _same(whole, resumed)


def test_recompile_with_another_optimizer_records_a_new_plan(tmp_path):
    plan = _run(tmp_path, "plan", mode="recompile", opt="momentum", opt2="adam", step_plan=1)
    eager = _run(tmp_path, "eager", mode="recompile", opt="momentum", opt2="adam", step_plan=0)
    assert int(plan["iterations"]) == 3
    _same(plan, eager)


def _dp_worker(rank, world, port, out_dir, opt):
    import torch
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    from lisec_amd import model_training as mt
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


@pytest.mark.parametrize("opt", ["adam", "momentum"])
def test_two_ranks_keep_identical_variables_and_slots(tmp_path, opt):
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
    assert any(k.startswith("slot_") for k in r0) and np.abs(r0["slot_" + _make_opt(opt).spec().slots[0]]).max() > 0


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _worker(json.loads(sys.argv[2]))
