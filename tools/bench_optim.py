"""Cost of the optimizers (GPU box only): Model.fit(batch_size=1) ms/step on the U20k sweeps of bench.py for
SGD-Nesterov (the reference's), SGD with plain momentum, Adam, AMSGrad, RMSprop (plain and centered with momentum),
Adagrad, Adadelta, Adamax and Nadam, alternated over rounds so that drift shows
as spread; then the update kernels alone over the model's 6.49 M variables (device-event timing, us and GB/s of the
bytes each update must move)."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic_targets, u20k_cloud
from lisec_amd import Constants, ops
from lisec_amd import model_training as mt

CONFIGS = {
    "sgd_nesterov": lambda: mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True),
    "sgd_momentum": lambda: mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=False),
    "adam": lambda: mt.optimizers.Adam(learning_rate=1e-3, decay=1e-6),
    "amsgrad": lambda: mt.optimizers.Adam(learning_rate=1e-3, decay=1e-6, amsgrad=True),
    "rmsprop": lambda: mt.optimizers.RMSprop(learning_rate=1e-3, decay=1e-6),
    "rmsprop_cm": lambda: mt.optimizers.RMSprop(learning_rate=1e-3, decay=1e-6, momentum=0.9, centered=True),
    "adagrad": lambda: mt.optimizers.Adagrad(learning_rate=1e-2, decay=1e-6),
    "adadelta": lambda: mt.optimizers.Adadelta(learning_rate=1.0, decay=1e-6),
    "adamax": lambda: mt.optimizers.Adamax(learning_rate=2e-3, decay=1e-6),
    "nadam": lambda: mt.optimizers.Nadam(learning_rate=2e-3),
}
# fp32 arrays each update reads + writes: theta r/w, grad r, and every slot r/w
STREAMS = {"sgd_nesterov": 5, "sgd_momentum": 5, "sgd": 3, "adam": 7, "amsgrad": 9, "rmsprop": 5, "rmsprop_c": 7,
           "rmsprop_m": 7, "rmsprop_cm": 9, "adagrad": 5, "adadelta": 7, "adamax": 7, "nadam": 7}


def fit_times(rounds=3, steps=200):
    n = 4
    pts = [u20k_cloud(i).astype(np.float64) for i in range(n)]
    samples = [mt.VFE_preprocessing(p, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                                    Constants.nx // 2, Constants.ny // 2, Constants.nz) for p in pts]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    ycls = np.stack([t[0] for t in tg]).astype(np.float64)
    yreg = np.stack([t[1] for t in tg]).astype(np.float64)
    model = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    times = {k: [] for k in CONFIGS}
    for _ in range(rounds):
        for name, make in CONFIGS.items():
            model.compile(optimizer=make(), loss=['mse', 'mse'])       # a new optimizer config records a new step plan
            model.fit(x=samples, y=[ycls, yreg], batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = model.fit(x=samples, y=[ycls, yreg], batch_size=1, verbose=0, epochs=1, steps_per_epoch=steps)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / steps)
            assert np.isfinite(hist.history["loss"][-1])
    return times, model.net.params.n_theta


def kernel_times(n, reps=200):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.randn(n, device=dev) * 1e-3
    theta = torch.randn(n, device=dev)
    slots = [torch.zeros(n, device=dev) for _ in range(3)]
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    cache = torch.ones(1, device=dev)
    s0, s1, s2 = slots
    runs = {
        "sgd_nesterov": lambda: ops.sgd_nesterov_step_dev(theta, g, slots[0], 0.01, 1e-6, 0.9, state),
        "sgd_momentum": lambda: ops.sgd_step_dev(theta, g, slots[0], 0.01, 1e-6, 0.9, False, state),
        "sgd": lambda: ops.sgd_step_dev(theta, g, None, 0.01, 1e-6, 0.0, False, state),
        "adam": lambda: ops.adam_step_dev(theta, g, slots[0], slots[1], None, 1e-3, 1e-6, 0.9, 0.999, 1e-7, state),
        "amsgrad": lambda: ops.adam_step_dev(theta, g, slots[0], slots[1], slots[2], 1e-3, 1e-6, 0.9, 0.999, 1e-7, state),
        "rmsprop": lambda: ops.rmsprop_step_dev(theta, g, s0, None, None, 1e-3, 1e-6, 0.9, 0.0, 1e-7, state),
        "rmsprop_c": lambda: ops.rmsprop_step_dev(theta, g, s0, None, s2, 1e-3, 1e-6, 0.9, 0.0, 1e-7, state),
        "rmsprop_m": lambda: ops.rmsprop_step_dev(theta, g, s0, s1, None, 1e-3, 1e-6, 0.9, 0.9, 1e-7, state),
        "rmsprop_cm": lambda: ops.rmsprop_step_dev(theta, g, s0, s1, s2, 1e-3, 1e-6, 0.9, 0.9, 1e-7, state),
        "adagrad": lambda: ops.adagrad_step_dev(theta, g, s0, 1e-2, 1e-6, 1e-7, state),
        "adadelta": lambda: ops.adadelta_step_dev(theta, g, s0, s1, 1.0, 1e-6, 0.95, 1e-7, state),
        "adamax": lambda: ops.adamax_step_dev(theta, g, s0, s1, 2e-3, 1e-6, 0.9, 0.999, 1e-7, state),
        "nadam": lambda: ops.nadam_step_dev(theta, g, s0, s1, cache, 2e-3, 0.9, 0.999, 1e-7, 0.004, state),
    }
    out = {}
    for name, fn in runs.items():
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = 1e3 * a.elapsed_time(b) / reps
        out[name] = (us, STREAMS[name] * 4 * n / (us * 1e-6) / 1e9)
    return out


if __name__ == "__main__":
    times, n = fit_times()
    base = np.median(times["sgd_nesterov"])
    print(f"Model.fit ms/step, U20k sweeps, Lyft grid, {len(times['adam'])} alternating rounds of 200 steps "
          f"(median [min..max], ratio to SGD-Nesterov):")
    for name, t in times.items():
        print(f"  {name:13s} {np.median(t):.4f} [{min(t):.4f}..{max(t):.4f}]  x{np.median(t) / base:.4f}")
    print(f"update kernels alone, {n:,} variables (device events, mean of 200 back-to-back launches):")
    for name, (us, gbs) in kernel_times(n).items():
        print(f"  {name:13s} {us:8.1f} us  {STREAMS[name]} x {4 * n / 1e6:.1f} MB  {gbs:7.0f} GB/s")
