"""Cost of weight averaging (optimizers.MovingAverage) in the training step (GPU box only).

    python tools/bench_weight_average.py [--cloud u20k|r200k] [--windows 7] [--steps 400] [--reps 200]

(a) lisec_weight_average alone over a buffer of the model's 6 491 024 variables: device events around --reps passes after a
    warm-up, as us per pass and as a share of the 8 TB/s HBM peak (12 bytes per float: two reads, one write); the same
    for lisec_weight_swap (16 bytes per float).
(b) Model.fit(batch_size=1) on the Lyft grid and the 20 000-point sweep with MovingAverage(SGD) and with the same SGD
    alone, in one process, in alternating windows (each preceded by a 20-step warm-up fit of its model, which also records
    its step plan the first time): steps per second per mode as the median of the windows.  A SECOND model without the
    wrapper runs in the same rotation: the difference between the two identical models is the spread that two equal runs
    show by chance, and the measure of whether the wrapped step can be told from the plain one.
(c) A commit from before the wrappers cannot run this tool.  To compare the unwrapped step with one, alternate `bench.py`
    of the two trees in one session and hold the difference against the spread of (b); the unwrapped model's step plan has
    the size it had (printed here), i.e. it issues the same launches."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import r200k_cloud, synthetic_targets, u20k_cloud
from lisec_amd import Constants, _lib, ops
from lisec_amd import model_training as mt

HBM_PEAK = 8.0e12            # bytes per second


def pass_alone(n, reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    theta = torch.randn(n, dtype=torch.float32, device=dev)
    avg = theta.clone()
    state = torch.tensor([1000, 0], dtype=torch.int64, device=dev)
    desc = _lib.WeightAverage(_lib.AVG_EMA, 1, 0, 1, 0.99)
    calls = (("lisec_weight_average (EMA)", 12, lambda: ops.weight_average(theta, avg, desc, state, state_bias=-1)),
             ("lisec_weight_swap", 16, lambda: ops.weight_swap(theta, avg)))
    for name, bytes_per_float, call in calls:
        for _ in range(20):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        us = 1e3 * t0.elapsed_time(t1) / reps
        rate = bytes_per_float * n / (us * 1e-6)
        print(f"(a) {name}: {us:.2f} us per pass over {n} floats ({bytes_per_float * n / 1e6:.1f} MB), "
              f"{rate / 1e12:.2f} TB/s = {rate / HBM_PEAK:.2f} of the HBM peak ({reps} back-to-back passes, launch gaps included)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", choices=("u20k", "r200k"), default="u20k")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    _lib.require_gpu()
    n = 4
    cloud = u20k_cloud if args.cloud == "u20k" else r200k_cloud
    samples = [mt.VFE_preprocessing(cloud(i).astype(np.float64), Constants.voxelx, Constants.voxely, Constants.voxelz,
                                    Constants.maxPoints, Constants.nx // 2, Constants.ny // 2, Constants.nz) for i in range(n)]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    y = [np.stack([t[0] for t in tg]).astype(np.float64), np.stack([t[1] for t in tg]).astype(np.float64)]

    def sgd():
        return mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)

    models = {}
    for mode, opt in (("plain", sgd()), ("MovingAverage", mt.optimizers.MovingAverage(sgd(), average_decay=0.99)),
                      ("plain again", sgd())):
        m = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
        m.compile(optimizer=opt, loss=['mse', 'mse'])
        models[mode] = m
    pass_alone(models["plain"].net.params.n_theta, args.reps)
    rate = {mode: [] for mode in models}
    for _ in range(args.windows):
        for mode, m in models.items():
            m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=args.steps)
            torch.cuda.synchronize()
            rate[mode].append(args.steps / (time.perf_counter() - t0))
    for mode, a in rate.items():
        m = models[mode]
        size = _lib.load().lisec_step_plan_size(m._captured[1].plans[0]) if m._captured is not None else 0
        print(f"(b) Model.fit ({args.cloud}), {mode}: median {np.median(a):.1f} steps/s (windows {min(a):.1f} .. {max(a):.1f}, "
              f"{args.windows} x {args.steps} steps), step plan of {size} operations")
    med = {mode: float(np.median(a)) for mode, a in rate.items()}
    print(f"(b) MovingAverage / plain = {med['MovingAverage'] / med['plain']:.4f}; plain again / plain = "
          f"{med['plain again'] / med['plain']:.4f} (two identical models: the spread of equal runs)")
