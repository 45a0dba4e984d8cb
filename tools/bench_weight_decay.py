"""Cost of decoupled weight decay (optimizers.AdamW) in the training step (GPU box only).

    python tools/bench_weight_decay.py [--cloud u20k|r200k] [--windows 7] [--steps 400] [--reps 200]

(a) lisec_weight_decay alone over the model's 6 491 024 variables, all of them and the kernels only: device events around
    --reps passes after a warm-up, as us per pass and as a share of the 8 TB/s HBM peak (8 bytes per decayed float: one
    read, one write).
(b) Model.fit(batch_size=1) on the Lyft grid and the 20 000-point sweep of bench.py, replayed from the recorded step plan,
    with Adam, with AdamW decaying every variable and with AdamW decaying the kernels only, in one process, in
    alternating windows (each preceded by a 20-step warm-up fit of its model, which also records its step plan the first
    time): ms per step per case as the median of the windows, with the windows' range.  A SECOND Adam model runs in the
    same rotation: the difference between the two identical models is the spread that two equal runs show by chance.
(c) On a commit from before AdamW the tool runs the Adam case alone (copy it there): the figure to hold this commit's Adam
    case against, in one session."""
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
HAVE_DECAY = hasattr(mt.optimizers, "AdamW")


def pass_alone(net, reps):
    dev = net.device
    theta = torch.randn(net.params.n_theta, dtype=torch.float32, device=dev)
    state = torch.tensor([1000, 0], dtype=torch.int64, device=dev)
    coeff = torch.zeros_like(net._wd.dev)
    ops.lr_schedule_set(coeff, mt.lr_schedules.descriptor(1e-4, 0.0))
    for what, variables in (("every variable", None), ("the kernels", ("kernel",))):
        table = net.decay_table(variables)
        n = sum(c for _, c in table.rows)

        def call():
            ops.weight_decay(theta, table, len(table), coeff, state)
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
        rate = 8 * n / (us * 1e-6)
        print(f"(a) lisec_weight_decay, {what}: {us:.2f} us per pass over {n} floats in {len(table)} chunks "
              f"({8 * n / 1e6:.1f} MB), {rate / 1e12:.2f} TB/s = {rate / HBM_PEAK:.2f} of the HBM peak "
              f"({reps} back-to-back passes, launch gaps included)")


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
    O = mt.optimizers
    cases = [("Adam", lambda: O.Adam(learning_rate=1e-3))]
    if HAVE_DECAY:
        cases += [("AdamW, every variable", lambda: O.AdamW(1e-4, learning_rate=1e-3)),
                  ("AdamW, kernels only", lambda: O.AdamW(1e-4, learning_rate=1e-3, decay_var_list=["kernel"]))]
    cases.append(("Adam again", cases[0][1]))
    models = {}
    for mode, make in cases:
        m = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
        m.compile(optimizer=make(), loss=['mse', 'mse'])
        models[mode] = m
    if HAVE_DECAY:
        pass_alone(models["Adam"].net, args.reps)
    ms = {mode: [] for mode in models}
    for _ in range(args.windows):
        for mode, m in models.items():
            m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=args.steps)
            torch.cuda.synchronize()
            ms[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
    for mode, a in ms.items():
        m = models[mode]
        size = _lib.load().lisec_step_plan_size(m._captured[1].plans[0]) if m._captured is not None else 0
        print(f"(b) Model.fit ({args.cloud}), {mode}: median {np.median(a):.4f} ms per step (windows {min(a):.4f} .. "
              f"{max(a):.4f}, {args.windows} x {args.steps} steps), step plan of {size} operations")
    med = {mode: float(np.median(a)) for mode, a in ms.items()}
    for mode in med:
        if mode != "Adam":
            print(f"(b) {mode} - Adam = {1e3 * (med[mode] - med['Adam']):+.1f} us per step")
