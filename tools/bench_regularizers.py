"""Cost of the weight-regularizer pass in the training step (GPU box only).

    python tools/bench_regularizers.py [--cloud u20k|r200k] [--windows 6] [--steps 400]

Model.fit(batch_size=1) on the 20 000-point sweep with kernel_regularizer=regularizers.l2(1e-4) and without, two models
in one process, in alternating windows of about 1.4 s (each preceded by a 20-step warm-up fit of its model, which also
records its step plan the first time): the median step time per mode, the spread of its windows, and the ratio.  The
unregularised model issues the launches it always did (its step plan has the size it had).  A commit from before the
regularizers cannot run this tool; to compare the unregularised step with one, alternate `bench.py` and
`tools/bench_fit.py` of the two trees in one session, and read this tool's `plain` window spread for how far two such
runs may differ by chance."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import r200k_cloud, synthetic_targets, u20k_cloud
from lisec_amd import Constants, _lib
from lisec_amd import model_training as mt

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", choices=("u20k", "r200k"), default="u20k")
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--steps", type=int, default=400)
    args = ap.parse_args()
    _lib.require_gpu()
    n = 4
    cloud = u20k_cloud if args.cloud == "u20k" else r200k_cloud
    samples = [mt.VFE_preprocessing(cloud(i).astype(np.float64), Constants.voxelx, Constants.voxely, Constants.voxelz,
                                    Constants.maxPoints, Constants.nx // 2, Constants.ny // 2, Constants.nz) for i in range(n)]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    y = [np.stack([t[0] for t in tg]).astype(np.float64), np.stack([t[1] for t in tg]).astype(np.float64)]
    models = {}
    for mode, kw in (("plain", {}), ("l2(1e-4) on kernels", dict(kernel_regularizer=mt.regularizers.l2(1e-4)))):
        m = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints, **kw)
        m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
        models[mode] = m
    ms = {mode: [] for mode in models}
    loss = {}
    for _ in range(args.windows):
        for mode, m in models.items():
            m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = m.fit(x=samples, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=args.steps)
            torch.cuda.synchronize()
            ms[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
            loss[mode] = hist.history["loss"][-1]
    for mode, a in ms.items():
        m = models[mode]
        size = _lib.load().lisec_step_plan_size(m._captured[1].plans[0]) if m._captured is not None else 0
        print(f"Model.fit ({args.cloud}), {mode}: median {np.median(a):.3f} ms/step (windows {min(a):.3f} .. {max(a):.3f}, "
              f"{args.windows} x {args.steps} steps), step plan of {size} operations, {len(m.net._reg or ())} chunks, "
              f"loss {loss[mode]:.4f}")
    a, b = (np.median(v) for v in ms.values())
    print(f"regularised / plain = {b / a:.4f}  ({1e3 * (b - a):+.1f} us per step)")
