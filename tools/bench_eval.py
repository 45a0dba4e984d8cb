"""Model.evaluate sweeps/s on the Lyft grid (U20k sweeps of bench.py): the eager forward against the recorded evaluation
step (network.EvalStep, eval_plan=1), in alternating runs; and the cost of validation in Model.fit with the default
(eager) evaluation: 20 % of the sweeps held out as validation_data, every epoch ONE pass over the other 80 %
(steps_per_epoch = the number of training sweeps), timed with and without validation (GPU box only).

    python tools/bench_eval.py [--sweeps 50] [--evals 50] [--epochs 3] [--runs 2]

A LISEC_TUNING the tool is started with holds for every measurement; the tool only adds eval_plan=0|1 to it."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic_targets, u20k_cloud
from lisec_amd import Constants
from lisec_amd import model_training as mt


USER_TUNING = os.environ.get("LISEC_TUNING", "")


def _tuning(plan):
    """The user's LISEC_TUNING with eval_plan set to `plan` (any eval_plan of theirs is replaced)."""
    kept = [kv for kv in USER_TUNING.split(",") if kv.strip() and kv.partition("=")[0].strip() != "eval_plan"]
    os.environ["LISEC_TUNING"] = ",".join(kept + ["eval_plan=%d" % plan])


def _evaluate_rate(model, x, y, n, plan):
    _tuning(plan)
    xs = (x * (-(-n // len(x))))[:n]
    ys = [np.concatenate([y[0]] * (-(-n // len(x))))[:n], np.concatenate([y[1]] * (-(-n // len(x))))[:n]]
    model.evaluate(xs[:len(x)], [ys[0][:len(x)], ys[1][:len(x)]], verbose=0)          # warm-up (records the plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = model.evaluate(xs, ys, verbose=0)[0]
    dt = time.perf_counter() - t0                   # evaluate() ends with the read-back of the sums
    return n / dt, loss


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--evals", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    n = args.sweeps
    pts = [u20k_cloud(i).astype(np.float64) for i in range(n)]
    x = [mt.VFE_preprocessing(p, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                              Constants.nx // 2, Constants.ny // 2, Constants.nz) for p in pts]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    y = [np.stack([t[0] for t in tg]), np.stack([t[1] for t in tg])]
    model = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    model.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    model.fit(x=x, y=y, verbose=0, epochs=1, steps_per_epoch=20)
    for r in range(args.runs):
        for plan in (False, True):
            rate, loss = _evaluate_rate(model, x, y, args.evals, plan)
            print(f"run {r}: evaluate ({'recorded EvalStep' if plan else 'eager forward'}): {rate:.1f} sweeps/s "
                  f"({1e3 / rate:.2f} ms/sweep), loss {loss:.6f}", flush=True)
    _tuning(0)                                      # the default evaluation path
    k = max(1, n // 5)                              # validation_data: 20 % of the sweeps
    xt, yt = x[:-k], [y[0][:-k], y[1][:-k]]
    xv, yv = x[-k:], [y[0][-k:], y[1][-k:]]
    steps = len(xt)                                 # one pass over the training sweeps per epoch
    for r in range(args.runs):
        per = {}
        for val in (False, True):
            kw = dict(validation_data=(xv, yv)) if val else {}
            model.fit(x=xt, y=yt, verbose=0, epochs=1, steps_per_epoch=steps, **kw)          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.fit(x=xt, y=yt, verbose=0, epochs=args.epochs, steps_per_epoch=steps, **kw)
            torch.cuda.synchronize()
            per[val] = (time.perf_counter() - t0) / args.epochs
        print(f"run {r}: fit epoch of {steps} steps (one pass) + {k} validation sweeps: without validation "
              f"{1e3 * per[False]:.1f} ms ({1e3 * per[False] / steps:.3f} ms/step), with {1e3 * per[True]:.1f} ms: "
              f"+{100 * (per[True] / per[False] - 1):.1f} % per epoch, {1e3 * (per[True] - per[False]) / k:.2f} ms per "
              f"validation sweep", flush=True)
