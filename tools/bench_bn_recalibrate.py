"""Cost of a BatchNormalization recalibration (LisecNet.recalibrate_batchnorm) on the Lyft grid (GPU box only).

    python tools/bench_bn_recalibrate.py [--sweeps 100] [--windows 5]

One recalibration over --sweeps voxelised 20 000-point synthetic sweeps (bench.u20k_cloud) against the same number of
forward(training=False) calls -- what an evaluation of those sweeps costs, and code this feature does not touch -- and
of plain forward(training=True) calls, in one process, in alternating windows after a warm-up of each: a host clock
around work that ends in a device synchronise, the median of the windows, and their spread.  The recalibration is the
training-mode forwards plus one small launch per sweep, two fills, one clone and the closing launch."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import u20k_cloud
from lisec_amd import Constants, _lib
from lisec_amd import model_training as mt

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    _lib.require_gpu()
    grid = (Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, Constants.nx // 2, Constants.ny // 2,
            Constants.nz)
    distinct = [mt.VFE_preprocessing(u20k_cloud(i).astype(np.float32), *grid).sample for i in range(4)]
    samples = [distinct[i % len(distinct)] for i in range(args.sweeps)]
    model = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    net = model.net

    def forwards(training):
        for s in samples:
            net.forward(s, training=training)

    modes = (("recalibrate_batchnorm ('mean')", lambda: net.recalibrate_batchnorm(samples)),
             ("recalibrate_batchnorm ('pooled')", lambda: net.recalibrate_batchnorm(samples, statistics="pooled")),
             ("forward(training=False)", lambda: forwards(False)),
             ("forward(training=True)", lambda: forwards(True)))
    for _, call in modes:                                 # warm-up: code objects, lazy workspaces, the folds
        call()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in modes}
    for _ in range(args.windows):
        for name, call in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    for name, a in ms.items():
        print(f"{name}: median {np.median(a):.1f} ms for {args.sweeps} sweeps = {np.median(a) / args.sweeps:.3f} ms per sweep "
              f"(windows {min(a):.1f} .. {max(a):.1f} ms, {args.windows} windows)")
    base = float(np.median(ms["forward(training=False)"]))
    print(f"recalibrate_batchnorm ('mean') / forward(training=False) = "
          f"{float(np.median(ms[modes[0][0]])) / base:.3f}")
