"""Throughput of the reference-named surface: Model.fit(batch_size=1) on voxelised sweeps (GPU box only).

    python tools/bench_fit.py [--lr constant|cosine]

--lr cosine trains with optimizers.schedules.CosineDecay (the update kernels read lr_t from the device descriptor)
instead of the reference's constant rate."""
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

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lr", choices=("constant", "cosine"), default="constant")
    args = ap.parse_args()
    n = 4
    pts = [u20k_cloud(i).astype(np.float64) for i in range(n)]
    samples = [mt.VFE_preprocessing(p, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                                    Constants.nx // 2, Constants.ny // 2, Constants.nz) for p in pts]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    ycls = np.stack([t[0] for t in tg]).astype(np.float64)
    yreg = np.stack([t[1] for t in tg]).astype(np.float64)
    model = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    lr = 0.01 if args.lr == "constant" else mt.optimizers.schedules.CosineDecay(0.01, decay_steps=1000, alpha=0.01)
    model.compile(optimizer=mt.optimizers.SGD(lr=lr, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    model.fit(x=samples, y=[ycls, yreg], batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
    torch.cuda.synchronize()
    steps = 200
    t0 = time.perf_counter()
    hist = model.fit(x=samples, y=[ycls, yreg], batch_size=1, verbose=0, epochs=1, steps_per_epoch=steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"Model.fit (lr {args.lr}): {steps / dt:.1f} steps/s ({1e3 * dt / steps:.2f} ms/step), loss {hist.history['loss'][-1]:.4f}")
