"""Throughput of the reference-named surface: Model.fit(batch_size=1) on voxelised sweeps (GPU box only).

    python tools/bench_fit.py [--lr constant|cosine] [--cloud u20k|r200k] [--augment [--sample-to N] [--subsample random]]

--lr cosine trains with optimizers.schedules.CosineDecay (the update kernels read lr_t from the device descriptor)
instead of the reference's constant rate.  --augment adds, beside plain fit on the same sweeps, fit(x=AugmentedSweeps) with
about 50 boxes per sweep (augmentation, label maps and balancing made on the device at every step), fit on the same Sequence
with augment=False (the label kernels alone), and the stand-alone device times of the three entries.  --sample-to N adds
the same stream with ground-truth object sampling from a database of the sweeps' own objects (each sweep filled up towards
N boxes) and the device times of lisec_augment_sample / lisec_augment_paste.  --subsample random adds the augmented stream
with the voxeliser's seeded random per-voxel subsample against the same stream with 'first', in alternating windows of one
process (each window records its own step plan in a warm-up fit): the mean and the spread of the windows per mode."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import event_time_ms, r200k_cloud, synthetic_targets, u20k_cloud
from lisec_amd import Constants
from lisec_amd import model_training as mt

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lr", choices=("constant", "cosine"), default="constant")
    ap.add_argument("--cloud", choices=("u20k", "r200k"), default="u20k")
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--sample-to", type=int, default=0)
    ap.add_argument("--subsample", choices=("first", "random"), default="first")
    args = ap.parse_args()
    n = 4
    cloud = u20k_cloud if args.cloud == "u20k" else r200k_cloud
    pts = [cloud(i).astype(np.float64) for i in range(n)]
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
    print(f"Model.fit (lr {args.lr}, {args.cloud}): {steps / dt:.1f} steps/s ({1e3 * dt / steps:.2f} ms/step), "
          f"loss {hist.history['loss'][-1]:.4f}")
    if args.augment:
        from lisec_amd import augment, boxes, ops
        rng = np.random.default_rng(0)
        bxs = []
        for i in range(n):                      # ~50 cars on a jittered 12 m lattice inside +-45 m
            cells = rng.permutation(49)[:50 - i]
            bxs.append(np.array([[-42 + 12 * (c % 7) + rng.uniform(-2, 2), -42 + 12 * (c // 7) + rng.uniform(-2, 2), 1.0,
                                  rng.uniform(3.8, 4.8), rng.uniform(1.7, 2.0), 1.6, rng.uniform(-3.1, 3.1)] for c in cells]))
        runs = [("augmented", {}), ("labels only (augment=False)", dict(augment=False))]
        if args.sample_to > 0:
            # objects need points: every box gets 40 of its own before the database is cut out
            pts = [np.concatenate([p[:, :3], np.concatenate([b[None, :3] + rng.uniform(-0.4, 0.4, (40, 3)) for b in bx])])
                   for p, bx in zip(pts, bxs)]
            db = augment.ObjectDatabase(pts, bxs)
            runs.append((f"sampled to {args.sample_to} boxes from {len(db)} objects", dict(database=db, sample_to=args.sample_to)))
        for label, kw in runs:
            seq = augment.AugmentedSweeps(pts, bxs, seed=1, **kw)
            model.fit(x=seq, batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = model.fit(x=seq, batch_size=1, verbose=0, epochs=1, steps_per_epoch=steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"Model.fit on AugmentedSweeps, {label}: {steps / dt:.1f} steps/s ({1e3 * dt / steps:.2f} ms/step), "
                  f"loss {hist.history['loss'][-1]:.4f}")
        if args.subsample == "random":
            ms = {"first": [], "random": []}
            label, kw = runs[2] if len(runs) > 2 else runs[0]           # with object sampling when it was asked for
            for _ in range(4):
                for mode in ms:
                    seq = augment.AugmentedSweeps(pts, bxs, seed=1, subsample=mode, **kw)
                    model.fit(x=seq, batch_size=1, verbose=0, epochs=1, steps_per_epoch=20)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.fit(x=seq, batch_size=1, verbose=0, epochs=1, steps_per_epoch=100)
                    torch.cuda.synchronize()
                    ms[mode].append(1e3 * (time.perf_counter() - t0) / 100)
            for mode, a in ms.items():
                print(f"Model.fit on AugmentedSweeps ({label}), subsample={mode}: {np.mean(a):.3f} ms/step "
                      f"(windows {min(a):.3f} .. {max(a):.3f}, 4 x 100 steps)")
            print(f"random / first = {np.mean(ms['random']) / np.mean(ms['first']):.4f}")
        seq = augment.AugmentedSweeps(pts, bxs, seed=1)
        src, bx = seq.points[0], seq.boxes[0]
        out = torch.empty((src.shape[0], 3), dtype=src.dtype, device=src.device)
        tr, glob, bx_out, _, _ = ops.augment_draw(bx, seq.params, 1, 0, 0)
        maps = boxes.rpnTargets(bx_out)
        seq.stage(0, out, *maps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            seq.stage(0, out, *maps)
        host = time.perf_counter() - t0          # the enqueue alone: read before the device is waited for
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        print(f"one staged item (draw + apply + targets): host enqueue {1e3 * host / 200:.3f} ms, "
              f"device-bound {1e3 * total / 200:.3f} ms")
        print(f"lisec_augment_draw  ({len(bx)} boxes): {1e3 * event_time_ms(lambda: ops.augment_draw(bx, seq.params, 1, 0, 0), 50):.1f} us")
        print(f"lisec_augment_apply ({src.shape[0]} points): "
              f"{1e3 * event_time_ms(lambda: ops.augment_apply(src, bx, tr, glob, out, augment.PAD_LIMIT), 50):.1f} us")
        for bal in (False, True):
            print(f"lisec_rpn_targets   (balance={bal}): {1e3 * event_time_ms(lambda: boxes.rpnTargets(bx_out, balance=bal, out=maps), 50):.1f} us")
        if args.sample_to > 0:
            K = augment._sample_count(len(bx), args.sample_to)
            smp = lambda: ops.augment_sample(bx, db.boxes, db.offsets, K, 1, 0, 0)
            index, n_boxes, boxes_all, point_offset, _ = smp()
            dbp = db.points_as(src.dtype)
            pasted = torch.empty((src.shape[0] + db.bound(K), 3), dtype=src.dtype, device=src.device)
            paste = lambda: ops.augment_paste(src, dbp, db.offsets, index, point_offset, boxes_all, n_boxes, pasted,
                                              augment.PAD_LIMIT)
            print(f"lisec_augment_sample ({len(bx)} boxes, {K} candidates, {int(n_boxes.item()) - len(bx)} accepted): "
                  f"{1e3 * event_time_ms(smp, 50):.1f} us")
            print(f"lisec_augment_paste  ({pasted.shape[0]} rows): {1e3 * event_time_ms(paste, 50):.1f} us")
