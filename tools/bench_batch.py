"""Throughput of Model.fit(batch_size=B) in sweeps per second (GPU box only).

    python tools/bench_batch.py [--batches 1,2,4,8] [--rounds 5] [--sweeps 480] [--parent TREE] [--out profiles/batch_ab.txt]

Lyft grid, the 20 000-point synthetic sweep of bench.py, SGD-Nesterov, loss ['mse', 'mse'], recorded plans.  One
configuration is one child process (`--only B`): it makes the model, runs a warm-up fit -- which records the plans --
and times ONE fit of `--sweeps` sweeps (sweeps / B updates) between two device synchronisations.  The driver runs the
configurations round-robin, `--rounds` times, so that every configuration meets the same drift of the machine, and
reports the median and the spread (min .. max) of each configuration's rounds.  A child opens the GPU alone: the driver
itself never does.

--parent TREE: a checkout of a commit from before mini-batches, built.  Its batch-1 step joins the rotation as `parent
B=1`, run by this very file with the parent's package on the path (`--only 1` asks nothing of fit() that commit lacks).
The comparison that counts is against it: B = 1 here within the parent's own round-to-round spread, and B = 4 not
slower per sweep than the parent's batch-1 step by more than that spread."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tree, B, sweeps):
    """One timed fit in this process, on the package of `tree`; prints one JSON line."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from bench import synthetic_targets, u20k_cloud
    from lisec_amd import Constants, _lib
    from lisec_amd import model_training as mt
    _lib.require_gpu()
    n = 8
    samples = [mt.VFE_preprocessing(u20k_cloud(i).astype(np.float64), Constants.voxelx, Constants.voxely, Constants.voxelz,
                                    Constants.maxPoints, Constants.nx // 2, Constants.ny // 2, Constants.nz) for i in range(n)]
    tg = [synthetic_targets(i, Constants.nx // 2, Constants.ny // 2) for i in range(n)]
    y = [np.stack([t[0] for t in tg]).astype(np.float64), np.stack([t[1] for t in tg]).astype(np.float64)]
    m = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    m.fit(x=samples, y=y, batch_size=B, verbose=0, epochs=1, steps_per_epoch=max(1, 40 // B), shuffle=False)     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = m.fit(x=samples, y=y, batch_size=B, verbose=0, epochs=1, steps_per_epoch=sweeps // B, shuffle=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    step = m._captured[1]
    print(json.dumps(dict(B=B, sweeps=sweeps // B * B, seconds=dt, sweeps_per_s=sweeps // B * B / dt,
                          plan=type(step).__name__, launches=step.launches, loss=hist.history["loss"][-1],
                          iterations=m.net.iterations)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=480)
    ap.add_argument("--parent", default=None, help="a built checkout of a commit before mini-batches")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "batch_ab.txt"))
    ap.add_argument("--only", type=int, default=None, help="child mode: time this batch size in this process")
    ap.add_argument("--tree", default=HERE, help="child mode: the tree whose package runs")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    args = ap.parse_args()
    if args.only is not None:
        child(os.path.abspath(args.tree), args.only, args.sweeps)
        sys.exit(0)
    configs = [("parent B=1", os.path.abspath(args.parent), 1)] if args.parent else []
    configs += [(f"B={b}", HERE, int(b)) for b in args.batches.split(",")]
    runs = {name: [] for name, _, _ in configs}
    for r in range(args.rounds):
        for name, tree, B in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--only", str(B), "--tree", tree, "--sweeps", str(args.sweeps)]
            p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.limit)
            if p.returncode != 0:
                # a child that failed ends the measurement: nothing more is started on the GPU
                sys.exit(f"{name}, round {r}: exit status {p.returncode}\n{p.stderr[-3000:]}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r} {name}: {runs[name][-1]['sweeps_per_s']:.1f} sweeps/s", flush=True)
    lines = [f"Model.fit(batch_size=B), Lyft grid, u20k sweep, SGD-Nesterov, mse; {args.rounds} rounds, round-robin, one "
             f"process per run, {args.sweeps} sweeps timed per run after a 40-sweep warm-up fit", ""]
    med = {}
    for name, rs in runs.items():
        v = sorted(x["sweeps_per_s"] for x in rs)
        med[name] = v[len(v) // 2]
        lines.append(f"{name:11s} median {med[name]:7.1f} sweeps/s  (rounds {v[0]:.1f} .. {v[-1]:.1f}; spread "
                     f"{100 * (v[-1] - v[0]) / med[name]:.1f} %)  {1e3 / med[name]:.3f} ms per sweep, {rs[0]['plan']}, "
                     f"batch-1 plan of {rs[0]['launches']} operations, {rs[0]['iterations']} updates in all")
    base = "parent B=1" if args.parent else "B=1"
    lines.append("")
    for name in runs:
        if name != base:
            lines.append(f"{name} / {base} = {med[name] / med[base]:.4f} in sweeps/s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
