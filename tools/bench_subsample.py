"""The voxeliser with subsample='first' against subsample='random' (GPU box only).

    python tools/bench_subsample.py [--windows 7] [--iters 40] [--out profiles/subsample_ab.txt]

Three float32 clouds of 200 000 points on the Lyft grid:
  r200k  bench.py's r200k_cloud(0): 66 of its 84 229 voxels hold more than 35 points, the largest 53 -- nearly all the work
         is what both modes share, so a gap beyond the spread of 'first' would be a regression in the shared part
  near   the same generator with the radius pulled in, r = 2 + 0.25 u^2 (u uniform): 559 voxels, 503 of them above 35
         points, median 226, largest 670 -- the selection against the 35-pass loop of the deterministic kernel
  flat   `near` with z squeezed into 0.3 .. 0.7 m (two voxel layers): voxels of up to a few thousand points
Both modes write into preallocated samples (out=), in one process, in alternating windows of --iters calls timed with
device events; per mode the mean and the spread (min .. max) of the window means are reported, and the ratio of the means.
'random' sets the draw words in front of every call (one more launch: lisec_voxel_draw_set), 'random, words left alone' does
not: the difference between the two is that launch, the difference to 'first' the drawing k_features."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import r200k_cloud
from lisec_amd import Constants
from lisec_amd.voxelizer import Voxelizer


def pulled_in_cloud(seed, n=200000, reach=0.25, z=(-0.2, 2.2)):
    """r200k_cloud with the radius 2 + 68 u^2 pulled in to 2 + reach u^2, and z uniform in `z`."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(0, 2 * np.pi, n)
    r = 2.0 + reach * rng.uniform(0, 1, n) ** 2
    return np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(z[0], z[1], n)], 1).astype(np.float32)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    grid = (Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, Constants.nx // 2, Constants.ny // 2,
            Constants.nz)
    lines = []
    for name, cloud in (("r200k", r200k_cloud(0)), ("near", pulled_in_cloud(0)), ("flat", pulled_in_cloud(0, z=(0.3, 0.7)))):
        pts = torch.from_numpy(cloud).to(dev)
        vox = {m: Voxelizer(*grid, device=dev, subsample=m, seed=1) for m in ("first", "random")}
        out = {m: v(pts) for m, v in vox.items()}
        call = {"first": lambda: vox["first"](pts, out=out["first"]),
                "random": lambda: vox["random"](pts, out=out["random"], draw=(0, 0)),
                "random, words left alone": lambda: vox["random"](pts, out=out["random"])}
        host = {m: s.to_host() for m, s in out.items()}
        counts = host["first"]["counts"]
        same = all(np.array_equal(host["first"][k], host["random"][k]) for k in ("coords", "counts", "npts", "row_start"))
        for m in call:
            window_ms(call[m], args.iters)              # warm-up: code objects, workspaces
        ms = {m: [] for m in call}
        for _ in range(args.windows):
            for m in call:
                ms[m].append(window_ms(call[m], args.iters))
        head = (f"{name}: {len(counts)} voxels, {int((counts > Constants.maxPoints).sum())} above {Constants.maxPoints} points, "
                f"median {int(np.median(counts))}, largest {int(counts.max())}; voxel tables equal: {same}")
        lines.append(head)
        for m in call:
            a = np.array(ms[m]) * 1e3
            lines.append(f"  {m:24s} {a.mean():8.1f} us per call  (windows {a.min():.1f} .. {a.max():.1f}, {args.windows} x {args.iters} calls)")
        lines.append(f"  random / first = {np.mean(ms['random']) / np.mean(ms['first']):.3f}"
                     f" (words left alone: {np.mean(ms['random, words left alone']) / np.mean(ms['first']):.3f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
