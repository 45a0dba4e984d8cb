"""Times of the gradient-clipping passes (csrc/grad_clip.hip), after tools/bench_lamb.py.  GPU box only.

1. Each entry alone on the network's 6 491 024 variables with its real chunk table: device time between two events
   around REPS back-to-back calls, median of 7 after a warm-up.  Every entry is timed twice: with a threshold far below
   the gradient's norms (every chunk is scaled: 4 bytes per element for the sum of squares and 8 for the apply pass) and
   with one far above (every scale is exactly 1: the apply pass reads a scale per chunk and skips the chunk, so only the
   4 bytes per element of the sum of squares remain).  clipvalue moves 8 bytes per element either way.  The finish entry
   of the global norm (the one-workgroup sum and the apply pass) is also timed alone in both regimes: the same two
   launches, so their difference is the traffic the apply pass skips.
2. ms per step of the replayed fit() step (PipelinedStep, the plan Model.fit replays) on the benchmark's sweep with Adam:
   without clipping -- the launches of the commit before clipping, measured in this same run --, with clipnorm and with
   global_clipnorm, which gives up the early update of the RPN tail."""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import synthetic_targets, u20k_cloud
from bench_lamb import REPS, event_time
from lisec_amd import Constants, _lib, ops
from lisec_amd import model_training as mt
from lisec_amd.network import LisecNet, PipelinedStep
from lisec_amd.params import ParamStore
from lisec_amd.voxelizer import Voxelizer

STEPS, WARMUP, ROUNDS = 100, 10, 5


def entries(dev):
    store = ParamStore(torch.device("cpu"))
    n = store.n_theta
    table = ops.lamb_table(*ops.clip_chunks(store), dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    source = torch.randn(n, device=dev, generator=gen)
    grad = source.clone()
    scales, norms = torch.ones(table.n_vars, device=dev), torch.zeros(table.n_vars, device=dev)
    ws = ops.clip_workspace(table.n_chunks, dev)
    bufs = dict(table=table, scales=scales, norms=norms, workspace=ws)
    mb = n * 4 / 1e6
    print(f"variables {n}, chunks {table.n_chunks}, trainable variables {table.n_vars}, {REPS} calls per timing, median of 7")

    def timed(name, fn, floats):
        med, lo, hi = event_time(fn)
        print(f"{name:34s} {med * 1e6:8.2f} us  (min {lo * 1e6:.2f}, max {hi * 1e6:.2f});  {floats} floats per element = "
              f"{floats * mb:.0f} MB -> {floats * mb / 1e6 / med:.2f} TB/s")
        return med

    # "clips": a threshold that STAYS below every norm however often the pass has run.  Clipping to c leaves a norm of
    # c, so a repeated call with the same c would find nothing to do; the gradient is restored in front of every call
    # instead, and the restoring copy (8 bytes per element) is timed alone and subtracted
    t_copy = timed("copy (restores the gradient)", lambda: grad.copy_(source), 2)

    def restored(fn):
        def call():
            grad.copy_(source)
            fn()
        return call

    for name, fn, floats in (
            ("clipvalue, clips", lambda: ops.grad_clip_value(grad, 0.5, table=table), 2),
            ("clipnorm, clips", lambda: ops.grad_clip_norm(grad, 1e-3, **bufs), 3),
            ("global_clipnorm, clips", lambda: ops.grad_clip_global_norm(grad, 1e-3, **bufs), 3)):
        med, lo, hi = event_time(restored(fn))
        t = med - t_copy
        print(f"{name:34s} {t * 1e6:8.2f} us  (with the copy: {med * 1e6:.2f}, min {lo * 1e6:.2f}, max {hi * 1e6:.2f});  "
              f"{floats} floats per element = {floats * mb:.0f} MB -> {floats * mb / 1e6 / t:.2f} TB/s")
    grad.copy_(source)
    timed("clipvalue, nothing above", lambda: ops.grad_clip_value(grad, 1e6, table=table), 2)
    timed("clipnorm, every scale 1", lambda: ops.grad_clip_norm(grad, 1e6, **bufs), 1)
    timed("global_clipnorm, scale 1", lambda: ops.grad_clip_global_norm(grad, 1e6, **bufs), 1)
    torch.cuda.synchronize()
    assert torch.equal(grad, source) and bool((scales == 1).all())          # scale 1: the gradient kept its bits
    timed("global_clipnorm, partials alone", lambda: ops.grad_clip_global_norm_partials(grad, table=table, workspace=ws), 1)
    # the finish entry alone is the one-workgroup sum and the apply pass: the same two launches in both lines, over the
    # partials left above, so the difference is the apply pass's traffic.  (With a small threshold every call scales by
    # the same factor again -- the partials are not retaken -- and the values shrink to zero; the traffic does not.)
    finish = lambda c: ops.grad_clip_global_norm_finish(grad, c, **bufs)
    timed("finish alone, scale 1 (skips)", lambda: finish(1e6), 0)
    timed("finish alone, scales every chunk", lambda: finish(1e-3), 2)
    grad.copy_(source)


def fit_step(dev, kind, value):
    """ms per replayed step: median, min and max of ROUNDS timings of STEPS steps."""
    O = mt.optimizers
    opt = O.clip_gradients(O.Adam(learning_rate=1e-4), **({kind: value} if kind else {}))
    net = LisecNet(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints, device=dev)
    vox = Voxelizer(Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, Constants.nx // 2,
                    Constants.ny // 2, Constants.nz, device=dev)
    cloud = u20k_cloud(0)
    pts = torch.from_numpy(cloud).to(dev)
    ycls, yreg = (torch.from_numpy(a).to(dev) for a in synthetic_targets(0, net.Ho, net.Wo))
    step = PipelinedStep(net, vox, len(cloud), dtype=pts.dtype, loss="mse", opt=opt.spec())
    step.prime(pts, ycls, yreg)
    step.stage_next(pts, ycls, yreg)
    step.step()
    step.stage_next(pts, ycls, yreg)
    for _ in range(WARMUP):
        step.step()
    times = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / STEPS * 1e3)
    norms = net.gradient_norms() if kind else {}
    launches = step.launches
    step.close()
    return statistics.median(times), min(times), max(times), launches, norms


if __name__ == "__main__":
    dev = _lib.require_gpu()
    entries(dev)
    print(f"replayed fit() step with Adam, {STEPS} steps per timing, median of {ROUNDS}:")
    base = None
    for kind, value in ((None, None), ("clipnorm", 1.0), ("global_clipnorm", 10.0), (None, None)):
        med, lo, hi, launches, norms = fit_step(dev, kind, value)
        base = med if base is None else base
        seen = f"largest norm of the last step {max(norms.values()):.4g}" if norms else "the step of the commit before"
        print(f"  {str(kind):16s} {'' if value is None else value!s:5s} {med:.4f} ms  (min {lo:.4f}, max {hi:.4f})  "
              f"{med / base:.4f} of the first line;  {launches} launches;  {seen}")
