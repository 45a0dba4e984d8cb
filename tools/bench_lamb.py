"""Time of one LAMB update (csrc/lamb.hip: moments, ratios, apply) on the network's 6 491 024 variables with its real
chunk table, beside the Adam update (csrc/optim.hip) timed in the same process: device time between two events around
REPS back-to-back updates, median of 7 after a warm-up.  By HBM traffic LAMB moves 10 floats per variable element
against Adam's 7.  GPU box only."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lisec_amd import _lib, ops
from lisec_amd.params import ParamStore

REPS = 20


def event_time(fn, reps=REPS, rounds=7, warmup=3):
    """Median over `rounds` of the device time of `reps` calls of fn, per call, in seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return statistics.median(times), min(times), max(times)


if __name__ == "__main__":
    dev = _lib.require_gpu()
    store = ParamStore(torch.device("cpu"))
    n = store.n_theta
    chunks, variables = ops.lamb_chunks(store, ("bias", "gamma", "beta"))
    table = ops.lamb_table(chunks, variables, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    theta, grad = (torch.randn(n, device=dev, generator=gen) for _ in range(2))
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ratios = torch.ones(table.n_vars, device=dev)
    ws = ops.lamb_workspace(table.n_chunks, table.n_vars, dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)

    def lamb():
        ops.lamb_step_dev(theta, grad, m, v, 1e-3, 0.0, 0.01, 0.9, 0.999, 1e-6, state, table=table, ratios=ratios,
                          workspace=ws)

    def adam():
        ops.adam_step_dev(theta, grad, m, v, None, 1e-3, 0.0, 0.9, 0.999, 1e-7, state)

    t_adam = event_time(adam)
    t_lamb = event_time(lamb)
    mb = n * 4 / 1e6
    print(f"variables {n}, chunks {table.n_chunks}, trainable variables {table.n_vars}, {REPS} updates per timing, median of 7")
    for name, (med, lo, hi), floats in (("adam", t_adam, 7), ("lamb", t_lamb, 10)):
        print(f"{name:5s} update  {med * 1e6:8.2f} us  (min {lo * 1e6:.2f}, max {hi * 1e6:.2f});  {floats} floats per "
              f"element = {floats * mb:.0f} MB -> {floats * mb / 1e6 / med:.2f} TB/s")
    print(f"lamb / adam  {t_lamb[0] / t_adam[0]:.3f}   (10/7 = {10 / 7:.3f} by bytes, plus two more launches)")
