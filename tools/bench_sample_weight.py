"""What a per-cell weight map costs the loss pass: the weighted head-loss and detection-loss entries against their
unweighted twins on a Lyft-grid head (M = 20 000 cells), timed back to back on one stream with device events, as
tools/phase_times.py times the step's phases.  Prints one line per entry: the median and range of the per-call time.

    python tools/bench_sample_weight.py [--calls 200] [--rounds 7]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lisec_amd import _lib, ops  # noqa: E402
from lisec_amd import losses as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cells", type=int, default=20000)
    args = ap.parse_args()
    dev = _lib.require_gpu()
    M = args.cells
    rng = np.random.default_rng(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    head, y_reg = up(rng.normal(0, 1.2, (M, 16))), up(rng.normal(0, 1, (M, 14)) + 1.0)
    y_cls = up(rng.choice(np.float32([0, 1, 2]), (M, 2), p=[0.49, 0.5, 0.01]))
    w = up(rng.uniform(0, 3, M))
    dhead = torch.zeros((M, 16), dtype=torch.float32, device=dev)
    loss_out = torch.zeros(3, dtype=torch.float32, device=dev)
    met = torch.zeros(8, dtype=torch.float32, device=dev)
    pairs = torch.zeros(16, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    spec = K.compile_weighted_loss([K.BinaryCrossentropy(from_logits=True), K.Huber(delta=0.5)], loss_weights=[2.0, 0.5],
                          metrics=["mae"], weighted_metrics=["mse"])[0]
    det = K.compile_loss("voxelnet")[0]
    iou = K.compile_loss("voxelnet_iou")[0]
    hd, dd, idesc = spec.descriptor(), det.descriptor(), iou.descriptor()
    sw_head = ops.sample_weights(w, w, M, weighted_metrics=spec.weighted)
    sw_det = ops.sample_weights(w, w, M)
    entries = [
        ("head loss", lambda: ops.head_loss(hd, head, y_cls, y_reg, M, dhead, loss_out, met)),
        ("head loss, weighted", lambda: ops.head_loss_weighted(hd, sw_head, head, y_cls, y_reg, M, dhead, loss_out, pairs)),
        ("detection loss", lambda: ops.detection_loss(dd, head, y_cls, y_reg, M, dhead, loss_out, counts)),
        ("detection loss, weighted", lambda: ops.detection_loss_weighted(dd, sw_det, head, y_cls, y_reg, M, dhead, loss_out,
                                                                        counts)),
        ("detection IoU loss", lambda: ops.detection_iou_loss(idesc, head, y_cls, y_reg, M, dhead, loss_out, counts)),
        ("detection IoU loss, weighted", lambda: ops.detection_loss_weighted(idesc, sw_det, head, y_cls, y_reg, M, dhead,
                                                                            loss_out, counts)),
    ]
    times = {name: [] for name, _ in entries}
    for name, call in entries:                      # warm-up
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    for _ in range(args.rounds):                    # the entries alternate, round by round
        for name, call in entries:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                call()
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / args.calls)
    for name, _ in entries:
        t = np.array(times[name])
        print(f"{name:30s} {np.median(t):7.2f} us per call  ({t.min():.2f} - {t.max():.2f}, {args.rounds} rounds of "
              f"{args.calls} calls, M = {M})")


if __name__ == "__main__":
    main()
