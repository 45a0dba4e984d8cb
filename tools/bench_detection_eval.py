"""Timing of boxes.evaluate_detections beside boxes.average_precision on the same inputs: 1000 samples of 20 predictions x 40
labels with the ten default thresholds, and one such sample alone (the sizes DESIGN section 7 names).  Median of 7, host
packing, the sort and the copy back included.  GPU box only.  The new entry computes strictly more (ignored overlaps, four
geometry words per prediction, a second envelope, the F1 walk), so it is expected to be somewhat slower; there is no target."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from lisec_amd import boxes
from union_overlap_ref import clustered_scene


def median7(fn):
    fn()
    ts = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[3]


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    scenes = [clustered_scene(rng, 20, 40, 10) for _ in range(1000)]
    dev_p = [torch.from_numpy(p).cuda() for p, _ in scenes]
    dev_l = [torch.from_numpy(l).cuda() for _, l in scenes]
    dev_s = [torch.from_numpy(rng.uniform(0.01, 0.99, 20)).cuda() for _ in scenes]
    flags = [rng.uniform(size=40) < 0.3 for _ in scenes]
    for n, what in ((1000, "1000 samples x (20 pred, 40 label)"), (1, "1 sample (20 pred, 40 label)      ")):
        p, s, l, f = dev_p[:n], dev_s[:n], dev_l[:n], flags[:n]
        t_ap = median7(lambda: boxes.average_precision(p, s, l))
        t_ev = median7(lambda: boxes.evaluate_detections(p, s, l))
        t_fl = median7(lambda: boxes.evaluate_detections(p, s, l, label_ignore=f))
        print(f"{what}, 10 thresholds   average_precision {t_ap * 1e3:8.3f} ms   evaluate_detections {t_ev * 1e3:8.3f} ms"
              f"   with 30% ignored labels {t_fl * 1e3:8.3f} ms   (median of 7, incl. packing, sort and copy back)")
