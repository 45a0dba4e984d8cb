"""Timing of the two "next" rows around the hot path: label generation (serialize_data.py:194-338) and RPN decode +
rotated NMS (rpnToRegion.py:18-164) on the GPU, with the CPU oracle (the reference's algorithm with the shapely polygon
clipping restated) beside it on a reduced case, and the many-box path (boxes.detect) beside rpnToRegion on the same maps with a
per-kernel breakdown.  GPU box only.  `--detect` prints the decode + NMS rows alone."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lisec_amd import boxes
from oracle import boxes_ref as B


def scene(rng, n):
    d = np.zeros((n, 7))
    d[:, 0] = rng.uniform(-48, 48, n); d[:, 1] = rng.uniform(-48, 48, n); d[:, 2] = rng.uniform(0.5, 1.5, n)
    d[:, 3] = rng.uniform(3.5, 5.2, n); d[:, 4] = rng.uniform(6.5, 9.0, n); d[:, 5] = rng.uniform(1.3, 1.8, n)
    d[:, 6] = rng.choice([0.0, np.pi / 2, 0.1, -0.2, 1.4], n)
    return d


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernel_breakdown(fn, reps=20):
    """Mean device time per call of each k_detect_* kernel (microseconds), from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.key_averages():
        if "k_detect_" in e.key:
            name = e.key[e.key.index("k_detect_"):].split("(")[0]
            rows[name] = rows.get(name, 0.0) + e.device_time_total / reps
    if len(rows) != 4:
        raise RuntimeError(f"the profiler recorded {sorted(rows)} instead of the four k_detect_* kernels")
    return rows


def detect_lines(cls, reg):
    """boxes.detect beside rpnToRegion on the same 40 000-candidate maps, both timed by `timed` in this run."""
    base = {}
    for mb in (20, 100):
        base[mb] = timed(lambda: boxes.rpnToRegion(cls, reg, maxBoxes=mb), 5)
        print(f"rpnToRegion  40 000 candidates, maxBoxes {mb:3d}   GPU {base[mb] * 1e3:8.2f} ms")
    for top_n, mb in ((1000, 20), (1000, 100), (1000, 300), (4096, 300)):
        t = timed(lambda: boxes.detect(cls, reg, pre_nms_top_n=top_n, max_boxes=mb), 20)
        beside = f"   ({base[mb] / t:5.1f} x rpnToRegion maxBoxes {mb})" if mb in base else ""
        print(f"detect       40 000 candidates, top-N {top_n:4d}, max_boxes {mb:3d}   GPU {t * 1e3:8.3f} ms{beside}")
    d_cls, d_reg = torch.from_numpy(cls[0]).cuda(), torch.from_numpy(reg[0]).cuda()
    for top_n, mb in ((1000, 100), (4096, 300)):
        call = lambda: boxes.detect(d_cls, d_reg, pre_nms_top_n=top_n, max_boxes=mb, as_device=True)
        t = timed(call, 50)
        rows = kernel_breakdown(call)
        print(f"detect       device maps, as_device, top-N {top_n:4d}, max_boxes {mb:3d}   GPU {t * 1e3:8.3f} ms per call;  kernels: "
              + ", ".join(f"{k} {v:.1f} us" for k, v in sorted(rows.items())) + f", sum {sum(rows.values()):.1f} us")


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    if "--detect" in sys.argv:                                 # the decode + NMS rows alone, on the maps the full run uses
        for n in (10, 40, 10):
            scene(rng, n)
        cls = rng.uniform(0, 1, (1, 100, 200, 2)).astype(np.float32)
        reg = rng.normal(0, 0.1, (1, 100, 200, 14)).astype(np.float32)
        detect_lines(cls, reg)
        sys.exit(0)
    for n in (10, 40):
        data = scene(rng, n)
        t = timed(lambda: boxes.preprocessLabels(data, seed=1), 5)
        print(f"preprocessLabels  {n:3d} boxes x 40 000 anchors   GPU {t * 1e3:8.2f} ms per sample (incl. host copies)")
    data = scene(rng, 10)
    t0 = time.perf_counter()
    B.preprocess_labels(data, seed=1)
    print(f"preprocess_labels  10 boxes   CPU oracle (python, circumradius pre-test)  {time.perf_counter() - t0:8.2f} s")
    cls = rng.uniform(0, 1, (1, 100, 200, 2)).astype(np.float32)
    reg = rng.normal(0, 0.1, (1, 100, 200, 14)).astype(np.float32)
    detect_lines(cls, reg)
    t0 = time.perf_counter()
    bi = B.decode_boxes(reg[0].astype(np.float64))
    pi = np.concatenate([cls[0, :, :, a].reshape(-1) for a in range(2)]).astype(np.float64)
    B.nms(bi[:4000], pi[:4000], maxBoxes=20)
    print(f"nms   4 000 candidates (a tenth), maxBoxes 20   CPU oracle  {time.perf_counter() - t0:8.2f} s")
    # scoring (rpnToRegion.py:202-255): 1000 samples of 20 predictions x 40 labels in one launch, and one sample alone
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
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
    scenes = [clustered_scene(rng, 20, 40, 10) for _ in range(1000)]
    dev_p = [torch.from_numpy(p).cuda() for p, _ in scenes]
    dev_l = [torch.from_numpy(l).cuda() for _, l in scenes]
    t = median7(lambda: boxes.union_overlap(dev_p, dev_l))
    print(f"union_overlap  1000 samples x (20 pred, 40 label), one launch   GPU {t * 1e3:8.2f} ms  (median of 7, incl. packing + copy back)")
    t = median7(lambda: boxes.union_overlap(dev_p[:1], dev_l[:1]))
    print(f"union_overlap  1 sample (20 pred, 40 label)                     GPU {t * 1e3:8.3f} ms  (median of 7)")
    # detection average precision (boxes.average_precision): the same 1000 samples with scores, and one sample alone
    dev_s = [torch.from_numpy(rng.uniform(0.01, 0.99, 20)).cuda() for _ in scenes]
    t = median7(lambda: boxes.average_precision(dev_p, dev_s, dev_l))
    print(f"average_precision  1000 samples x (20 pred, 40 label), 10 thresholds   GPU {t * 1e3:8.2f} ms  (median of 7, incl. packing + copy back)")
    t = median7(lambda: boxes.average_precision(dev_p[:1], dev_s[:1], dev_l[:1]))
    print(f"average_precision  1 sample (20 pred, 40 label), 10 thresholds         GPU {t * 1e3:8.3f} ms  (median of 7)")
