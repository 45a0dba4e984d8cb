"""Per-tensor gradient error at the full Lyft grid: GPU vs fp64 oracle next to the fp32 oracle vs fp64 oracle
(what tests/test_gpu_network.py bounds).  python tools/grad_conditioning.py [u20k|r200k|dense|empty] [mse|smoothl1_ce]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_network as T  # noqa: E402

cloud = sys.argv[1] if len(sys.argv) > 1 else "u20k"
loss = sys.argv[2] if len(sys.argv) > 2 else "mse"
# the clouds and seeds of the tests that bound these errors
cases = dict(u20k=lambda: (T.u20k(5), dict(seed=5)),
             r200k=lambda: (T.r200k(9), dict(seed=9, wseed=78)),
             dense=lambda: (T.dense_sweep(6), dict(seed=6)),
             empty=lambda: (np.zeros((0, 3), np.float32), dict(seed=10, wseed=78, exact_zero=T.EMPTY_ZERO)))
if cloud not in cases:
    sys.exit(f"unknown cloud {cloud!r}: one of {', '.join(cases)}")
pts, kw = cases[cloud]()
out, rows = T.full_grid_gradient_report(pts, loss, **kw)
print(f"{cloud} {loss}: loss {out['loss']:.8g} ref {out['loss_ref']:.8g} | regime {out['regime']}")
for n, sc, e, o in rows:
    flag = "" if out["l2"][n][0] <= max(T.FLAT, T.SPREAD * out["l2"][n][1]) else "  <-- beyond max(FLAT, SPREAD x own)"
    a, b, c = out["l2"][n]
    print(f"{n:20s} max|ref| {sc:8.2e} max-norm: gpu {e:8.2e} o32 {o:8.2e} r {e / max(o, 1e-30):5.2f} | "
          f"L2: gpu {a:8.2e} o32 {b:8.2e} r {a / max(b, 1e-30):5.2f} gpu-vs-o32 {c:8.2e}{flag}")
for n, (g, r64, r32) in out["zero"].items():
    print(f"{n:20s} exact gradient 0: max |gpu| {g:8.2e} max |fp64 oracle| {r64:8.2e} max |fp32 oracle| {r32:8.2e}")
ratios = [out["l2"][n][0] / out["l2"][n][1] for n, *_ in rows if out["l2"][n][1] > 1e-4]
print("worst gpu", max(r[2] for r in rows), "worst fp32 oracle", max(r[3] for r in rows))
print(f"L2 ratio gpu / fp32 oracle over {len(ratios)} tensors: median {np.median(ratios):.3f} worst {max(ratios):.3f}")
