"""Forward-only (inference BatchNormalization) latency of voxelise + VFE + middle + RPN on one sweep (GPU box only).

--policy float32 | mixed_bfloat16 | both (default: both nets in one process, timed alternately, so that the two columns
saw the same machine).  Prints the whole voxelise + forward time per sweep (median and spread of --rounds windows) and the
time of each of the eighteen contractions the 'mixed_bfloat16' policy moves to the bf16 kernel, under each policy: the
layer's own launch repeated back to back on the activations of a real forward, between two device events."""
import argparse
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import r200k_cloud, u20k_cloud
from lisec_amd import Constants
from lisec_amd.network import LisecNet
from lisec_amd.voxelizer import Voxelizer

COMPUTE = {"float32": "float32", "mixed_bfloat16": "bfloat16"}


def sweep_ms(net, vox, pts, K):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        net.forward(vox(pts), training=False)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / K


def layer_us(net, reps):
    """{layer: us per launch} of the mid2 / mid3 Conv3Ds and the RPN Conv2Ds, on the activations the last forward left."""
    out = {}
    a = net.act
    for L in net.layers:
        if L["kind"] == "deconv" or L["src"] == "grid":
            continue
        c = L["conv"]
        dst = a[L["name"] + ".y"] if L["kind"] == "mid" else a[L["dst"]]
        for _ in range(3):
            net._run_conv(c, a[L["src"]], dst, False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            net._run_conv(c, a[L["src"]], dst, False)
        e1.record()
        torch.cuda.synchronize()
        out[c.name] = 1e3 * e0.elapsed_time(e1) / reps
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", choices=["float32", "mixed_bfloat16", "both"], default="both")
    ap.add_argument("--cloud", choices=["u20k", "r200k"], default="u20k")
    ap.add_argument("--steps", type=int, default=200, help="sweeps per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per policy (alternating)")
    ap.add_argument("--layer-reps", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda")
    policies = ["float32", "mixed_bfloat16"] if args.policy == "both" else [args.policy]
    nets = {p: LisecNet(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints, device=dev, compute_dtype=COMPUTE[p])
            for p in policies}
    vox = Voxelizer(Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, Constants.nx // 2,
                    Constants.ny // 2, Constants.nz, device=dev)
    pts = torch.from_numpy((u20k_cloud if args.cloud == "u20k" else r200k_cloud)(0)).to(dev)
    if len(nets) == 2:          # the same variables under both policies
        nets["mixed_bfloat16"].params.theta.copy_(nets["float32"].params.theta)
        nets["mixed_bfloat16"].params.state.copy_(nets["float32"].params.state)
        nets["mixed_bfloat16"].params.touch()
    for net in nets.values():
        for _ in range(10):
            net.forward(vox(pts), training=False)
    times = {p: [] for p in policies}
    for _ in range(args.rounds):
        for p in policies:
            times[p].append(sweep_ms(nets[p], vox, pts, args.steps))
    print(f"cloud {args.cloud} ({pts.shape[0]} points), {args.rounds} windows of {args.steps} sweeps, alternating")
    for p in policies:
        t = times[p]
        med = statistics.median(t)
        print(f"{p:>15}: voxelise + forward (inference BN) {med:.3f} ms per sweep (min {min(t):.3f}, max {max(t):.3f}) "
              f"= {1e3 / med:.0f} sweeps/s")
    if len(policies) == 2:
        print(f"whole forward, float32 / mixed_bfloat16: {statistics.median(times['float32']) / statistics.median(times['mixed_bfloat16']):.2f}x")
    per = {}
    for p in policies:
        nets[p].forward(vox(pts), training=False)
        a, b = layer_us(nets[p], args.layer_reps), layer_us(nets[p], args.layer_reps)
        per[p] = {k: (min(a[k], b[k]), max(a[k], b[k])) for k in a}
    print("per layer, us per launch (two runs of %d back-to-back launches: low - high)" % args.layer_reps)
    for name in per[policies[0]]:
        row = "  ".join(f"{p} {per[p][name][0]:7.1f} - {per[p][name][1]:7.1f}" for p in policies)
        gain = f"  {per['float32'][name][0] / per['mixed_bfloat16'][name][1]:.2f}x .. " \
               f"{per['float32'][name][1] / per['mixed_bfloat16'][name][0]:.2f}x" if len(policies) == 2 else ""
        print(f"{name:>12}: {row}{gain}")
    for p in policies:
        print(f"{p:>15}: the eighteen layers together {sum(v[0] for v in per[p].values()):.0f} us")
