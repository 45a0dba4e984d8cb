"""Logs the sequence of library calls of one training step: every lisec_* entry in the order it is issued, the stream it
goes to (main, side or other) and, for the event edges, which event (numbered by first appearance).  No address enters
the log, so the logs of two processes -- two versions of the schedule -- can be compared as text; it is also what a
step timeline is read against.  Measurement aid.

    python tools/backward_order.py --grid lyft --compose-head 1 --hook early_update --out step.log

--hook none traces forward(training=True) + backward(); early_update traces train_step() with an optimizer, so that
the rpn_grads_ready hook fires.  --plan recorded|pipelined traces the recording steps of a RecordedStep / PipelinedStep
instead (PipelinedStep: the next sweep's voxelisation rides as the side_filler) and logs the plan's size."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench import synthetic_targets, u20k_cloud
from lisec_amd import Constants, _lib
from lisec_amd.network import LisecNet, OptimizerSpec, PipelinedStep, RecordedStep
from lisec_amd.voxelizer import Voxelizer

ap = argparse.ArgumentParser()
ap.add_argument("--grid", choices=["small", "lyft"], default="lyft")
ap.add_argument("--compose-head", type=int, choices=[0, 1], default=1)
ap.add_argument("--hook", choices=["none", "early_update"], default="none")
ap.add_argument("--plan", choices=["none", "recorded", "pipelined"], default="none")
ap.add_argument("--out", default=None, help="file for the log (default: standard output)")
args = ap.parse_args()


class LoggedLibrary:
    """Stands in for the loaded library (_lib._lib): every lisec_* entry called through it is logged while `lines` is a
    list, or from the first call of the entry `start_at` on.  The stream of an entry is its last argument where that is a
    void* and the entry returns a status."""

    NO_STREAM = ("lisec_step_plan_", "lisec_comm_", "lisec_debug_")

    def __init__(self, real):
        self.real, self.lines, self.start_at, self.streams, self.events = real, None, None, {}, {}

    @staticmethod
    def handle(v):
        return getattr(v, "value", v) or 0

    def role(self, v):
        return self.streams.get(self.handle(v), "other")

    def event(self, v):
        return "ev%d" % self.events.setdefault(self.handle(v), len(self.events))

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("lisec_"):
            return fn

        def call(*a):
            if self.lines is None and name == self.start_at:
                self.lines = []
            if self.lines is not None:
                if name == "lisec_event_record":
                    what = f"{self.event(a[0])} on {self.role(a[1])}"
                elif name == "lisec_stream_wait_event":
                    what = f"{self.event(a[1])} by {self.role(a[0])}"
                elif (fn.restype is ctypes.c_int and fn.argtypes and fn.argtypes[-1] is ctypes.c_void_p
                      and not name.startswith(self.NO_STREAM)):
                    what = self.role(a[-1])
                else:
                    what = "-"
                self.lines.append(f"{name} {what}")
            return fn(*a)
        return call


lib = _lib._lib = LoggedLibrary(_lib.load())        # in place before anything keeps a reference to the library
dev = torch.device("cuda")
if args.grid == "lyft":
    net = LisecNet(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints, device=dev,
                   compose_head=bool(args.compose_head))
    vox = Voxelizer(Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints, Constants.nx // 2,
                    Constants.ny // 2, Constants.nz, device=dev)
    cloud = u20k_cloud(0)
else:
    net = LisecNet(16, 32, 8, 35, device=dev, compose_head=bool(args.compose_head))
    vox = Voxelizer(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)
    rng = np.random.default_rng(1)
    cloud = np.stack([rng.uniform(-4.2, 4.2, 3000), rng.uniform(-4.2, 4.2, 3000), rng.uniform(0.0, 2.1, 3000)], 1)
    cloud = cloud.astype(np.float32)
pts = torch.from_numpy(cloud).to(dev)
yc, yr = (torch.from_numpy(t).to(dev) for t in synthetic_targets(0, net.Ho, net.Wo))
lib.streams = {torch.cuda.current_stream().cuda_stream: "main", net.side.cuda_stream: "side"}

if args.plan == "none":
    for _ in range(2):                               # lazy workspaces, descriptor tables, events, the pending repack
        net.train_step(vox(pts), yc, yr)
    torch.cuda.synchronize()
    sample = vox(pts)
    lib.lines = []
    if args.hook == "early_update":
        net.train_step(sample, yc, yr, opt=OptimizerSpec())
    else:
        net.forward(sample, training=True)
        lib.lines.append("---- backward ----")
        net.backward(yc, yr)
    lines, lib.lines = lib.lines, None
else:
    # the constructor warms up eagerly and then records one step per buffer set: logged from the first recording on
    lib.start_at = "lisec_step_plan_begin"
    step = (PipelinedStep if args.plan == "pipelined" else RecordedStep)(net, vox, len(cloud), dtype=pts.dtype)
    lines, lib.lines = lib.lines, None
    lines.append(f"launches {step.launches}")
    step.close()
torch.cuda.synchronize()
text = "\n".join(lines) + "\n"
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
else:
    sys.stdout.write(text)
