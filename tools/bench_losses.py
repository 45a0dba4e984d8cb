"""The loss kernels on the Lyft head (M = 100*200 cells): the legacy pair (k_loss + k_loss_finalize, lisec_rpn_loss) against
lisec_head_loss (k_head_loss + k_head_loss_finalize, csrc/losses.hip) and lisec_detection_loss (k_det_count + k_det_loss +
k_det_finalize, csrc/detection_loss.hip; with metrics also lisec_detection_metrics: k_detm_anchors + k_detm_finalize,
csrc/detection_metrics.hip) and lisec_detection_iou_loss (the same with k_det_iou ahead of the finalize,
csrc/detection_iou_loss.hip) for the configurations of Model.compile below, each
timed over back-to-back launches with device events; then a short Model.fit on U20k sweeps under each, timed per step
(GPU box only).  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times: --config restricts the run to
one configuration, so that the per-kernel statistics of a profile hold that configuration alone.

    python tools/bench_losses.py [--config all|mse|smoothl1_ce|keras|keras_metrics|voxelnet|voxelnet_focal|voxelnet_metrics|
                                            voxelnet_iou] [--iters 500] [--fit-steps 20] [--repeats 1]

  mse             loss=['mse','mse']                          lisec_rpn_loss kind 0 (the reference's step)
  smoothl1_ce     loss='smoothl1_ce'                          lisec_rpn_loss kind 1
  keras           [BinaryCrossentropy(from_logits=True), Huber()]            lisec_head_loss, no metrics
  keras_metrics   the same with metrics [[BinaryAccuracy(threshold=0), 'accuracy'], ['mae', 'mse']]
  voxelnet        loss='voxelnet' (VoxelNetLoss(): gamma 0)           lisec_detection_loss
  voxelnet_focal  VoxelNetLoss(alpha=0.5, beta=1.5, gamma=2.0)        lisec_detection_loss, the pow() path
  voxelnet_metrics  loss='voxelnet' with the five detection metrics   lisec_detection_loss + lisec_detection_metrics
  voxelnet_iou    VoxelNetIoULoss(iou_mode='3d')                      lisec_detection_iou_loss

--repeats N times the fit N times per configuration and prints each: the run-to-run spread."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic_targets, u20k_cloud
from lisec_amd import Constants, ops
from lisec_amd import model_training as mt

K, Mx = mt.losses, mt.metrics


def _configs():
    configs = {
        "mse": dict(loss=["mse", "mse"]),
        "smoothl1_ce": dict(loss="smoothl1_ce"),
        "keras": dict(loss=[K.BinaryCrossentropy(from_logits=True), K.Huber()]),
        "keras_metrics": dict(loss=[K.BinaryCrossentropy(from_logits=True), K.Huber()],
                              metrics=[[Mx.BinaryAccuracy(threshold=0.0), "accuracy"], ["mae", "mse"]]),
        "voxelnet": dict(loss="voxelnet"),
        "voxelnet_focal": dict(loss=K.VoxelNetLoss(alpha=0.5, beta=1.5, gamma=2.0)),
        "voxelnet_metrics": dict(loss="voxelnet", metrics=["anchor_precision", "anchor_recall", "anchor_accuracy",
                                                           "positive_mae", "positive_iou"]),
    }
    if hasattr(K, "VoxelNetIoULoss"):                # absent from a parent commit the tool is run against
        configs["voxelnet_iou"] = dict(loss=K.VoxelNetIoULoss(iou_mode="3d"))
    return configs


def _kernel_time(step_loss, head, yc, yr, M, iters):
    """us per loss call (kernel + finalize), back to back on one stream."""
    dev = head.device
    dhead = torch.empty_like(head)
    loss_out = torch.zeros(3, dtype=torch.float32, device=dev)
    met = torch.zeros(8, dtype=torch.float32, device=dev)
    if isinstance(step_loss, K.LossSpec):
        desc = step_loss.descriptor()
        call = lambda: ops.head_loss(desc, head, yc, yr, M, dhead, loss_out, met)          # noqa: E731
    elif isinstance(step_loss, getattr(K, "DetectionLossSpec", ())):
        desc = step_loss.descriptor()
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        mdesc = step_loss.metrics_descriptor()
        pairs = torch.zeros(16, dtype=torch.float64, device=dev)

        with_iou = isinstance(step_loss, getattr(K, "DetectionIoULossSpec", ()))
        run = ops.detection_iou_loss if with_iou else ops.detection_loss

        def call():
            run(desc, head, yc, yr, M, dhead, loss_out, counts)
            if mdesc is not None:
                ops.detection_metrics(mdesc, head, yc, yr, M, pairs)
    else:
        kind = {"mse": 0, "smoothl1_ce": 1}[step_loss]
        call = lambda: ops.rpn_loss(head, yc, yr, M, kind, dhead, loss_out)                 # noqa: E731
    for _ in range(20):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        call()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters, loss_out.cpu().numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(_configs()))
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--fit-steps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    configs = _configs() if args.config == "all" else {args.config: _configs()[args.config]}
    dev = torch.device("cuda")
    Ho, Wo = Constants.nx // 2, Constants.ny // 2
    M = Ho * Wo
    rng = np.random.default_rng(0)
    head = torch.from_numpy(rng.normal(0, 1, (M, 16)).astype(np.float32)).to(dev)
    tc, tr = synthetic_targets(0, Ho, Wo)
    yc, yr = torch.from_numpy(tc).to(dev), torch.from_numpy(tr).to(dev)
    n = args.sweeps
    x = [mt.VFE_preprocessing(u20k_cloud(i), Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                              Ho, Wo, Constants.nz) for i in range(n)]
    tg = [synthetic_targets(i, Ho, Wo) for i in range(n)]
    y = [np.stack([t[0] for t in tg]), np.stack([t[1] for t in tg])]
    model = mt.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    print(f"{'config':<15}{'loss kernels us/call':>22}{'fit ms/step':>14}  loss_out", flush=True)
    for name, kw in configs.items():
        step_loss, _ = K.compile_loss(kw["loss"], metrics=kw.get("metrics"))
        us, lo = _kernel_time(step_loss, head, yc, yr, M, args.iters)
        model.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), **kw)
        model.fit(x=x, y=y, verbose=0, epochs=1, steps_per_epoch=4)                       # records the step plan
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.fit(x=x, y=y, verbose=0, epochs=1, steps_per_epoch=args.fit_steps)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / args.fit_steps
            print(f"{name:<15}{us:>22.2f}{ms:>14.3f}  {np.array2string(lo, precision=5)}", flush=True)
