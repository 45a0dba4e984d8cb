"""Training-time augmentation of a lidar sweep together with its boxes (VoxelNet section 3.3), on the GPU, and the
keras.utils.Sequence-like stream of augmented sweeps that Model.fit(x=...) trains on.  Ours, not the reference's: it
trains on fixed sweeps with precomputed label maps.

Per (seed, item, epoch): every box, in index order, is turned by U[-rot_box, rot_box] and shifted by N(0, sigma^2) per axis
-- the first of `attempts` candidates whose footprint touches no other box is taken, else the box stays -- and the points
inside it ride along; then the whole scene is scaled by U[scale] and rotated by U[-rot_global, rot_global] about the z
axis.  The draws are Philox4x32-10 counters (include/lisec_hip.h section 5c), so an item is a pure function of
(seed, item, epoch).  Box rows are (x, y, z, l, w, h, yaw) in ego metres, z the box centre, as boxes.annotationBoxes
returns them.  The label maps of the moved boxes are made on the device too (boxes.rpnTargets)."""
import math

import numpy as np
import torch

from . import _lib, boxes as _boxes, ops

PAD_LIMIT = 0.5e6             # rows at |x| >= this are the pad rows of a recorded step's point buffer (_StepPlans.PAD / 2)

DEFAULTS = dict(rot_box=math.pi / 10, sigma=(1.0, 1.0, 0.0), scale=(0.95, 1.05), rot_global=math.pi / 4, attempts=10)
IDENTITY = dict(rot_box=0.0, sigma=(0.0, 0.0, 0.0), scale=(1.0, 1.0), rot_global=0.0, attempts=0)


def _params(params):
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"unknown augmentation parameter(s) {', '.join(unknown)}: {', '.join(sorted(DEFAULTS))} are accepted")
    return ops.augment_params(**dict(DEFAULTS, **params))


def _device_points(points, dev):
    """(n, >= 3) float32 / float64 points on the device, rows of unit element stride."""
    if not torch.is_tensor(points):
        points = np.asarray(points)
        if points.dtype not in (np.float32, np.float64):
            points = points.astype(np.float64)
        points = torch.from_numpy(np.ascontiguousarray(points))
    if points.dtype not in (torch.float32, torch.float64):
        points = points.double()
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("points must have shape (n, >= 3)")
    points = points.to(dev)
    return points if points.shape[0] == 0 or points.stride(1) == 1 else points.contiguous()


def _device_boxes(boxes, dev):
    if torch.is_tensor(boxes):
        return boxes.to(device=dev, dtype=torch.float64).reshape(-1, 7).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 7))).to(dev)


def augment_sweep(points, boxes, seed, item=0, epoch=0, out=None, **params):
    """One augmented (sweep, boxes): points (n, >= 3) numpy or device tensor, boxes (B, 7) -> (points' (n, 3) in the
    points' dtype, boxes' (B, 7) float64), device tensors; nothing waits for the GPU.  params: rot_box, sigma, scale,
    rot_global, attempts (DEFAULTS).  out: a dense (n, 3) device tensor to write the points into."""
    dev = _lib.require_gpu()
    p = _params(params)
    pts, bx = _device_points(points, dev), _device_boxes(boxes, dev)
    transforms, glob, boxes_out, _, _ = ops.augment_draw(bx, p, seed, item, epoch)
    if out is None:
        out = torch.empty((pts.shape[0], 3), dtype=pts.dtype, device=dev)
    ops.augment_apply(pts, bx, transforms, glob, out, PAD_LIMIT)
    return out, boxes_out


class _Staged:
    """Item i of an AugmentedSweeps as a recorded step stages it: straight into the step's point and target buffers."""

    def __init__(self, seq, i):
        self.seq, self.i = seq, i

    def stage_into(self, points, y_cls, y_reg):
        return self.seq.stage(self.i, points, y_cls, y_reg)


class AugmentedSweeps:
    """keras.utils.Sequence of augmented training sweeps: len(), seq[i] -> (points' (n, 3) device tensor, [y_cls, y_reg]
    device float32), on_epoch_end() moves on to the next epoch's draws.  The same (seed, epoch, i) always gives the same
    item.  points_list[i]: (n, >= 3) numpy or device tensor, boxes_list[i]: (B, 7) rows as boxes.annotationBoxes returns
    them; both are uploaded once.  augment=False yields the sweeps as they are, with device-made labels; balance=False
    skips the region balancing of the label maps.  params: as augment_sweep.  Model.fit(x=AugmentedSweeps(...)) trains on
    it: the augmentation and the label kernels run where fit() stages a sweep, and write the step's buffers directly."""

    def __init__(self, points_list, boxes_list, seed=0, augment=True, balance=True, **params):
        if len(points_list) != len(boxes_list):
            raise ValueError("one box set per sweep")
        dev = _lib.require_gpu()
        self.params = _params(params)
        self.seed, self.augment, self.balance, self.epoch = int(seed), bool(augment), bool(balance), 0
        self.points = [_device_points(p, dev) for p in points_list]
        self.boxes = [_device_boxes(b, dev) for b in boxes_list]
        for b in self.boxes:
            if b.shape[0] > _lib.AUG_MAX_BOXES:
                raise ValueError(f"{b.shape[0]} boxes in one sweep exceed the limit of {_lib.AUG_MAX_BOXES}")
        self.max_points = max((int(p.shape[0]) for p in self.points), default=0)
        self.dtype = torch.float64 if any(p.dtype == torch.float64 for p in self.points) else torch.float32

    def __len__(self):
        return len(self.points)

    def on_epoch_end(self):
        self.epoch += 1

    def staged(self, i):
        """Item i for a recorded step (it has stage_into(points, y_cls, y_reg))."""
        return _Staged(self, int(i))

    def stage(self, i, points, y_cls, y_reg):
        """Writes item i into the caller's buffers: points (capacity >= n, 3) of any float dtype -- rows n.. are left alone --
        and the dense float32 label maps.  Returns n."""
        src, bx = self.points[i], self.boxes[i]
        n = int(src.shape[0])
        if n > points.shape[0]:
            raise ValueError(f"sweep of {n} points exceeds the capacity {points.shape[0]}")
        if self.augment:
            transforms, glob, bx_out, _, _ = ops.augment_draw(bx, self.params, self.seed, i, self.epoch)
            if src.dtype == points.dtype:
                ops.augment_apply(src, bx, transforms, glob, points[:n], PAD_LIMIT)
            else:
                tmp = torch.empty((n, 3), dtype=src.dtype, device=src.device)
                points[:n].copy_(ops.augment_apply(src, bx, transforms, glob, tmp, PAD_LIMIT))
        else:
            bx_out = bx
            points[:n].copy_(src[:, :3])
        _boxes.rpnTargets(bx_out, seed=self.seed, item=i, epoch=self.epoch, balance=self.balance, out=[y_cls, y_reg])
        return n

    def __getitem__(self, i):
        i = range(len(self))[i]
        dev = self.points[i].device
        ho_wo = _boxes._cfg()
        pts = torch.empty((self.points[i].shape[0], 3), dtype=self.points[i].dtype, device=dev)
        y_cls = torch.empty((ho_wo.outX, ho_wo.outY, 2), dtype=torch.float32, device=dev)
        y_reg = torch.empty((ho_wo.outX, ho_wo.outY, 14), dtype=torch.float32, device=dev)
        self.stage(i, pts, y_cls, y_reg)
        return pts, [y_cls, y_reg]
