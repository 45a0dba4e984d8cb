"""Training-time augmentation of a lidar sweep together with its boxes (VoxelNet section 3.3), on the GPU, and the
keras.utils.Sequence-like stream of augmented sweeps that Model.fit(x=...) trains on.  Ours, not the reference's: it
trains on fixed sweeps with precomputed label maps.

Per (seed, item, epoch): every box, in index order, is turned by U[-rot_box, rot_box] and shifted by N(0, sigma^2) per axis
-- the first of `attempts` candidates whose footprint touches no other box is taken, else the box stays -- and the points
inside it ride along; then the whole scene is scaled by U[scale] and rotated by U[-rot_global, rot_global] about the z
axis.  The draws are Philox4x32-10 counters (include/lisec_hip.h section 5c), so an item is a pure function of
(seed, item, epoch).  Box rows are (x, y, z, l, w, h, yaw) in ego metres, z the box centre, as boxes.annotationBoxes
returns them.  The label maps of the moved boxes are made on the device too (boxes.rpnTargets).

Ground-truth object sampling (Yan et al., SECOND, 2018, section 3.2) comes in front of the noise when an ObjectDatabase is
given: up to `sample_to - B` objects cut out of other sweeps are drawn (Philox stream 3), those whose footprint touches
neither a scene box nor an earlier accepted object are pasted at their original pose, the scene points inside a pasted box
are removed, and the pasted boxes take the per-box noise like any other.  How many objects are accepted is known only on the
device, so the sweep keeps a FIXED row count, n + database.bound(K): removed and unused rows are pad rows at (1e6, 1e6, 1e6),
which the voxeliser drops as it drops any point outside the grid, and the box count travels as a device int32."""
import math

import numpy as np
import torch

from . import _lib, boxes as _boxes, ops
from .voxelizer import check_subsample

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


class ObjectDatabase:
    """The objects ground-truth sampling pastes: every box of the given sweeps that owns at least min_points points (closed
    slab test, a point inside several boxes belongs to the lowest index), with those points in the sweep's order and dtype, as
    absolute ego coordinates (min_points below 1 counts as 1: an object has points).  Built on the device (lisec_augment_owner, then a stable sort by owner).  boxes (M, 7) float64,
    points (P, 3), offsets (M + 1,) int32 -- object m owns points[offsets[m]:offsets[m + 1]] --, counts (M,) int32: device
    tensors; dtype: float64 when any sweep is, else float32; len() = M, which may be 0 (nothing is ever sampled then)."""

    def __init__(self, points_list, boxes_list, min_points=5):
        if len(points_list) != len(boxes_list):
            raise ValueError("one box set per sweep")
        dev = _lib.require_gpu()
        sweeps = [_device_points(p, dev) for p in points_list]
        self.dtype = torch.float64 if any(p.dtype == torch.float64 for p in sweeps) else torch.float32
        self.min_points = int(min_points)
        rows, pts, counts = [], [], []
        for p, b in zip(sweeps, boxes_list):
            b = _device_boxes(b, dev)
            if b.shape[0] == 0:
                continue
            own = ops.augment_owner(p, b, PAD_LIMIT).long()
            per_box = torch.bincount(own + 1, minlength=b.shape[0] + 1)[1:]        # plumbing: the build is not on the step's path
            keep = per_box >= max(self.min_points, 1)
            order = torch.sort(own, stable=True).indices                             # by box, the sweep's point order within
            sorted_own = own[order]
            sel = order[(sorted_own >= 0) & keep[sorted_own.clamp(min=0)]]
            rows.append(b[keep])
            pts.append(p[sel, :3].to(self.dtype))
            counts.append(per_box[keep])
        self.boxes = torch.cat(rows) if rows else torch.zeros((0, 7), dtype=torch.float64, device=dev)
        self.points = (torch.cat(pts) if pts else torch.zeros((0, 3), dtype=self.dtype, device=dev)).contiguous()
        counts = torch.cat(counts) if counts else torch.zeros(0, dtype=torch.int64, device=dev)
        self.counts = counts.to(torch.int32)
        self.offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)]).to(torch.int32)
        self._largest = np.sort(self.counts.cpu().numpy().astype(np.int64))[::-1]
        self._as = {self.dtype: self.points}

    def __len__(self):
        return int(self.boxes.shape[0])

    def bound(self, K):
        """The most points K sampled objects can add: the sum of the K largest point counts (known on the host)."""
        return int(self._largest[:max(int(K), 0)].sum())

    def points_as(self, dtype):
        """The points in `dtype` (a float32 database pasted into a float64 sweep; converted once)."""
        if dtype not in self._as:
            self._as[dtype] = self.points.to(dtype)
        return self._as[dtype]


def _sample_count(B, sample_to):
    """K of section 5c: the candidates drawn for a scene of B boxes."""
    K = min(_lib.AUG_MAX_SAMPLES, max(0, int(sample_to) - B))
    if B + K > _lib.AUG_MAX_BOXES:
        raise ValueError(f"{B} boxes and {K} sampled objects exceed the limit of {_lib.AUG_MAX_BOXES}")
    return K


def _sample_paste(pts, bx, database, sample_to, seed, item, epoch):
    """sample + paste of one sweep (device points, device rows) -> (scratch points (n + bound, 3) in the wider of the two
    dtypes, boxes_all (B + K, 7), n_boxes (1,) int32, index (K,))."""
    K = _sample_count(int(bx.shape[0]), sample_to)
    dtype = torch.float64 if torch.float64 in (pts.dtype, database.dtype) else torch.float32
    if pts.dtype != dtype:
        pts = pts[:, :3].to(dtype)
    index, n_boxes, boxes_all, point_offset, _ = ops.augment_sample(bx, database.boxes, database.offsets, K, seed, item, epoch)
    out = torch.empty((int(pts.shape[0]) + database.bound(K), 3), dtype=dtype, device=pts.device)
    ops.augment_paste(pts, database.points_as(dtype), database.offsets, index, point_offset, boxes_all, n_boxes, out, PAD_LIMIT)
    return out, boxes_all, n_boxes, index


def sample_objects(points, boxes, database, sample_to, seed, item=0, epoch=0):
    """Ground-truth sampling alone, as augment_sweep is draw + apply alone: K = min(64, max(0, sample_to - B)) objects of
    `database` are drawn for (seed, item, epoch) and the accepted ones pasted.  Returns device tensors (points' (n +
    database.bound(K), 3): the scene rows, the pasted points, then pad rows at 1e6 -- a scene point inside a pasted box is
    a pad row too --, boxes_all (B + K, 7): the scene rows then the accepted ones, zero past n_boxes, n_boxes (1,) int32,
    index (K,) int32: the database index of candidate k or -1).  Nothing waits for the GPU."""
    dev = _lib.require_gpu()
    return _sample_paste(_device_points(points, dev), _device_boxes(boxes, dev), database, sample_to, seed, item, epoch)


def augment_sweep(points, boxes, seed, item=0, epoch=0, out=None, database=None, sample_to=0, **params):
    """One augmented (sweep, boxes): points (n, >= 3) numpy or device tensor, boxes (B, 7) -> (points' (n, 3) in the
    points' dtype, boxes' (B, 7) float64), device tensors; nothing waits for the GPU.  params: rot_box, sigma, scale,
    rot_global, attempts (DEFAULTS).  out: a dense (n, 3) device tensor to write the points into.
    database: an ObjectDatabase to sample up to sample_to - B objects from in front of the noise (sample_objects); the
    result is then (points' (n + bound, 3), pad rows included, boxes' (B + K, 7), zero past n_boxes, n_boxes (1,) int32)."""
    dev = _lib.require_gpu()
    p = _params(params)
    pts, bx = _device_points(points, dev), _device_boxes(boxes, dev)
    if database is not None:
        scratch, boxes_all, n_boxes, _ = _sample_paste(pts, bx, database, sample_to, seed, item, epoch)
        transforms, glob, boxes_out, _, _ = ops.augment_draw(boxes_all, p, seed, item, epoch, n_boxes=n_boxes)
        if out is None:
            out = torch.empty_like(scratch)
        ops.augment_apply(scratch, boxes_all, transforms, glob, out, PAD_LIMIT, n_boxes=n_boxes)
        return out, boxes_out, n_boxes
    transforms, glob, boxes_out, _, _ = ops.augment_draw(bx, p, seed, item, epoch)
    if out is None:
        out = torch.empty((pts.shape[0], 3), dtype=pts.dtype, device=dev)
    ops.augment_apply(pts, bx, transforms, glob, out, PAD_LIMIT)
    return out, boxes_out


class _Staged:
    """Item i of an AugmentedSweeps as a recorded step stages it: straight into the step's point and target buffers."""

    def __init__(self, seq, i):
        self.seq, self.i = seq, i
        # (seed, item, epoch) of the voxeliser's per-voxel subsample, None for subsample='first'
        self.draw = (seq.seed, i, seq.epoch) if seq.subsample == "random" else None

    def stage_into(self, points, y_cls, y_reg):
        return self.seq.stage(self.i, points, y_cls, y_reg)


class AugmentedSweeps:
    """keras.utils.Sequence of augmented training sweeps: len(), seq[i] -> (points' (n, 3) device tensor, [y_cls, y_reg]
    device float32), on_epoch_end() moves on to the next epoch's draws.  The same (seed, epoch, i) always gives the same
    item.  points_list[i]: (n, >= 3) numpy or device tensor, boxes_list[i]: (B, 7) rows as boxes.annotationBoxes returns
    them; both are uploaded once.  augment=False yields the sweeps as they are, with device-made labels; balance=False
    skips the region balancing of the label maps -- the natural setting under losses.VoxelNetLoss, which normalises
    positives and negatives separately and needs no sampled subset.  params: as augment_sweep.  Model.fit(x=AugmentedSweeps(...)) trains on
    it: the augmentation and the label kernels run where fit() stages a sweep, and write the step's buffers directly.
    database: an ObjectDatabase; every item is then filled up towards sample_to boxes with sampled objects before the
    noise (with augment=False: sampled and pasted only).  Item i then has n_i + database.bound(K_i) rows, pad rows at 1e6
    included -- the voxeliser drops them --, and max_points covers the largest.
    subsample='random': fit() voxelises item i with the reference's random per-voxel subsample as the draw of (seed, i,
    epoch) (Voxelizer(subsample='random')), so a crowded voxel keeps other points every epoch; 'first' (the default) keeps
    the lowest point indices.  The draw goes by the item index, not by the rank that trains on it: data parallel needs
    nothing more.  The items themselves -- points and label maps -- do not depend on it."""

    def __init__(self, points_list, boxes_list, seed=0, augment=True, balance=True, database=None, sample_to=15,
                 subsample="first", **params):
        if len(points_list) != len(boxes_list):
            raise ValueError("one box set per sweep")
        self.subsample = check_subsample(subsample)
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
        self.database, self.sample_to = database, int(sample_to)
        if database is not None:
            self.max_points = max((self.rows(i) for i in range(len(self.points))), default=0)
            if database.dtype == torch.float64:
                self.dtype = torch.float64

    def __len__(self):
        return len(self.points)

    def on_epoch_end(self):
        self.epoch += 1

    def rows(self, i):
        """The row count of item i: its sweep's, plus with a database the most points its sampled objects can add."""
        n = int(self.points[i].shape[0])
        if self.database is None:
            return n
        return n + self.database.bound(_sample_count(int(self.boxes[i].shape[0]), self.sample_to))

    def staged(self, i):
        """Item i for a recorded step (it has stage_into(points, y_cls, y_reg))."""
        return _Staged(self, int(i))

    def stage(self, i, points, y_cls, y_reg):
        """Writes item i into the caller's buffers: points (capacity >= n, 3) of any float dtype -- rows n.. are left alone --
        and the dense float32 label maps.  Returns n (with a database: rows(i), pad rows included)."""
        src, bx = self.points[i], self.boxes[i]
        n = self.rows(i)
        if n > points.shape[0]:
            raise ValueError(f"sweep of {n} points exceeds the capacity {points.shape[0]}")
        if self.database is not None:
            scratch, bx, n_boxes, _ = _sample_paste(src, bx, self.database, self.sample_to, self.seed, i, self.epoch)
            bx_out = bx
            if self.augment:
                transforms, glob, bx_out, _, _ = ops.augment_draw(bx, self.params, self.seed, i, self.epoch, n_boxes=n_boxes)
                if scratch.dtype == points.dtype:
                    ops.augment_apply(scratch, bx, transforms, glob, points[:n], PAD_LIMIT, n_boxes=n_boxes)
                else:
                    points[:n].copy_(ops.augment_apply(scratch, bx, transforms, glob, torch.empty_like(scratch), PAD_LIMIT,
                                                       n_boxes=n_boxes))
            else:
                points[:n].copy_(scratch)
            _boxes.rpnTargets(bx_out, seed=self.seed, item=i, epoch=self.epoch, balance=self.balance, out=[y_cls, y_reg],
                              n_boxes=n_boxes)
            return n
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
        pts = torch.empty((self.rows(i), 3), dtype=self.points[i].dtype, device=dev)
        y_cls = torch.empty((ho_wo.outX, ho_wo.outY, 2), dtype=torch.float32, device=dev)
        y_reg = torch.empty((ho_wo.outX, ho_wo.outY, 14), dtype=torch.float32, device=dev)
        self.stage(i, pts, y_cls, y_reg)
        return pts, [y_cls, y_reg]
