"""Host side of the HIP voxeliser (lisec_voxelize, include/lisec_hip.h section 1).

Mirrors VFE_preprocessing of the reference (model_training.py:112-152): same arguments,
same (z, x, y, t, f) index convention, but the result stays on the GPU as occupied voxels +
compact feature rows instead of a 134 M element dense tensor.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import VoxelCfg


class VoxelSample:
    """Device-resident result of one voxeliser call (one lidar sweep).

    info        int32[8]   V, rows, valid points, max count, overflow (LISEC_VI_*)
    cell_voxel  int32[NZ*NX*NY]   voxel ordinal per grid cell (-1 = empty)
    coords      int32[cap,3]      (z, x, y)
    counts/npts int32[cap]
    row_start   int32[cap+1]
    rows        float32[n,6]      compact feature rows
    row_point   int32[n]          original point index per row
    row_stats   int64[LISEC_ROW_STATS_WORDS]  first / second moments of the rows (fixed point) + VFE scratch
    draw        int32[4] or None  (seed low word, seed high word, item, epoch) of the per-voxel subsample, read by the
                kernel when it runs; only a sample of a Voxelizer(subsample='random') has it
    """

    def __init__(self, cfg, n_points, cap, info, cell_voxel, coords, counts, npts, row_start, rows,
                 row_point, row_stats=None, draw=None):
        self.cfg, self.n_points, self.cap = cfg, n_points, cap
        self.info, self.cell_voxel, self.coords = info, cell_voxel, coords
        self.counts, self.npts, self.row_start = counts, npts, row_start
        self.rows, self.row_point, self.row_stats, self.draw = rows, row_point, row_stats, draw
        self._host_info = None

    @property
    def grid_shape(self):
        c = self.cfg
        return (c.maxVoxelZ, 2 * c.maxVoxelX, 2 * c.maxVoxelY)

    def host_info(self):
        """Synchronises; returns dict(V, rows, valid, max_count)."""
        if self._host_info is None:
            h = self.info.cpu().numpy()
            if h[4]:
                raise _lib.LisecError("voxeliser output capacity overflow")
            self._host_info = dict(V=int(h[0]), rows=int(h[1]), valid=int(h[2]), max_count=int(h[3]))
        return self._host_info

    def to_host(self):
        """numpy copies trimmed to V / rows (same keys as oracle.voxel_ref.voxelize_ref)."""
        hi = self.host_info()
        V, R, T = hi["V"], hi["rows"], self.cfg.sampleSize
        out = dict(coords=self.coords[:V].cpu().numpy(), counts=self.counts[:V].cpu().numpy(),
                   npts=self.npts[:V].cpu().numpy(), row_start=self.row_start[:V + 1].cpu().numpy(),
                   rows=self.rows[:R].cpu().numpy(), row_point=self.row_point[:R].cpu().numpy())
        out["feats"] = self.padded_feats()[:V].cpu().numpy()
        pidx = np.full((V, T), -1, dtype=np.int32)
        for_rows = np.repeat(np.arange(V), out["npts"])
        slot = np.arange(R) - out["row_start"][for_rows]
        pidx[for_rows, slot] = out["row_point"]
        out["point_index"] = pidx
        return out

    def padded_feats(self):
        """(V, T, 6) zero padded feature blocks on the device (model_training.py:141)."""
        V = self.host_info()["V"]
        T = self.cfg.sampleSize
        padded = torch.empty((max(V, 1), T, 6), dtype=torch.float32, device=self.rows.device)
        lib = _lib.load()
        _lib.check(lib.lisec_voxel_rows_to_padded(_lib.ptr(self.info), _lib.ptr(self.npts),
                                                  _lib.ptr(self.row_start), _lib.ptr(self.rows), T, V,
                                                  _lib.ptr(padded), _lib.current_stream()))
        return padded[:V]


def host_row_stats(rows):
    """row_stats for rows that did not come from lisec_voxelize (a dense array turned into a sample): the 6 + 21
    moments in the same two-limb fixed-point layout (everything in replica 0), VFE scratch zeroed."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    vals = [r[:, j].sum() for j in range(6)] + [(r[:, j] * r[:, k]).sum() for j in range(6) for k in range(j, 6)]
    out = np.zeros(_lib.ROW_STATS_WORDS, dtype=np.int64)
    for i, s in enumerate(vals):
        hi = np.floor(s * 256.0)
        out[2 * i] = int(hi)
        out[2 * i + 1] = int(np.rint((s - hi / 256.0) * 1099511627776.0))
    return out


SUBSAMPLE_MODES = ("first", "random")


def check_subsample(mode):
    if mode not in SUBSAMPLE_MODES:
        raise ValueError(f"subsample must be one of {', '.join(SUBSAMPLE_MODES)}, not {mode!r}")
    return mode


class Voxelizer:
    """Reusable voxeliser for one grid; owns its workspace (grown on demand).

    subsample: which points a voxel holding more than sampleSize keeps.  'first' (the default, lisec_voxelize): the lowest
    point indices.  'random' (lisec_voxelize_draw, include/lisec_hip.h section 1b): the reference's random choice, as a
    seeded draw that is a pure function of (seed, item, epoch) and the point's row index -- the same whatever the arrival
    order, the padding behind the sweep or the rank that voxelises it (data parallel: the draw goes by the item index).
    The slots of a voxel stay in ascending point index either way."""

    def __init__(self, xSize, ySize, zSize, sampleSize, maxVoxelX, maxVoxelY, maxVoxelZ, device=None, subsample="first",
                 seed=0):
        self.subsample, self.seed = check_subsample(subsample), int(seed)
        self.device = device or _lib.require_gpu()
        self.lib = _lib.load()
        self.cfg = VoxelCfg(float(xSize), float(ySize), float(zSize), int(maxVoxelX), int(maxVoxelY),
                            int(maxVoxelZ), int(sampleSize))
        self.ncells = 4 * int(maxVoxelX) * int(maxVoxelY) * int(maxVoxelZ)
        self._ws = None

    def _workspace(self, n):
        need = self.lib.lisec_voxelize_workspace_bytes(ctypes.byref(self.cfg), n)
        if need == 0:
            raise _lib.LisecError("invalid voxel grid configuration: " + self.lib.lisec_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.bump_alloc_generation()           # recorded step plans hold the old address
        return self._ws

    def set_draw(self, sample, item, epoch, seed=None):
        """Writes (seed, item, epoch) into the draw words of `sample` on the current stream: a one-thread kernel with
        scalar arguments, so nothing waits for the GPU.  seed: this voxeliser's unless given."""
        if sample.draw is None:
            raise ValueError("the sample has no draw words: it was not made by a Voxelizer(subsample='random')")
        seed = self.seed if seed is None else int(seed)
        _lib.check(self.lib.lisec_voxel_draw_set(_lib.ptr(sample.draw), seed & (2 ** 64 - 1), int(item) & 0xffffffff,
                                                 int(epoch) & 0xffffffff, _lib.current_stream()))

    def _enqueue(self, pts, n, stride, ws, cap, s):
        args = (ctypes.byref(self.cfg), _lib.ptr(pts), 0 if pts.dtype == torch.float32 else 1, n, stride,
                _lib.ptr(ws), ws.numel(), cap, _lib.ptr(s.info), _lib.ptr(s.cell_voxel), _lib.ptr(s.coords),
                _lib.ptr(s.counts), _lib.ptr(s.npts), _lib.ptr(s.row_start), _lib.ptr(s.rows),
                _lib.ptr(s.row_point), _lib.ptr(s.row_stats))
        if self.subsample == "random":
            if s.draw is None:
                raise ValueError("out: a sample without draw words (made by a subsample='first' voxeliser)")
            _lib.check(self.lib.lisec_voxelize_draw(*args, _lib.ptr(s.draw), _lib.current_stream()))
        else:
            _lib.check(self.lib.lisec_voxelize(*args, _lib.current_stream()))

    def __call__(self, points, out=None, draw=None):
        """points: (N, >=3) float32/float64 numpy array or torch tensor (host or device).
        out: a VoxelSample of an earlier call with the same number of points whose buffers are written again (a recorded
        step plan points at fixed addresses).
        draw: (item, epoch) of a subsample='random' voxeliser, written into the sample's draw words in front of the
        launches.  None leaves the words of `out` alone -- a call made while a step plan is recorded bakes in their
        address, not their values, and whoever replays the plan sets them (set_draw) -- and gives a new sample (0, 0)."""
        if draw is not None and self.subsample != "random":
            raise ValueError("draw: only a Voxelizer(subsample='random') draws")
        if isinstance(points, np.ndarray):
            if points.dtype not in (np.float32, np.float64):
                points = points.astype(np.float64)
            points = torch.from_numpy(np.ascontiguousarray(points))
        if points.dtype not in (torch.float32, torch.float64):
            points = points.double()
        if points.dim() != 2 or points.shape[1] < 3:
            raise ValueError("points must have shape (N, >=3)")
        pts = points.to(self.device, non_blocking=True).contiguous()
        n, stride = int(pts.shape[0]), int(pts.shape[1])
        cap = min(n, self.ncells)
        dev, i32 = self.device, torch.int32
        ws = self._workspace(n)
        if out is not None:
            if out.n_points != n or out.cap != cap:
                raise ValueError("out: a sample of another size")
            if draw is not None:
                self.set_draw(out, *draw)
            self._enqueue(pts, n, stride, ws, cap, out)
            out._keepalive, out._host_info = pts, None
            return out
        info = torch.empty(8, dtype=i32, device=dev)
        cell_voxel = torch.empty(self.ncells, dtype=i32, device=dev)
        coords = torch.empty((max(cap, 1), 3), dtype=i32, device=dev)
        counts = torch.empty(max(cap, 1), dtype=i32, device=dev)
        npts = torch.empty(max(cap, 1), dtype=i32, device=dev)
        row_start = torch.empty(max(cap, 1) + 1, dtype=i32, device=dev)
        rows = torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev)
        row_point = torch.empty(max(n, 1), dtype=i32, device=dev)
        row_stats = torch.empty(_lib.ROW_STATS_WORDS, dtype=torch.int64, device=dev)
        s = VoxelSample(self.cfg, n, cap, info, cell_voxel, coords, counts, npts, row_start, rows,
                        row_point, row_stats)
        if self.subsample == "random":
            s.draw = torch.empty(4, dtype=i32, device=dev)
            self.set_draw(s, *(draw or (0, 0)))
        self._enqueue(pts, n, stride, ws, cap, s)
        s._keepalive = pts
        return s
