"""Test-local restatement of the seeded per-voxel subsample (lisec_voxelize_draw) -- TEST ONLY, never imported by the product.

Plain numpy, written from the text of include/lisec_hip.h section 1b: Philox4x32-10 with key = seed (low word, high word)
and counter = (4, item, epoch, point index); a voxel with more than sampleSize points keeps the sampleSize points with the
smallest keys (Philox word 0 << 32 | point index) and emits them in ascending point index.  Everything else -- the voxel
keys, the sequential fp64 centroid, the single rounding to fp32 -- is oracle.voxel_ref.voxelize_ref's arithmetic.
"""
import numpy as np

from oracle.voxel_ref import voxel_keys

STREAM = 4
_M32 = np.uint64(0xFFFFFFFF)


def philox_word0(seed, item, epoch, index):
    """Word 0 of Philox4x32-10(counter = (4, item, epoch, index), key = seed) for an array of indices: uint64 array holding
    32-bit values.  (tests/augment_ref.words is the scalar form; test_voxel_subsample_ref.py holds the two together.)"""
    index = np.asarray(index, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    c0 = np.full(index.shape, STREAM, dtype=np.uint64)
    c1 = np.full(index.shape, int(item) & 0xFFFFFFFF, dtype=np.uint64)
    c2 = np.full(index.shape, int(epoch) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = index & _M32
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def keys(seed, item, epoch, index):
    """The 64-bit selection keys of the points `index`: (Philox word 0 << 32) | index."""
    index = np.asarray(index, dtype=np.uint64)
    return (philox_word0(seed, item, epoch, index) << np.uint64(32)) | index


def keep(bucket, sampleSize, seed, item, epoch):
    """The points of one voxel that survive: `bucket` (point indices, any order) -> ascending indices, at most sampleSize."""
    bucket = np.sort(np.asarray(bucket, dtype=np.int64))
    if len(bucket) <= sampleSize:
        return bucket
    order = np.argsort(keys(seed, item, epoch, bucket), kind="stable")           # keys are unique
    return np.sort(bucket[order[:sampleSize]])


def voxelize_draw_ref(points, xSize, ySize, zSize, sampleSize, maxVoxelX, maxVoxelY, maxVoxelZ, seed, item=0, epoch=0):
    """voxelize_ref with the seeded subsample: dict(coords, counts, npts, row_start, row_point, feats, point_index, rows)."""
    p = np.asarray(points, dtype=np.float64)
    nxg, nyg = 2 * maxVoxelX, 2 * maxVoxelY
    valid, fx, fy, fz = voxel_keys(p, xSize, ySize, zSize, maxVoxelX, maxVoxelY, maxVoxelZ)
    idx = np.nonzero(valid)[0]
    lin = (fz[idx] * nxg + fx[idx]) * nyg + fy[idx]
    order = np.argsort(lin, kind="stable")
    lin_s, idx_s = lin[order], idx[order]
    ukeys, start, counts = np.unique(lin_s, return_index=True, return_counts=True)
    V = len(ukeys)
    coords = np.empty((V, 3), dtype=np.int32)
    coords[:, 0] = ukeys // (nxg * nyg)
    coords[:, 1] = (ukeys // nyg) % nxg
    coords[:, 2] = ukeys % nyg
    npts = np.minimum(counts, sampleSize).astype(np.int32)
    row_start = np.concatenate([[0], np.cumsum(npts)]).astype(np.int32)
    feats = np.zeros((V, sampleSize, 6), dtype=np.float32)
    pidx = np.full((V, sampleSize), -1, dtype=np.int32)
    for v in range(V):
        s = int(npts[v])
        sel = keep(idx_s[start[v]:start[v] + counts[v]], sampleSize, seed, item, epoch)
        cur = p[sel, :3]
        acc = np.zeros(3, dtype=np.float64)
        for r in range(s):                                 # np.mean's order: the rows one after the other, one divide
            acc = acc + cur[r]
        centroid = acc / np.float64(s)
        feats[v, :s, :] = np.hstack((cur, cur - centroid)).astype(np.float32)
        pidx[v, :s] = sel
    live = pidx >= 0
    return dict(coords=coords, counts=counts.astype(np.int32), npts=npts, row_start=row_start, feats=feats,
                point_index=pidx, row_point=pidx[live].astype(np.int32), rows=feats[live])
