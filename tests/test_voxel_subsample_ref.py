"""The CPU restatement of the seeded per-voxel subsample (tests/voxel_subsample_ref.py) against the deterministic oracle, the
scalar Philox of tests/augment_ref.py, and the statistics a random subsample must have.  No GPU."""
import numpy as np

import augment_ref
import voxel_subsample_ref as S
from oracle import voxel_ref

GRID = dict(xSize=1.0, ySize=1.0, zSize=1.0, sampleSize=35, maxVoxelX=4, maxVoxelY=4, maxVoxelZ=4)


def test_vector_philox_is_the_scalar_one():
    idx = np.array([0, 1, 2, 69, 70, 12345, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.uint64)
    for seed, item, epoch in ((0, 0, 0), (7, 3, 5), (2 ** 63 + 11, 2 ** 32 - 1, 9)):
        got = S.philox_word0(seed, item, epoch, idx)
        want = [augment_ref.words(seed, S.STREAM, item, epoch, int(i))[0] for i in idx]
        assert got.tolist() == want
        assert S.keys(seed, item, epoch, idx).tolist() == [(w << 32) | int(i) for w, i in zip(want, idx)]


def test_small_voxels_are_the_deterministic_oracle():
    """count <= sampleSize everywhere: nothing is drawn, the restatement is voxelize_ref."""
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(-4, 4, 900), rng.uniform(-4, 4, 900), rng.uniform(0, 4, 900)], 1)
    pts[:30] = (1.5, 1.5, 1.5) + rng.uniform(-0.4, 0.4, (30, 3))                  # one voxel of at least 30 points
    ref = voxel_ref.voxelize_ref(pts, **GRID)
    assert 30 <= ref["counts"].max() <= GRID["sampleSize"]
    got = S.voxelize_draw_ref(pts, **GRID, seed=7, item=3, epoch=1)
    for k in ("coords", "counts", "npts", "feats", "point_index"):
        assert np.array_equal(got[k], ref[k]), k


def test_oversize_voxels_differ_only_inside_and_stay_sorted():
    rng = np.random.default_rng(3)
    a = np.stack([rng.uniform(1, 2, 200), rng.uniform(1, 2, 200), rng.uniform(1, 2, 200)], 1)      # one crowded voxel
    b = np.stack([rng.uniform(-4, 4, 300), rng.uniform(-4, 4, 300), rng.uniform(0, 4, 300)], 1)
    pts = np.concatenate([a, b])
    rng.shuffle(pts)
    ref = voxel_ref.voxelize_ref(pts, **GRID)
    got = S.voxelize_draw_ref(pts, **GRID, seed=7, item=3, epoch=1)
    for k in ("coords", "counts", "npts"):
        assert np.array_equal(got[k], ref[k]), k
    big = ref["counts"] > GRID["sampleSize"]
    assert big.sum() == 1
    assert np.array_equal(got["feats"][~big], ref["feats"][~big])
    assert not np.array_equal(got["point_index"][big], ref["point_index"][big])
    assert (np.diff(got["point_index"][big][0]) > 0).all()                                          # ascending point index


def test_rule_is_uniform_and_redrawn_every_epoch():
    """256 voxels of 70 points (voxel v holds points 70 v .. 70 v + 69), sampleSize 35, seed 7, item 3, epochs 0..7: every
    in-voxel position is kept 256 * 8 / 2 = 1024 times in expectation, sigma = sqrt(2048 * 0.25) = 22.6 -- asserted within
    4 sigma -- and two consecutive epochs share half their kept points (+- 0.02)."""
    n_vox, per, T = 256, 70, 35
    kept = np.zeros((8, n_vox, per), dtype=bool)
    for epoch in range(8):
        for v in range(n_vox):
            sel = S.keep(np.arange(v * per, (v + 1) * per), T, 7, 3, epoch)
            assert len(sel) == T and (np.diff(sel) > 0).all()
            kept[epoch, v, sel - v * per] = True
    count = kept.sum(axis=(0, 1))
    print("kept per position:", count.min(), "..", count.max())
    assert count.sum() == 8 * n_vox * T
    assert (np.abs(count - 1024) <= 91).all(), (count.min(), count.max())
    for epoch in range(7):
        overlap = (kept[epoch] & kept[epoch + 1]).sum() / (n_vox * T)
        print("overlap of epochs", epoch, epoch + 1, overlap)
        assert abs(overlap - 0.5) <= 0.02, (epoch, overlap)
