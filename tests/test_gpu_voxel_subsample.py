"""The seeded per-voxel subsample on the GPU (lisec_voxelize_draw, Voxelizer(subsample='random')) against its CPU
restatement (tests/voxel_subsample_ref.py, written from include/lisec_hip.h section 1b), bit for bit, and through
Model.fit on the recorded, the pipelined and the Python schedule."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_subsample_ref as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

# 4 x 8 x 8 cells of edge 1: the strict range test keeps z cells 1..3 and x, y cells 1..7
GRID = dict(xSize=1.0, ySize=1.0, zSize=1.0, maxVoxelX=4, maxVoxelY=4, maxVoxelZ=4)
# points per voxel: both sides of every branch of the kernel (35 | 36 the draw, 64 | 65 shuffles | radix select, 384 | 385
# Philox words cached in LDS | computed again per pass)
COUNTS = (1, 35, 36, 63, 64, 65, 128, 129, 5003, 2, 40, 384, 385)
SEED, ITEM, EPOCH = 7, 3, 1


@functools.lru_cache(maxsize=None)
def _sweep():
    """One sweep (float64) with voxels of COUNTS points: a fifth of every crowded voxel's points are exact duplicates of
    others, and the rows are shuffled, so a voxel's points are scattered over the buffer."""
    rng = np.random.default_rng(41)
    cells = [(x, y, z) for z in (1, 2, 3) for x in (-3, -1, 0, 2) for y in (-3, 0, 1, 3)]
    pts = []
    for (x, y, z), c in zip(cells, COUNTS):
        p = np.array([x, y, z], dtype=np.float64) + rng.uniform(0.05, 0.95, (c, 3))
        if c >= 10:
            p[: c // 5] = p[c // 5: 2 * (c // 5)]
        pts.append(p)
    pts = np.concatenate(pts)
    rng.shuffle(pts)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _ref(dtype, T, item=ITEM, epoch=EPOCH):
    return S.voxelize_draw_ref(_sweep().astype(dtype).astype(np.float64), sampleSize=T, **GRID, seed=SEED, item=item, epoch=epoch)


def _vox(T, **kw):
    from lisec_amd.voxelizer import Voxelizer
    return Voxelizer(sampleSize=T, **GRID, subsample="random", seed=SEED, **kw)


def _decode_row_stats(words):
    from lisec_amd import _lib
    w = np.asarray(words[:_lib.ROW_STATS_MOMENT_WORDS], dtype=np.int64).reshape(_lib.ROW_STATS_REPLICAS, 27, 2)
    return w[:, :, 0].sum(0) / 256.0 + w[:, :, 1].sum(0) / 1099511627776.0


def _check(sample, ref):
    got = sample.to_host()
    for k in ("coords", "counts", "npts", "row_start", "row_point", "feats"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    rows = ref["rows"].astype(np.float64)
    want = np.array([rows[:, j].sum() for j in range(6)] + [(rows[:, j] * rows[:, k]).sum() for j in range(6) for k in range(j, 6)])
    assert np.allclose(_decode_row_stats(sample.row_stats.cpu().numpy()), want, rtol=1e-12, atol=1e-9)
    return got


@pytest.mark.parametrize("T", [35, 1, 64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_equals_the_restatement(dtype, T):
    ref = _ref(dtype, T)
    assert sorted(ref["counts"]) == sorted(COUNTS) and len(COUNTS) % 4 != 0          # a block runs four waves
    got = _check(_vox(T)(_sweep().astype(dtype), draw=(ITEM, EPOCH)), ref)
    if T == 35:
        from oracle import voxel_ref
        first = voxel_ref.voxelize_ref(_sweep().astype(dtype).astype(np.float64), sampleSize=T, **GRID)
        big = ref["counts"] > T
        assert np.array_equal(got["feats"][~big], first["feats"][~big])
        assert all(not np.array_equal(got["point_index"][v], first["point_index"][v]) for v in np.nonzero(big)[0])


def test_empty_and_pad_only_sweeps():
    vox = _vox(35)
    for pts in (np.zeros((0, 3), np.float32), np.full((300, 3), 1.0e6, np.float64)):
        s = vox(pts, draw=(ITEM, EPOCH))
        assert s.host_info() == dict(V=0, rows=0, valid=0, max_count=0)
        assert (s.cell_voxel.cpu().numpy() == -1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_padding_behind_the_sweep_changes_nothing(dtype):
    """A fixed-capacity buffer (a recorded step's): the key goes by the row index, so the pad rows are not seen."""
    pts = _sweep().astype(dtype)
    padded = np.concatenate([pts, np.full((1777, 3), 1.0e6, dtype)])
    _check(_vox(35)(padded, draw=(ITEM, EPOCH)), _ref(dtype, 35))


def test_epochs_and_items_redraw_only_oversize_voxels():
    vox, pts = _vox(35), _sweep().copy()
    base = _check(vox(pts, draw=(ITEM, EPOCH)), _ref(np.float64, 35))
    again = vox(pts, draw=(ITEM, EPOCH)).to_host()
    assert all(np.array_equal(base[k], again[k]) for k in base)
    big = base["counts"] > 35
    for item, epoch in ((ITEM, EPOCH + 1), (ITEM + 1, EPOCH)):
        other = _check(vox(pts, draw=(item, epoch)), _ref(np.float64, 35, item, epoch))
        assert np.array_equal(other["feats"][~big], base["feats"][~big])
        assert all(not np.array_equal(other["point_index"][v], base["point_index"][v]) for v in np.nonzero(big)[0])
    # out= with draw=None reads the words as they are: the sample of the last call, drawn again with its own words
    s = vox(pts, draw=(ITEM, EPOCH))
    vox.set_draw(s, ITEM, EPOCH + 1)
    _check(vox(pts, out=s), _ref(np.float64, 35, ITEM, EPOCH + 1))
    # another seed through VFE_preprocessing: the same rule
    from lisec_amd.model_training import VFE_preprocessing
    sv = VFE_preprocessing(pts, 1.0, 1.0, 1.0, 35, 4, 4, 4, seed=SEED, item=ITEM, epoch=EPOCH)
    _check(sv.sample, _ref(np.float64, 35))


def test_equal_philox_words_fall_to_the_lower_index():
    """Two points with the same Philox word exactly at the cut: the low word of the key decides, in the shuffle ranking
    (a voxel of 46) and in the radix select, which has to go on into the index bytes (a voxel of 76).  Such pairs exist
    among 400 000 row indices (about 18 expected); the rows in between are pad rows."""
    n = 400_000
    w = S.philox_word0(SEED, ITEM, EPOCH, np.arange(n))
    order = np.argsort(w, kind="stable")
    at = np.nonzero(w[order][1:] == w[order][:-1])[0]
    at = [d for d in at if 1000 < d < n - 1000][:2]
    assert len(at) == 2
    rng = np.random.default_rng(8)
    pts = np.full((n, 3), 1.0e6)
    pairs = []
    for d, cell, above in zip(at, ((1.0, 1.0, 1.0), (-2.0, 2.0, 2.0)), (40, 10)):
        i, j = int(order[d]), int(order[d + 1])
        assert i < j and w[i] == w[j]
        below = rng.choice(order[:d], 34, replace=False)                      # 34 smaller words: the pair straddles the cut
        over = rng.choice(order[d + 2:], above, replace=False)
        rows = np.concatenate([below, [i, j], over])
        assert len(set(rows.tolist())) == 36 + above and (pts[rows, 0] == 1.0e6).all()
        pts[rows] = np.array(cell) + rng.uniform(0.1, 0.9, (len(rows), 3))
        pairs.append((i, j))
    ref = S.voxelize_draw_ref(pts, sampleSize=35, **GRID, seed=SEED, item=ITEM, epoch=EPOCH)
    assert sorted(ref["counts"]) == [46, 76]
    got = _check(_vox(35)(pts, draw=(ITEM, EPOCH)), ref)
    for i, j in pairs:
        assert i in got["row_point"] and j not in got["row_point"]


def _direct(lib, entry, cfg, pts, extra=()):
    """One call of a voxeliser entry of the C ABI on buffers of its own, all filled with a sentinel first."""
    import torch
    from lisec_amd import _lib
    n, cap, dev = pts.shape[0], min(pts.shape[0], 4 * 8 * 8), pts.device
    ws = torch.empty(lib.lisec_voxelize_workspace_bytes(ctypes.byref(cfg), n), dtype=torch.uint8, device=dev)
    sizes = dict(info=8, cell_voxel=4 * 8 * 8, coords=cap * 3, counts=cap, npts=cap, row_start=cap + 1, rows=n * 6, row_point=n)
    out = {k: torch.full((v,), -7, dtype=torch.float32 if k == "rows" else torch.int32, device=dev) for k, v in sizes.items()}
    out["row_stats"] = torch.full((_lib.ROW_STATS_WORDS,), -7, dtype=torch.int64, device=dev)
    rc = getattr(lib, entry)(ctypes.byref(cfg), _lib.ptr(pts), 0 if pts.dtype == torch.float32 else 1, n, 3, _lib.ptr(ws),
                             ws.numel(), cap, *(_lib.ptr(out[k]) for k in (*sizes, "row_stats")), *extra,
                             _lib.current_stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_default_path_is_lisec_voxelize():
    """subsample='first' through the new arguments: lisec_voxelize's output, bit for bit, and no draw words."""
    import torch
    from lisec_amd import _lib
    from lisec_amd.voxelizer import Voxelizer
    pts = torch.from_numpy(_sweep().copy()).cuda()
    vox = Voxelizer(sampleSize=35, **GRID, subsample="first", seed=SEED)
    s = vox(pts)
    assert s.draw is None
    rc, want = _direct(vox.lib, "lisec_voxelize", vox.cfg, pts)
    assert rc == 0
    V, R = int(want["info"][0]), int(want["info"][1])
    assert V == len(COUNTS)
    trim = dict(info=8, cell_voxel=256, coords=3 * V, counts=V, npts=V, row_start=V + 1, rows=6 * R, row_point=R,
                row_stats=_lib.ROW_STATS_WORDS)
    for k, m in trim.items():
        assert np.array_equal(getattr(s, k).cpu().numpy().reshape(-1)[:m], want[k][:m]), k
    from oracle import voxel_ref
    first = voxel_ref.voxelize_ref(_sweep(), sampleSize=35, **GRID)
    assert np.array_equal(s.to_host()["point_index"], first["point_index"])
    with pytest.raises(ValueError):
        vox(pts, draw=(0, 0))


def test_refusals_enqueue_nothing():
    import torch
    from lisec_amd import _lib, augment
    from lisec_amd.voxelizer import Voxelizer
    pts = torch.from_numpy(_sweep().copy()).cuda()
    vox = _vox(35)
    rc, out = _direct(vox.lib, "lisec_voxelize_draw", vox.cfg, pts, extra=(None,))
    assert rc == -1                                                         # LISEC_EINVAL
    assert b"draw" in vox.lib.lisec_last_error()
    assert all((v == -7).all() for v in out.values())                       # not one launch ran
    assert vox.lib.lisec_voxel_draw_set(None, 1, 2, 3, _lib.current_stream()) != 0
    with pytest.raises(ValueError):
        Voxelizer(sampleSize=35, **GRID, subsample="shuffle")
    with pytest.raises(ValueError):
        augment.AugmentedSweeps([], [], subsample="shuffle")
    first = Voxelizer(sampleSize=35, **GRID)(pts)
    with pytest.raises(ValueError):
        vox(pts, out=first)                                                 # a sample without draw words


# ---- Model.fit: the draw reaches the replayed step ------------------------------------------------------------------------
_FIT = r"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import augment_cases as C
from lisec_amd import Constants, _lib, augment
from lisec_amd import model_training as mt
from lisec_amd.network import PipelinedStep, RecordedStep
Constants.nx, Constants.ny = 16, 32                 # the (16, 32, 8) grid of the augmentation tests
pts, bxs = C.fit_sweeps()
rng = np.random.default_rng(5)
for i, b in enumerate(bxs):                          # crowded voxels: 90 and 400 points in 0.1 m cubes inside the first box
    c = np.array([b[0][0], b[0][1], 1.0])                # (a cube meets at most 8 voxels: one of them holds 50 or more)
    extra = np.concatenate([c + rng.uniform(-0.05, 0.05, (90, 3)), c + (0.6, 0.0, 0.3) + rng.uniform(-0.05, 0.05, (400, 3))])
    p = np.concatenate([pts[i], extra.astype(np.float32)])
    rng.shuffle(p)
    pts[i] = p


class Padded(augment.AugmentedSweeps):
    # seq[i], what the Python schedule voxelises, padded to the recorded step's capacity with rows the voxeliser drops: the
    # row-list kernels then take the K-slice plans, hence the summation order, of the recorded step (as the sweeps of
    # tests/test_gpu_optimizers._data are padded).  The recorded steps stage their items themselves and never ask for it.
    def __getitem__(self, i):
        p, y = super().__getitem__(i)
        out = torch.full((4096, 3), 1.0e6, dtype=p.dtype, device=p.device)
        out[:p.shape[0]] = p
        return out, y


def fit(tuning, subsample):
    os.environ["LISEC_TUNING"] = tuning
    np.random.seed(0)
    torch.manual_seed(0)
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    seq = Padded(pts, bxs, seed=11, subsample=subsample)
    if subsample == "random":
        for i in range(3):
            v = mt.VFE_preprocessing(seq[i][0], *m._sequence_grid(), seed=11, item=i, epoch=0).sample
            assert v.host_info()["max_count"] >= 50, v.host_info()
    m.fit(x=seq, batch_size=1, verbose=0, epochs=2, shuffle=False)
    torch.cuda.synchronize()
    assert seq.epoch == 2
    step = m._captured[1] if m._captured is not None else None
    assert step is None or step.capacity == 4096
    return m.net.params.theta.cpu().numpy().copy(), step


piped, step = fit("", "random")
assert type(step) is PipelinedStep and step.vox.subsample == "random"
words = [s.draw.cpu().numpy().tolist() for s in step.samples]
assert sorted(words) == [[11, 0, 1, 1], [11, 0, 2, 1]], words          # the last two items, epoch 1, one per buffer set
recorded, step = fit("pipeline_voxels=0", "random")
assert type(step) is RecordedStep
eager, step = fit("step_plan=0", "random")
assert step is None
first, step = fit("", "first")
assert step.vox.subsample == "first" and all(s.draw is None for s in step.samples)
assert np.array_equal(piped, recorded), np.abs(piped - recorded).max()
assert np.array_equal(piped, eager), np.abs(piped - eager).max()
assert not np.array_equal(piped, first)
print("FIT-OK")
"""


def test_fit_draws_alike_on_every_schedule(tmp_path):
    """Model.fit(x=AugmentedSweeps(subsample='random')), two epochs of three sweeps with crowded voxels: PipelinedStep,
    RecordedStep and the Python schedule end with bit-identical variables -- a draw frozen into a plan, or written to the
    other buffer set, would not -- and 'first' ends elsewhere.  A child process, as the schedules go by LISEC_TUNING."""
    script = tmp_path / "fit_subsample.py"
    script.write_text(_FIT)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("LISEC_TUNING", None)
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "FIT-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
