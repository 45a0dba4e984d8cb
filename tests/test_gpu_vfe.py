"""HIP sparse-exact VFE (C ABI) vs the dense torch oracle (small grid) and the fp64 sparse oracle
(full Lyft grid).  Tolerance: rtol 1e-3 with atol 1e-3*max|ref| (BASELINE north_star); observed
errors are ~1e-6 because both sides are fp32 with fp64 statistics."""
import zlib

import numpy as np
import pytest
import torch

from conftest import LYFT
from test_gpu_lyft_layers import rel_l2    # relative L2, reported next to the per-layer errors

pytestmark = pytest.mark.gpu


def _oracle_params(seed):
    from oracle import model_ref as M
    return M.glorot_params(seed=seed, randomize_bn=True)


def _close(got, ref, rtol=1e-3):
    ref = np.asarray(ref, dtype=np.float64)
    atol = 1e-3 * np.abs(ref).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"max err {err.max():.3e} (atol {atol:.3e})"
    return err.max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("training", [True, False])
def test_vfe_small_grid_vs_dense_oracle(training):
    from lisec_amd.params import ParamStore
    from lisec_amd.vfe import VFEStack
    from lisec_amd.voxelizer import Voxelizer
    from oracle import model_ref as M
    from oracle import voxel_ref

    cfg = dict(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)
    rng = np.random.default_rng(1)
    n = 3000       # dense enough that several voxels hold > 35 points and many are full
    pts = np.stack([rng.uniform(-4.2, 4.2, n), rng.uniform(-4.2, 4.2, n), rng.uniform(0.0, 2.1, n)], 1)
    pts[:600, :2] *= 0.1
    pts[:600, 2] = 0.5 + 0.5 * rng.uniform(0, 1, 600)
    pts = pts.astype(np.float32)
    op = _oracle_params(5)
    dev = torch.device("cuda")
    store = ParamStore(dev, init=op)
    sample = Voxelizer(**cfg)(pts)
    grid = VFEStack(store).forward(sample, training=training).cpu().numpy()

    ref_vox = voxel_ref.voxelize_ref(pts.astype(np.float64), **cfg)
    assert ref_vox["counts"].max() > 35
    dense = torch.from_numpy(voxel_ref.to_dense(ref_vox, (8, 16, 32, 35, 6)))[None]
    p64 = {k: v.double() for k, v in op.items()}
    stats = {}
    h = M._vfe(dense.double(), p64, "vfe1", training, stats)
    h = M._vfe(h, p64, "vfe2", training, stats)
    h = M._fcn(h, p64, "fcn", training, stats)
    ref = h.max(dim=-2).values[0].numpy()
    rel = _close(grid, ref)
    assert rel < 1e-4
    if training:
        new = M.updated_moving_stats(p64, stats)
        got = store.to_dict()
        for k, v in new.items():
            _close(got[k], v.numpy(), rtol=1e-5)


def test_vfe_full_lyft_grid_vs_sparse_oracle():
    from lisec_amd.params import ParamStore
    from lisec_amd.vfe import VFEStack
    from lisec_amd.voxelizer import Voxelizer
    from oracle import vfe_sparse_ref as S
    from oracle import voxel_ref

    rng = np.random.default_rng(0)
    n = 20000
    pts = np.stack([rng.uniform(-55, 55, n), rng.uniform(-55, 55, n), rng.uniform(-0.5, 2.5, n)], 1).astype(np.float32)
    op = _oracle_params(9)
    store = ParamStore(torch.device("cuda"), init=op)
    sample = Voxelizer(**LYFT)(pts)
    grid = VFEStack(store).forward(sample, training=True)
    torch.cuda.synchronize()
    ref_vox = voxel_ref.voxelize_ref(pts.astype(np.float64), **LYFT)
    ncells = 8 * 200 * 400
    x, w, vox, seg = S.build_rows(ref_vox["feats"], ref_vox["npts"], 35, ncells)
    pn = {k: v.double().numpy() for k, v in op.items()}
    out, _ = S.forward(pn, x, w, vox, seg, N=float(ncells * 35), training=True)
    g = grid.cpu().numpy().reshape(ncells, 64)
    c = ref_vox["coords"]
    cells = (c[:, 0] * 200 + c[:, 1]) * 400 + c[:, 2]
    _close(g[cells], out[:-1])
    empty = np.ones(ncells, bool)
    empty[cells] = False
    # every empty cell holds the same (non-zero) constant
    const = g[empty][0]
    assert (g[empty] == const[None, :]).all()
    _close(const, out[-1])
    assert np.abs(const).max() > 0


@pytest.mark.parametrize("path", ["tiled", "valu"])
@pytest.mark.parametrize("grid", ["small", "lyft"])
def test_vfe_backward_vs_sparse_oracle(grid, path):
    """Gradients of the VFE variables from a random grid gradient, vs the fp64 row-class oracle
    (itself proven equal to dense torch autograd in tests/test_oracle_model.py).  Both backward paths: layers 3 and 2
    on 32-row MFMA tiles with the forward's saved winner slots (the default), and row by row per voxel."""
    from lisec_amd.params import ParamStore
    from lisec_amd.vfe import VFEStack
    from lisec_amd.voxelizer import Voxelizer
    from oracle import vfe_sparse_ref as S
    from oracle import voxel_ref

    rng = np.random.default_rng(4)
    if grid == "small":
        cfg = dict(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)
        n = 3000
        pts = np.stack([rng.uniform(-4.2, 4.2, n), rng.uniform(-4.2, 4.2, n), rng.uniform(0.0, 2.1, n)], 1)
        pts[:600, :2] *= 0.1
        pts[:600, 2] = 0.5 + 0.5 * rng.uniform(0, 1, 600)
    else:
        cfg = LYFT
        n = 20000
        pts = np.stack([rng.uniform(-55, 55, n), rng.uniform(-55, 55, n), rng.uniform(-0.5, 2.5, n)], 1)
    pts = pts.astype(np.float32)
    D, H, W = cfg["maxVoxelZ"], 2 * cfg["maxVoxelX"], 2 * cfg["maxVoxelY"]
    ncells = D * H * W
    op = _oracle_params(13)
    dev = torch.device("cuda")
    store = ParamStore(dev, init=op)
    vfe = VFEStack(store)
    vfe.tiled, vfe.tiled_min_points = path == "tiled", 0
    sample = Voxelizer(**cfg)(pts)
    vfe.forward(sample, training=True)
    dgrid = torch.randn(D, H, W, 64, device=dev) * (1.0 / ncells) ** 0.5
    grad = torch.zeros_like(store.theta)
    vfe.backward(dgrid, grad)
    torch.cuda.synchronize()

    ref_vox = voxel_ref.voxelize_ref(pts.astype(np.float64), **cfg)
    x, w, vox, seg = S.build_rows(ref_vox["feats"], ref_vox["npts"], 35, ncells)
    pn = {k: v.double().numpy() for k, v in op.items()}
    _, cache = S.forward(pn, x, w, vox, seg, N=float(ncells * 35), training=True)
    dg = dgrid.cpu().numpy().astype(np.float64).reshape(ncells, 64)
    c = ref_vox["coords"]
    cells = (c[:, 0] * H + c[:, 1]) * W + c[:, 2]
    empty = np.ones(ncells, bool)
    empty[cells] = False
    dout = np.concatenate([dg[cells], dg[empty].sum(0, keepdims=True)])
    ref = S.backward(pn, cache, dout)
    for name, r in ref.items():
        got = store.grad_view(grad, name).cpu().numpy()
        _close(got, r, rtol=2e-3)


def _decode_row_stats(words):
    """int64 row_stats -> the 27 moments (sum over replicas of hi * 2^-8 + lo * 2^-40)."""
    from lisec_amd import _lib
    w = np.asarray(words[:_lib.ROW_STATS_MOMENT_WORDS], dtype=np.int64).reshape(_lib.ROW_STATS_REPLICAS, 27, 2)
    return w[:, :, 0].sum(0) / 256.0 + w[:, :, 1].sum(0) / 1099511627776.0


def test_voxeliser_row_moments_and_vfe_without_them():
    """lisec_voxelize's side output row_stats: the 6 first and 21 second moments of the feature rows it wrote (what
    the closed-form statistics of the VFE's first BatchNormalization are made of), and the scratch behind them left
    zeroed by a training forward.  A caller without row_stats (NULL) gets the same grid: lisec_vfe_forward then sums
    the moments itself."""
    from lisec_amd import _lib
    from lisec_amd.params import ParamStore
    from lisec_amd.vfe import VFEStack
    from lisec_amd.voxelizer import Voxelizer, host_row_stats
    rng = np.random.default_rng(11)
    n = 20000
    pts = np.stack([rng.uniform(-55, 55, n), rng.uniform(-55, 55, n), rng.uniform(-0.5, 2.5, n)], 1).astype(np.float32)
    sample = Voxelizer(**LYFT)(pts)
    h = sample.to_host()
    rows = h["rows"].astype(np.float64)
    want = np.array([rows[:, j].sum() for j in range(6)] +
                    [(rows[:, j] * rows[:, k]).sum() for j in range(6) for k in range(j, 6)])
    got = _decode_row_stats(sample.row_stats.cpu().numpy())
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert np.allclose(_decode_row_stats(host_row_stats(h["rows"])), want, rtol=1e-12, atol=1e-9)
    assert (sample.row_stats.cpu().numpy()[_lib.ROW_STATS_MOMENT_WORDS:] == 0).all()
    op = _oracle_params(9)
    dev = torch.device("cuda")
    a = VFEStack(ParamStore(dev, init=op))
    g1 = a.forward(sample, training=True).cpu().numpy()
    state1 = a.params.state.cpu().numpy().copy()
    assert (sample.row_stats.cpu().numpy()[_lib.ROW_STATS_MOMENT_WORDS:] == 0).all()        # scratch re-zeroed
    g1b = a.forward(sample, training=True).cpu().numpy()                                    # same sample again
    assert np.array_equal(g1, g1b)
    keep, sample.row_stats = sample.row_stats, None
    b = VFEStack(ParamStore(dev, init=op))
    g2 = b.forward(sample, training=True).cpu().numpy()
    sample.row_stats = keep
    assert np.allclose(g1, g2, rtol=1e-6, atol=1e-7)
    assert np.allclose(state1, b.params.state.cpu().numpy(), rtol=1e-6, atol=1e-9)      # moving statistics too


def _edge_cloud(name):
    """Lyft-grid clouds at the VFE's occupancy edges.  Voxels are 0.5 x 0.25 x 0.25 m; a point is in range for
    -49.5 <= x < 50, -49.75 <= y < 50, 0.25 <= z < 2 (oracle/voxel_ref.py).  Returns (points, {voxel key: count}) with
    the counts the designed voxels must have; the designed voxels sit at x > 0, the random background at x < -1."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))

    def box(kx, ky, kz, n):        # n points strictly inside the voxel of signed keys (kx, ky, kz)
        u = rng.uniform(0.05, 0.95, (n, 3))
        return np.stack([(kx + u[:, 0]) * 0.5, (ky + u[:, 1]) * 0.25, (kz + u[:, 2]) * 0.25], 1)

    def background(n):
        return np.stack([rng.uniform(-49, -1, n), rng.uniform(-49, 49, n), rng.uniform(0.3, 1.9, n)], 1)

    want = {}
    if name == "single_point":                         # V = 1
        parts, want = [box(10, 20, 3, 1)], {(10, 20, 3): 1}
    elif name == "35_and_36":                          # exactly full (no pad row) and one point beyond (subsampled)
        parts, want = [box(10, 20, 3, 35), box(12, -30, 5, 36), background(300)], {(10, 20, 3): 35, (12, -30, 5): 36}
    elif name == "over_64":                            # more points than a wave has lanes
        parts = [box(10, 20, 3, 64), box(12, -30, 5, 65), box(30, 100, 7, 100), box(60, -150, 1, 300), background(300)]
        want = {(10, 20, 3): 64, (12, -30, 5): 65, (30, 100, 7): 100, (60, -150, 1): 300}
    elif name == "duplicates":                         # bit-identical rows: tied maxima between real rows
        a = np.repeat(box(10, 20, 3, 1), 12, 0)        # one point 12 times
        b = np.repeat(box(14, 8, 4, 5), 4, 0)          # five points 4 times each
        c = np.repeat(box(20, -40, 6, 1), 50, 0)       # one point 50 times: 35 identical rows kept, no pad row
        d = np.repeat(box(22, 40, 2, 3), 12, 0)        # three points 12 times: the kept 35 hold 12 + 12 + 11 copies
        bg = background(300)
        parts = [a, b, c, d, bg, bg[:100]]             # and 100 background points twice
        want = {(10, 20, 3): 12, (14, 8, 4): 20, (20, -40, 6): 50, (22, 40, 2): 36}
    elif name == "faces_and_limits":
        # points on voxel faces (multiples of 0.5 / 0.25 and halves of them: exact in fp32): on three faces, on two, and on
        # the face shared with the voxel below
        k = np.stack([rng.integers(-99, 100, 400), rng.integers(-199, 200, 400), rng.integers(1, 8, 400)], 1)
        f = k * np.array([0.5, 0.25, 0.25])
        lo, hi = np.array([-49.5, -49.75, 0.25]), np.array([50.0, 50.0, 2.0])
        below_hi = np.nextafter(hi.astype(np.float32), np.float32(0)).astype(np.float64)
        below_lo = np.nextafter(lo.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
        lim = []
        for ax in range(3):                            # each limit on one axis, the others at a face inside the range
            for v in (lo[ax], below_hi[ax], hi[ax], below_lo[ax]):
                q = np.array([1.0, 2.0, 1.0])
                q[ax] = v
                lim.append(q)
        lim += [lo, below_hi, hi, below_lo, np.array([lo[0], below_hi[1], lo[2]]), np.array([below_hi[0], lo[1], below_hi[2]])]
        parts = [f, f + np.array([0.25, 0.0, 0.0]), f + np.array([0.0, 0.125, 0.0]), f - np.array([0.0, 0.0, 0.25]),
                 np.array(lim)]
    elif name == "one_voxel":                          # every point in one voxel
        parts, want = [box(0, 0, 4, 5000)], {(0, 0, 4): 5000}
    else:
        raise KeyError(name)
    return np.concatenate(parts).astype(np.float32), want


EDGE_CLOUDS = ["single_point", "35_and_36", "over_64", "duplicates", "faces_and_limits", "one_voxel"]
# relative L2 bounds of the edge cases, from the measurement in the test's docstring
EDGE_TOL_FWD, EDGE_TOL_BWD = 2e-6, 2e-5
# the BatchNormalization beta gradients of vfe1 / vfe2 when every real row sits in ONE voxel (ONE_VOXEL_CLOUDS)
EDGE_TOL_BWD_ONE_VOXEL_BETA = 5e-4
ONE_VOXEL_CLOUDS = ("single_point", "one_voxel")


@pytest.fixture(scope="module")
def edge_oracle():
    """fp64 sparse-oracle forward (training) of each edge cloud, computed once per cloud."""
    from oracle import vfe_sparse_ref as S
    from oracle import voxel_ref
    op = _oracle_params(17)
    pn = {k: v.double().numpy() for k, v in op.items()}
    ncells = 8 * 200 * 400
    cache = {}

    def get(name):
        if name not in cache:
            pts, want = _edge_cloud(name)
            ref_vox = voxel_ref.voxelize_ref(pts.astype(np.float64), **LYFT)
            x, w, vox, seg = S.build_rows(ref_vox["feats"], ref_vox["npts"], 35, ncells)
            out, c = S.forward(pn, x, w, vox, seg, N=float(ncells * 35), training=True)
            cache[name] = (pts, want, ref_vox, out, c)
        return cache[name]
    return op, pn, get


@pytest.mark.parametrize("form", ["compact", "grid"])
@pytest.mark.parametrize("path", ["tiled", "valu"])
@pytest.mark.parametrize("cloud", EDGE_CLOUDS)
def test_vfe_edge_occupancy_vs_sparse_oracle(edge_oracle, cloud, path, form):
    """The VFE at the Lyft grid on clouds at its occupancy edges (_edge_cloud): a single point, voxels with exactly 35
    and 36 points, voxels beyond 64 points, exact duplicate points (tied maxima between real rows), points on voxel
    faces and on the range limits, every point in one voxel.  Training forward -- the compact per-voxel outputs the
    field form of the first Conv3D reads, or the dense grid -- and the moving statistics; then the backward from a
    random gradient (compact rows + g_all, or the dense grid gradient) on both paths: the 32-row MFMA tiles
    (tiled_min_points = 0) and row by row.  All vs the fp64 sparse oracle, at the module's bounds, and in relative L2
    per tensor at the tighter bounds the measurement supports (one MI355X run of all 24 cases):
      * forward (per-voxel outputs and the empty-cell constant): worst 3.9e-7 (single_point), bound EDGE_TOL_FWD 2e-6;
      * every gradient, except the one below: worst 5.2e-6 (single_point, d vfe1.bn.gamma), bound EDGE_TOL_BWD 2e-5;
      * d vfe1.bn.beta and d vfe2.bn.beta when every real row sits in one voxel (ONE_VOXEL_CLOUDS): up to 1.8e-4 on the
        tiled path, 5e-5 row by row, bound EDGE_TOL_BWD_ONE_VOXEL_BETA 5e-4.  The fp64 gradient of several channels
        there is 0 up to rounding (3e-12 next to 27): what the voxel's rows give cancels against the ~2e7-weight empty
        row class.  The same sparse oracle evaluated with an fp32 forward lands at 1.75e-4 on one_voxel's d vfe2.bn.beta
        as well: the conditioning of the case, not an error of either path.  Every other case keeps its beta gradients
        within EDGE_TOL_BWD (worst 2.1e-6)."""
    from lisec_amd.params import ParamStore
    from lisec_amd.vfe import VFEStack
    from lisec_amd.voxelizer import Voxelizer
    from oracle import vfe_sparse_ref as S

    op, pn, get = edge_oracle
    pts, want, ref_vox, out, cache = get(cloud)
    D, H, W = 8, 200, 400
    ncells = D * H * W
    c = ref_vox["coords"]
    V = len(c)
    for (kx, ky, kz), n in want.items():           # the cloud holds the designed voxels
        hit = (c[:, 0] == kz) & (c[:, 1] == kx + 100) & (c[:, 2] == ky + 200)
        assert hit.sum() == 1 and ref_vox["counts"][hit][0] == n, (kx, ky, kz)
    dev = torch.device("cuda")
    store = ParamStore(dev, init=op)
    vfe = VFEStack(store)
    vfe.tiled, vfe.tiled_min_points = path == "tiled", 0
    sample = Voxelizer(**LYFT)(pts)
    h = sample.to_host()
    assert np.array_equal(h["coords"], c) and np.array_equal(h["npts"], ref_vox["npts"])
    assert np.array_equal(h["feats"], ref_vox["feats"])
    grid = vfe.forward(sample, training=True, dense=form == "grid")
    torch.cuda.synchronize()
    assert (vfe._saved_rows > 0) == (path == "tiled")
    case = f"{cloud} [{path}, {form}]"
    note = f"vfe edge {case}"
    if form == "grid":
        g = grid.cpu().numpy().reshape(ncells, 64)
        cells = (c[:, 0] * H + c[:, 1]) * W + c[:, 2]
        empty = np.ones(ncells, bool)
        empty[cells] = False
        assert (g[empty] == g[empty][0][None, :]).all()
        got_out = np.concatenate([g[cells], g[empty][:1]])
    else:
        got_out = vfe.saved_field("vout").cpu().numpy()[:V + 1]
    _close(got_out, out)
    assert rel_l2(got_out, out, f"{note} forward") <= EDGE_TOL_FWD
    st = store.to_dict()
    for n in ("vfe1", "vfe2", "fcn"):
        mm = pn[f"{n}.bn.moving_mean"] * 0.99 + cache[n]["mean"] * 0.01
        mv = pn[f"{n}.bn.moving_variance"] * 0.99 + cache[n]["var"] * 0.01
        _close(st[f"{n}.bn.moving_mean"], mm, rtol=1e-5)
        _close(st[f"{n}.bn.moving_variance"], mv, rtol=1e-5)

    grad = torch.zeros_like(store.theta)
    gen = torch.Generator(device=dev).manual_seed(zlib.crc32(case.encode()))
    if form == "grid":
        dgrid = torch.randn(D, H, W, 64, device=dev, generator=gen) * (1.0 / ncells) ** 0.5
        vfe.backward(dgrid, grad)
        dg = dgrid.cpu().numpy().astype(np.float64).reshape(ncells, 64)
        dout = np.concatenate([dg[cells], dg[empty].sum(0, keepdims=True)])
    else:
        rows = torch.full((sample.cap + 1, 64), float("nan"), device=dev)
        rows[:V] = torch.randn(V, 64, device=dev, generator=gen)
        g_all = torch.randn(64, device=dev, generator=gen) * 30.0
        vfe.backward(None, grad, dout_rows=rows, g_all=g_all)
        r64 = rows[:V].cpu().numpy().astype(np.float64)
        dout = np.concatenate([r64, g_all.cpu().numpy().astype(np.float64)[None] - r64.sum(0, keepdims=True)])
    torch.cuda.synchronize()
    ref = S.backward(pn, cache, dout)
    for name, r in ref.items():
        got = store.grad_view(grad, name).cpu().numpy()
        _close(got, r, rtol=2e-3)
        beta = cloud in ONE_VOXEL_CLOUDS and name in ("vfe1.bn.beta", "vfe2.bn.beta")
        assert rel_l2(got, r, f"{note} d {name}") <= (EDGE_TOL_BWD_ONE_VOXEL_BETA if beta else EDGE_TOL_BWD), name
