"""The 64 x 64 tile of the implicit-GEMM family (csrc/igemm.hip: k_igemm_small, LISEC_CONV_SMALL_TILE, lisec_tuning.small_tile)
on small maps, one contraction at a time through the C ABI.

What can break, and the case that shows it:
  * the wave -> (row half, column half) mapping, the row tail and tiles spanning several lines: 13 x 25 (M = 325 = 5 tiles +
    5 rows), Cin 64 / 96 (a partial channel slab), Cout 64 / 128, plain form;
  * the w-halo staging of a 64-row tile that crosses a line end, first and last line: 9 x 70 and 6 x 100, 128 -> 128;
  * the K slices' half-size slabs, their stride and the combine: force_splitk 1, 2, 3, 6, every call TWICE on the same
    workspace (the arrival counters must be back at zero);
  * the epilogue's statistics reduction over two row halves: forward sink (mode 0, BatchNormalization + ReLU on load) and
    backward sink with ACCUMULATE and an output gate (mode 1).
Bounds: output relative L2 <= 2e-6 against the fp64 definition oracle/conv_ref.py (the bound of the direct kernels,
tests/test_gpu_lyft_layers.py); sink results within the bounds of the sink checks there; and against the 128-row kernels
on the same inputs and K slices the output is BIT-IDENTICAL (each element's fmaf chain and the slice-order sum do not
depend on the tile height), and so are the statistics: the two 64-row tiles of a 128-row tile meet and send the sink the
one fp64 addend the 128-row tile sends (the issue allows rtol 1e-6; a training step only reproduces the 128-row step
bit for bit if they are equal).  12 x 25 (M = 300: five 64-row tiles) ends in a tile without a partner; the others pair up.
The planner's choice is asserted from lisec_conv_plan_query without launching."""
import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-6
SLICES = (1, 2, 3, 6)
K33, S1, P1 = (1, 3, 3), (1, 1, 1), (0, 1, 1)

# name, map (h, w), cin, cout
PLAIN = [(f"13x25 {ci}->{co}", (13, 25), ci, co) for ci in (64, 96) for co in (64, 128)] + [("12x25 64->64", (12, 25), 64, 64)]
HALO = [("9x70 128->128", (9, 70), 128, 128), ("6x100 128->128", (6, 100), 128, 128)]


@pytest.fixture(autouse=True)
def default_tuning():
    from lisec_amd import _lib
    prev = _lib.set_tuning(small_tile=1, force_splitk=0)
    yield
    _lib.set_tuning(**prev)


@functools.lru_cache(maxsize=None)
def problem(name, mode, hw, cin, cout):
    """Seeded inputs of one case and their fp64 results, computed once and shared by every K slicing (never modified)."""
    from oracle import conv_ref
    rng = np.random.default_rng(zlib.crc32(f"{name} mode {mode}".encode()))
    dims, M = (1, *hw), hw[0] * hw[1]
    x = rng.normal(0, 1, (*dims, cin)).astype(np.float32)
    Wt = (rng.normal(0, 1, (9, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    p = dict(dims=dims, M=M, x=x, Wt=Wt)
    if mode == 0:
        st = np.concatenate([rng.uniform(0.5, 1.5, cin), rng.normal(0, 0.3, cin), rng.normal(0, 0.2, cin),
                             rng.uniform(0.7, 1.4, cin)]).astype(np.float32)
        p["in_bn"] = st
        p["bias"] = rng.normal(0, 0.1, cout).astype(np.float32)
        p["gamma"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        p["beta"] = rng.normal(0, 0.2, cout).astype(np.float32)
        p["ref"] = conv_ref.conv_forward(x, Wt, dims, K33, S1, P1, mode=0, bias=p["bias"],
                                         in_bn=(st[:cin].astype(np.float64), st[cin:2 * cin].astype(np.float64)), relu=True)
    else:
        p["base"] = rng.normal(0, 1, (*dims, cout)).astype(np.float32)       # what ACCUMULATE adds onto
        p["gate"] = rng.normal(0, 1, (*dims, cout)).astype(np.float32)       # out_mask
        p["y"] = rng.normal(0, 1, (*dims, cout)).astype(np.float32)          # raw output of the layer below
        p["y_bn"] = np.concatenate([rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout), rng.normal(0, 0.2, cout),
                                    rng.uniform(0.7, 1.4, cout)]).astype(np.float32)
        conv = conv_ref.conv_forward(x, Wt, dims, K33, S1, P1, mode=1)
        p["ref"] = np.where(p["gate"].astype(np.float64).reshape(M, cout) > 0, p["base"].astype(np.float64).reshape(M, cout) + conv.reshape(M, cout), 0.0)
    return p


def run(p, mode, cin, cout, small, nslices):
    """One call as the training step issues it; returns (out, statistics the sink finalised, plan)."""
    from lisec_amd import _lib, ops
    dev = torch.device("cuda")
    _lib.set_tuning(small_tile=small, force_splitk=nslices)
    t = lambda a: torch.from_numpy(a).to(dev)
    g = ops.geom(mode, p["dims"], p["dims"], K33, S1, P1, cin, cout)
    wp = ops.pack_weights(t(p["Wt"]), 9, cin, cout, cin * cout, cout, 1)
    if mode == 0:
        bnstate = torch.zeros(4 * cout, device=dev)
        sink = ops.BnSink(cout, p["M"], dev, gamma=t(p["gamma"]), beta=t(p["beta"]), bnstate=bnstate)
        kw = dict(bias=t(p["bias"]), in_bn=t(p["in_bn"]), flags=ops.IN_RELU | ops.SMALL_TILE, sink=sink)
        plan = ops.conv_plan(g, in_bn=True, flags=kw["flags"], sink=sink)
    else:
        dgamma, dbeta = torch.zeros(cout, device=dev), torch.zeros(cout, device=dev)
        sink = ops.BnSink(cout, p["M"], dev, dgamma=dgamma, dbeta=dbeta)
        kw = dict(flags=ops.ACCUMULATE | ops.SMALL_TILE, out_mask=t(p["gate"]), bwd=(t(p["y"]), t(p["y_bn"]), True), sink=sink)
        plan = ops.conv_plan(g, flags=kw["flags"], out_mask=kw["out_mask"], bwd=kw["bwd"], sink=sink)
    results = []
    for rep in range(2):                                   # twice on the same workspace and sink: both come back to zero
        out = t(p["base"]).clone() if mode == 1 else torch.full((*p["dims"], cout), float("nan"), device=dev)
        ops.conv_forward(g, t(p["x"]), wp, out, **kw)
        torch.cuda.synchronize()
        stats = bnstate.cpu().numpy().copy() if mode == 0 else np.concatenate([dbeta.cpu().numpy(), dgamma.cpu().numpy(),
                                                                                 sink.coef.cpu().numpy()])
        results.append((out.cpu().numpy(), stats))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]), "second call differs"
    ws = ops._SPLITK_WS.get((str(dev), "main"))
    if ws is not None:
        assert int(ws[:4096 * 4].view(torch.int32).abs().sum().item()) == 0, "arrival counters not back at zero"
    return results[0][0], results[0][1], plan


def check_case(name, mode, hw, cin, cout, kernel):
    p = problem(name, mode, hw, cin, cout)
    M = p["M"]
    ref = p["ref"].reshape(M, cout)
    for ns in SLICES:
        out, stats, plan = run(p, mode, cin, cout, 1, ns)
        assert plan["tile_rows"] == 64 and plan["kernel"] == kernel and plan["k_slices"] == ns and plan["double_buffered"] == 1, plan
        assert plan["workgroups"] == -(-M // 64) * (cout // 64) * ns, plan
        got = out.reshape(M, cout).astype(np.float64)
        e = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        print(f"{name} mode {mode} slices {ns}: relative L2 {e:.3e}")
        assert e <= TOL, f"{name} mode {mode} slices {ns}: relative L2 {e:.2e}"
        st = stats.astype(np.float64)
        if mode == 0:
            mean, var = ref.mean(0), ref.var(0)
            inv = 1.0 / np.sqrt(var + 1e-3)
            gm, bt = p["gamma"].astype(np.float64), p["beta"].astype(np.float64)
            assert np.allclose(st[2 * cout:3 * cout], mean, rtol=0, atol=2e-6 * np.abs(ref).max()), "batch mean"
            assert np.allclose(st[3 * cout:], inv, rtol=2e-5), "inverse std"
            assert np.allclose(st[:cout], gm * inv, rtol=2e-5), "scale"
            assert np.allclose(st[cout:2 * cout], bt - mean * gm * inv, rtol=1e-4, atol=1e-5), "shift"
        else:
            yb = p["y_bn"].astype(np.float64)
            y64 = p["y"].astype(np.float64).reshape(M, cout)
            dz = np.where(y64 * yb[:cout] + yb[cout:2 * cout] > 0, ref, 0.0)
            yhat = (y64 - yb[2 * cout:3 * cout]) * yb[3 * cout:]
            db, dg = dz.sum(0), (dz * yhat).sum(0)
            tol_s = 3e-6 * np.sqrt(M) * np.abs(dz).max()
            assert np.abs(st[:cout] - db).max() <= tol_s and np.abs(st[cout:2 * cout] - dg).max() <= 3 * tol_s, "dbeta / dgamma"
            assert np.abs(st[2 * cout:3 * cout] - db / M).max() <= tol_s / M, "mean(dz)"
            assert np.abs(st[3 * cout:] - dg / M).max() <= 3 * tol_s / M, "mean(dz yhat)"
        # the 128-row kernels, same inputs, same K slices
        out128, stats128, plan128 = run(p, mode, cin, cout, 0, ns)
        assert plan128["tile_rows"] == 128 and plan128["k_slices"] == ns, plan128
        assert np.array_equal(out, out128), f"{name} mode {mode} slices {ns}: output differs from the 128-row kernel"
        assert np.array_equal(stats, stats128), f"{name} mode {mode} slices {ns}: statistics differ from the 128-row kernel"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_form(case, mode):
    check_case(*case[:1], mode, *case[1:], kernel="igemm")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", HALO, ids=[c[0] for c in HALO])
def test_halo_form(case, mode):
    check_case(*case[:1], mode, *case[1:], kernel="halo2")


def test_no_statistics_path():
    """Neither sink nor table: the epilogue's reduction is skipped altogether (the plain data gradient of dgrad_into)."""
    from lisec_amd import _lib, ops
    from oracle import conv_ref
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    dims, cin, cout = (1, 13, 25), 96, 128
    x = rng.normal(0, 1, (*dims, cin)).astype(np.float32)
    Wt = (rng.normal(0, 1, (9, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    g = ops.geom(1, dims, dims, K33, S1, P1, cin, cout)
    wp = ops.pack_weights(torch.from_numpy(Wt).to(dev), 9, cin, cout, cin * cout, cout, 1)
    ref = conv_ref.conv_forward(x, Wt, dims, K33, S1, P1, mode=1)
    outs = []
    for small in (1, 0):
        _lib.set_tuning(small_tile=small)
        assert ops.conv_plan(g, flags=ops.SMALL_TILE)["tile_rows"] == (64 if small else 128)
        out = torch.full((*dims, cout), float("nan"), device=dev)
        ops.conv_forward(g, torch.from_numpy(x).to(dev), wp, out, flags=ops.SMALL_TILE)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    e = float(np.linalg.norm(outs[0].astype(np.float64) - ref) / np.linalg.norm(ref))
    assert e <= TOL, f"relative L2 {e:.2e}"
    assert np.array_equal(outs[0], outs[1])


RPN = [("rpn2.conv1", (50, 100), 128, "halo2", 3, 3 * 158), ("rpn3.conv1", (25, 50), 256, "igemm", 6, 6 * 80)]


@pytest.mark.parametrize("case", RPN, ids=[c[0] for c in RPN])
def test_planner_picks_64_rows_for_the_small_rpn_maps(case):
    """The stride-1 layers of RPN blocks 2 and 3 at the Lyft maps, forward and data gradient as the training step issues
    them: 64-row tiles at the K slicing of the 128-row plan, two workgroups per CU.  Nothing is launched."""
    from lisec_amd import _lib, ops
    name, hw, ch, kernel, ns, wgs = case
    dev = torch.device("cuda")
    dims, M = (1, *hw), hw[0] * hw[1]
    z = lambda n: torch.zeros(n, device=dev)
    fsink = ops.BnSink(ch, M, dev, gamma=z(ch), beta=z(ch), bnstate=z(4 * ch))
    bsink = ops.BnSink(ch, M, dev, dgamma=z(ch), dbeta=z(ch))
    y = torch.zeros(*dims, ch, device=dev)
    calls = [(0, dict(in_bn=True, flags=ops.IN_RELU, sink=fsink)),
             (1, dict(bwd=(y, z(4 * ch), True), sink=bsink)),
             (1, dict(flags=ops.ACCUMULATE, bwd=(y, z(4 * ch), True), sink=bsink)),
             (1, dict())]
    for mode, kw in calls:
        g = ops.geom(mode, dims, dims, K33, S1, P1, ch, ch)
        base = ops.conv_plan(g, **kw)                       # the caller did not ask: the 128-row plan
        assert base["tile_rows"] == 128 and base["workgroups"] == 240 and base["k_slices"] == ns, base
        kw = dict(kw, flags=kw.get("flags", 0) | ops.SMALL_TILE)
        plan = ops.conv_plan(g, **kw)
        assert plan["tile_rows"] == 64 and plan["kernel"] == kernel and plan["cols"] == 64, plan
        assert plan["k_slices"] == ns == base["k_slices"] and plan["workgroups"] == wgs and plan["double_buffered"] == 1, plan
        assert plan["tiles"] == -(-M // 64) and plan["tail_tile0"] == 0 and plan["launches"] == 1, plan
        _lib.set_tuning(small_tile=0)
        assert ops.conv_plan(g, **kw) == base
        _lib.set_tuning(small_tile=1)


def test_planner_keeps_128_rows_where_the_small_kernel_does_not_serve():
    """Per-tile statistics table, row list, BatchNormalization backward on load, tail contraction, parity classes,
    pixel-shuffle store: asked for or not, these stay on 128-row tiles.  Nothing is launched."""
    from lisec_amd import ops
    dev = torch.device("cuda")
    z = lambda *n: torch.zeros(*n, device=dev)
    ST = ops.SMALL_TILE
    dims, ch = (1, 25, 50), 256
    g0 = ops.geom(0, dims, dims, K33, S1, P1, ch, ch)
    g1 = ops.geom(1, dims, dims, K33, S1, P1, ch, ch)
    assert ops.conv_plan(g0, flags=ST)["tile_rows"] == 64                                  # (the geometry is a candidate)
    table = ops.conv_plan(g0, in_bn=True, flags=ops.IN_RELU | ST, stats=True)
    assert table["tile_rows"] == 128 and table["workgroups"] == 240, table
    rows = ops.conv_plan(ops.geom(1, (1, 25, 50), (1, 25, 50), K33, S1, P1, ch, ch), flags=ST, rows_capacity=1250)
    assert rows["tile_rows"] == 128, rows
    fold = ops.conv_plan(g1, flags=ST, fold=(z(*dims, ch), z(4 * ch), z(2 * ch), True))
    assert fold["tile_rows"] == 128 and fold["workgroups"] == 240, fold
    tdims = (1, 10, 130)                                                                    # two-line halo geometry, 64 -> 64
    gt = ops.geom(1, tdims, tdims, K33, S1, P1, 64, 64)
    assert ops.conv_plan(gt, flags=ST)["tile_rows"] == 64
    bsink = ops.BnSink(64, 1300, dev, dgamma=z(64), dbeta=z(64))
    tail = ops.conv_plan(gt, flags=ST, out_mask=z(*tdims, 64), bwd=(z(*tdims, 64), z(256), False), sink=bsink,
                         tail=(z(4096), z(*tdims, 64)))
    assert tail["tile_rows"] == 128 and tail["kernel"] == "halo2", tail
    parity = ops.conv_plan(ops.geom(1, (1, 25, 50), (1, 50, 100), K33, (1, 2, 2), P1, 256, 128), flags=ST)
    assert parity["tile_rows"] == 128 and parity["parity_classes"] == 1, parity
    shuffle = ops.conv_plan(ops.geom(0, (1, 25, 50), (1, 25, 50), (1, 1, 1), S1, (0, 0, 0), 256, 1024, out_stride=768, ps=4,
                                     ps_channels=64), in_bn=True, flags=ops.IN_RELU | ST)
    assert shuffle["tile_rows"] == 128, shuffle
    odd = ops.conv_plan(ops.geom(0, dims, dims, K33, S1, P1, ch, 96), flags=ST)             # Cout not a multiple of 64
    assert odd["tile_rows"] == 128, odd
