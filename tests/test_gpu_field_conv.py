"""lisec_conv_field_forward (csrc/field_conv.hip: k_field_taps + k_field_combine) on its own, against the fp64 restatement
oracle/conv_ref.py over the materialised grid, and the sparse backward of the same layer as network.py::first_conv3d composes
it (csrc/sparse_grid.hip + the row-list contractions).  Inputs are written by hand (tests/field_cases.py): no voxeliser, no
VFE.  tests/test_field_cases.py shows on the host that the criteria below pass a correct fp32 evaluation of the decomposition
and fail one with a single dropped or misplaced (tap, voxel) term.

Criteria (none taken from the code under test):
  * integer operands: y BIT-EQUAL to the fp64 reference (every partial sum is an integer below 2^24);
  * normal operands: |y - ref| <= (n + 2) u A elementwise (glue_ref.sum_bound; n products, A their absolute sum) and relative
    L2 <= 2e-6 over the map -- the bound of the direct kernels, which ops.conv_forward on the materialised fp32 grid is held
    to in the same test;
  * y bit-identical across the launch shapes (field_tpw = 1 / KW, field_seg = default / 16 / 1024) and across two runs.
Every call: `out` starts as NaN (gap columns of a strided output as a sentinel), the workspace has exactly the queried size,
is filled with 0xff bytes (NaN) before each run -- a Z row that k_field_combine reads and k_field_taps skipped cannot pass --
and is followed by a guard tail; sink accumulators are zero after each run.

What reaches which branch (the layouts are asserted in tests/test_field_cases.py):
  tile skipping          G1 odd / even planes (whole tiles of one depth parity), G3 line (tiles 0-3: one line; kh = 2 and
                         kd = 0, 2 skip them), G4 (kw = 0, 2 skip every tile under field_tpw = 1), G1 random (m0 > V)
  the constant row       G1 V=128 / V=256 / full (alone in its tile), V=0 (the only row), V=cap (last addressable row),
                         overflow (info[NVOX] > cap)
  launch shapes          every case under field_tpw = 1 and KW; G1 / G2 under field_seg = 0 and 16 (segments of 14, 14, 12,
                         voxels at w = 13, 14, 27, 28), G3 under 0 (2 x 300) and 1024 (1 x 600: staging loop runs twice)
  contract geometries    G2 (valid depth), 2D and 1x1x1 kernels, strides along h and w, Wi = 1

Largest values seen on an MI355X (every test prints its own):
  integer operands       bit equality in every case, variant and launch shape; sparse backward (S, g_all, dW, rows) bit-equal
  normal operands        err/bound   relative L2     (the dense kernel on the same grid: relative L2 <= 2.99e-7)
    G1, ten layouts      0.0015      1.93e-7
    G1 no bias / stride  0.0014      1.56e-7
    G2                   0.0005      1.52e-7
    G3                   0.0008      1.72e-7
    G4 (Wi = 1)          0.0013      1.47e-7
    2D                   0.0019      1.37e-7
    1x1x1                0.0247      1.47e-7
    strides along h, w   0.0033      1.48e-7
  forward sink           batch mean of an exact sum: err / once_bound 0.458 (G1), 0.442 (G3)
No case failed, so csrc/field_conv.hip is unchanged.  Two wrong builds tried on a scratch copy: the depth test of the tile
skip taken with stride 1 fails 17 of the 44 tests here (NaN from Z rows nobody wrote: G1 random, V=256, odd planes, full,
faces and everything built on G1 random); a segment's staged span moved by one cell fails 30 (every case with voxels and more
than one segment: G1 and G2 under field_seg = 16, G3 under the default).  Dropping only the parity term of `feeds` makes
the tile skip rarer, not wrong: all 44 pass, as they should.
"""
import types

import numpy as np
import pytest
import torch

import field_cases as F
import glue_ref as R
import wgrad_edge_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = F.C
NAN = float("nan")
SENTINEL = -1234.5
HEAD_BYTES = 4096 * 4                # the arrival counters at the head of a weight-gradient workspace
TAIL_BYTES, TAIL_BYTE = 4096, 0xA5
IDS = [c["name"] for c in F.CASES]
KINDS = pytest.mark.parametrize("integer", [True, False], ids=["int", "normal"])

_REF = {}


def _reference(case, integer, with_bias=True):
    """(sweep, W, bias, ref, n, A) of a case, computed once and shared (read only)"""
    key = (case["name"], integer, with_bias)
    if key not in _REF:
        sw, W, bias = F.draw(case, integer)
        if not with_bias:
            bias = None
        _REF[key] = (sw, W, bias) + F.reference(sw, case["geom"], W, bias, bounds=True)
    return _REF[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _geom(geo, mode=0, out_stride=None):
    from lisec_amd import ops
    if mode == 0:
        return ops.geom(0, geo["ind"], geo["outd"], geo["k"], geo["s"], geo["p"], C, C, out_stride=out_stride)
    return ops.geom(1, geo["outd"], geo["ind"], geo["k"], geo["s"], geo["p"], C, C)


class _Call:
    """Device operands of one sweep and one kernel; run() is one guarded lisec_conv_field_forward."""

    def __init__(self, geo, sw, W, bias, out_stride=None):
        from lisec_amd import ops
        self.geo, self.sw, self.out_stride = geo, sw, out_stride or C
        self.g = _geom(geo, out_stride=out_stride)
        self.M = int(np.prod(geo["outd"]))
        self.sample = types.SimpleNamespace(info=_dev(sw.info), coords=_dev(sw.coords), cell_voxel=_dev(sw.cell_voxel),
                                            cap=sw.cap)
        self.vout, self.delta = _dev(sw.vout), _dev(sw.delta)
        self.W = _dev(W)
        taps = W.shape[0]
        self.wp = ops.pack_weights(self.W, taps, C, C, C * C, C, 1)
        self.bias = _dev(bias) if bias is not None else None
        self.nbytes = ops.conv_field_forward_workspace_bytes(self.g, sw.cap)
        assert self.nbytes > 0
        self.whole = torch.empty(self.nbytes + TAIL_BYTES, dtype=torch.uint8, device=DEV)

    def arm(self):
        self.whole[:self.nbytes] = 0xFF
        self.whole[self.nbytes:] = TAIL_BYTE
        out = torch.full((self.M, self.out_stride), NAN, device=DEV)
        out[:, C:] = SENTINEL
        return out

    def run(self, sink=None, what=""):
        """-> y (M, 64) on the host; the guards hold"""
        from lisec_amd import ops
        out = self.arm()
        ops.conv_field_forward(self.g, self.vout, self.delta, self.sample, self.wp, out, self.whole[:self.nbytes],
                               bias=self.bias, sink=sink)
        torch.cuda.synchronize()
        assert bool((self.whole[self.nbytes:] == TAIL_BYTE).all()), f"{what}: written behind the workspace"
        assert bool((out[:, C:] == SENTINEL).all()), f"{what}: gap columns of the strided output written"
        if sink is not None:
            assert int(sink.acc.abs().sum().item()) == 0, f"{what}: sink accumulators not back at zero"
        y = out[:, :C].cpu().numpy()
        assert np.isfinite(y).all(), f"{what}: {int((~np.isfinite(y)).sum())} output elements unwritten or NaN"
        return y

    def run_twice(self, knobs, what):
        with E.tuning(**knobs):
            a = self.run(what=what)
            b = self.run(what=what)
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: the second run differs from the first"
        return a


def _check(y, ref, n, A, integer, what):
    """the criterion of the operand kind; -> (err / bound, relative L2), printed"""
    ref2, y64 = ref.reshape(-1, C), y.astype(np.float64)
    if integer:
        bad = int((y64 != ref2).sum())
        print(f"{what}: integer operands, {bad} of {y.size} elements differ")
        assert bad == 0, f"{what}: {bad} elements differ from the exact result, max |diff| {np.abs(y64 - ref2).max()}"
        return 0.0, 0.0
    ratio, l2 = F.criteria(y64, ref2, n.reshape(-1, 1), A.reshape(-1, C))
    print(f"{what}: max err/bound {ratio:.4f}, relative L2 {l2:.3e}")
    assert ratio <= 1.0, f"{what}: max err/bound {ratio:.3f}"
    assert l2 <= F.TOL_L2, f"{what}: relative L2 {l2:.2e}"
    return ratio, l2


def _dense(call, sw, geo):
    """ops.conv_forward over the materialised fp32 grid"""
    from lisec_amd import ops
    grid = _dev(sw.grid.astype(np.float32))
    out = torch.full((call.M, C), NAN, device=DEV)
    ops.conv_forward(_geom(geo), grid, call.wp, out, bias=call.bias)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
@KINDS
def test_field_forward(case, integer):
    """Every case of tests/field_cases.py under every launch shape listed for it: the criterion of the operand kind, the
    same bits for every shape, and (normal operands) the dense kernel on the materialised grid within the same 2e-6."""
    geo = case["geom"]
    sw, W, bias, ref, n, A = _reference(case, integer)
    call = _Call(geo, sw, W, bias)
    first, worst = None, (0.0, 0.0)
    for knobs in case["knobs"]:
        what = f"{case['name']} {knobs}"
        y = call.run_twice(knobs, what)
        worst = tuple(max(a, b) for a, b in zip(worst, _check(y, ref, n, A, integer, what)))
        if first is None:
            first = y
        assert np.array_equal(_bits(y), _bits(first)), f"{what}: y differs from the first launch shape's"
    if not integer:
        l2 = F.rel_l2(_dense(call, sw, geo), ref)
        print(f"{case['name']}: dense kernel on the materialised grid, relative L2 {l2:.3e}")
        assert l2 <= F.TOL_L2
    print(f"{case['name']}: largest err/bound {worst[0]:.4f}, relative L2 {worst[1]:.3e}")


@KINDS
@pytest.mark.parametrize("variant", ["no bias", "out_stride 80"])
def test_field_forward_variants(variant, integer):
    """bias = NULL, and a strided output whose gap columns must keep their sentinel, on G1 random under all four shapes."""
    case = F.by_name("G1 random")
    sw, W, bias, ref, n, A = _reference(case, integer, with_bias=variant != "no bias")
    call = _Call(case["geom"], sw, W, bias, out_stride=80 if variant == "out_stride 80" else None)
    first = None
    for knobs in case["knobs"]:
        y = call.run_twice(knobs, f"{variant} {knobs}")
        _check(y, ref, n, A, integer, f"{variant} {knobs}")
        first = y if first is None else first
        assert np.array_equal(_bits(y), _bits(first))


@pytest.mark.parametrize("name", F.SINK_CASES)
@KINDS
def test_forward_sink(name, integer):
    """A LISEC_SINK_FORWARD sink with moving statistics: bnstate and the moving mean / variance against glue_ref.bn_finalize
    fed the fp64 (sum y, sum y^2) of the STORED output, at the tolerances tests/test_gpu_winograd.py::test_lyft_geometries
    (bnstate) and tests/test_gpu_network.py::test_field_conv_equals_dense_contraction (moving statistics) use.  A second call
    with the same sink gives the same bits and the same batch statistics; the moving statistics advance once more."""
    from lisec_amd import ops
    case = F.by_name(name)
    sw, W, bias, ref, n, A = _reference(case, integer)
    call = _Call(case["geom"], sw, W, bias)
    rng = np.random.default_rng(len(name) + integer)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
    mm, mv = _dev(rng.normal(0, 0.2, C).astype(np.float32)), _dev(rng.uniform(0.5, 1.5, C).astype(np.float32))
    bnstate = torch.full((4 * C,), NAN, device=DEV)
    sink = ops.BnSink(C, call.M, DEV, gamma=_dev(gamma), beta=_dev(beta), moving_mean=mm, moving_var=mv, unbiased=True,
                      bnstate=bnstate)
    plain = call.run_twice(case["knobs"][0], name)
    prev = None
    for knobs in (case["knobs"][0], case["knobs"][-1]):          # the statistics' partial sums depend on the segmentation
        for rep in range(2):
            what = f"{name} sink {knobs} call {rep}"
            mm0, mv0 = mm.cpu().numpy(), mv.cpu().numpy()
            with E.tuning(**knobs):
                y = call.run(sink=sink, what=what)
            assert np.array_equal(_bits(y), _bits(plain)), f"{what}: y differs from the call without a sink"
            _check(y, ref, n, A, integer, what)
            y64 = y.astype(np.float64)
            st_ref, mm_ref, mv_ref = R.bn_finalize(np.stack([y64.sum(0), (y64 * y64).sum(0)])[None], call.M, gamma, beta,
                                                   mm0, mv0, unbiased=True)
            st = bnstate.cpu().numpy().astype(np.float64)
            assert np.isfinite(st).all(), what
            part = lambda a, i: a[i * C:(i + 1) * C]
            np.testing.assert_allclose(part(st, 2), part(st_ref, 2), rtol=0, atol=2e-6 * np.abs(y64).max(), err_msg=what + " mean")
            np.testing.assert_allclose(part(st, 3), part(st_ref, 3), rtol=2e-5, atol=0, err_msg=what + " invstd")
            np.testing.assert_allclose(part(st, 0), part(st_ref, 0), rtol=2e-5, atol=0, err_msg=what + " scale")
            np.testing.assert_allclose(part(st, 1), part(st_ref, 1), rtol=1e-4, atol=1e-5, err_msg=what + " shift")
            if integer:                                        # the sum is exact: the mean is its fp64 value rounded once
                err = np.abs(part(st, 2) - part(st_ref, 2))
                print(f"{what}: batch mean, max err / once_bound {(err / R.once_bound(part(st_ref, 2))).max():.3f}")
                assert (err <= R.once_bound(part(st_ref, 2))).all(), what + " batch mean of an exact sum"
            for got, want, k in ((mm, mm_ref, "moving mean"), (mv, mv_ref, "moving variance")):
                np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-5, atol=2e-6 * max(1.0, np.abs(want).max()),
                                           err_msg=f"{what} {k}")
            if rep == 1:
                assert np.array_equal(_bits(bnstate.cpu().numpy()), prev), f"{what}: batch statistics differ from the first call's"
            prev = _bits(bnstate.cpu().numpy()).copy()


def test_refusals_launch_nothing():
    """mode 1, Cin = 32, KW = 4, a backward-kind sink: LISEC_EINVAL; a workspace one byte short: LISEC_ENOSPC.  `out` and
    the workspace keep the bytes they had."""
    from lisec_amd import _lib, ops
    case = F.by_name("G1 random")
    geo = case["geom"]
    sw, W, bias, *_ = _reference(case, True)
    call = _Call(geo, sw, W, bias)
    z = lambda k: torch.zeros(k, device=DEV)
    bwd_sink = ops.BnSink(C, call.M, DEV, gamma=z(C), beta=z(C), bnstate=z(4 * C), dgamma=z(C), dbeta=z(C))
    assert bwd_sink.desc.kind == 2
    k4 = dict(geo, k=(3, 3, 4), outd=(4, 6, 39))
    wp4 = torch.zeros(ops.packed_floats(36, C, C), device=DEV)
    room = 2 * call.nbytes                                     # enough for 36 taps: the refusal is not about space
    refused = [
        ("mode 1", _geom(geo, mode=1), call.wp, None, room, "error -1"),
        ("Cin 32", ops.geom(0, geo["ind"], geo["outd"], geo["k"], geo["s"], geo["p"], 32, C), call.wp, None, room, "error -1"),
        ("KW 4", ops.geom(0, k4["ind"], k4["outd"], k4["k"], k4["s"], k4["p"], C, C), wp4, None, room, "error -1"),
        ("backward sink", call.g, call.wp, bwd_sink, room, "error -1"),
        ("workspace one byte short", call.g, call.wp, None, call.nbytes - 1, "error -2"),
    ]
    ws = torch.empty(room, dtype=torch.uint8, device=DEV)
    for what, g, wp, sink, nbytes, code in refused:
        ws.fill_(0xFF)
        out = torch.full((call.M, C), NAN, device=DEV)
        with pytest.raises(_lib.LisecError, match=code):
            ops.conv_field_forward(g, call.vout, call.delta, call.sample, wp, out, ws[:nbytes], bias=call.bias, sink=sink)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), f"{what}: out was written"
        assert bool((ws == 0xFF).all()), f"{what}: the workspace was written"
    # the same operands are accepted once nothing is wrong with the call
    y = call.run_twice(case["knobs"][0], "accepted")
    assert np.array_equal(y.astype(np.float64), _reference(case, True)[3].reshape(-1, C))


@pytest.mark.parametrize("name", F.BACKWARD_CASES)
def test_sparse_backward_as_first_conv3d_composes_it(name):
    """The four calls of network.py::first_conv3d without the BatchNormalization apply -- tap sums, g_all, the row-list
    weight gradient + the constant's share, the row-list data gradient -- with integer operands against the dense definition
    on the materialised grid: bit equality (every sum stays below 2^24, tests/test_field_cases.py).  Rows of dout_rows at
    or above V keep their sentinel; the queue words and the arrival counters are zero afterwards.  Run twice."""
    from lisec_amd import ops
    case = F.by_name(name)
    geo = case["geom"]
    sw, W, _ = F.draw(case, True)
    dy = F.draw_dy(case, geo)
    ref = F.backward_reference(sw, geo, W, dy)
    assert ref["largest"] < F.EXACT
    taps, V, cap = W.shape[0], sw.V, sw.cap
    g, dg = _geom(geo), _geom(geo, mode=1)
    rcap = max(cap, 1)
    info, coords = _dev(sw.info), _dev(sw.coords)
    rows = (coords, info, rcap)
    Wd, dyd, delta, vout = _dev(W), _dev(dy), _dev(sw.delta), _dev(sw.vout)
    packed_t = ops.pack_weights(Wd, taps, C, C, C * C, 1, C)            # transposed: K = Cout, N = Cin
    tap_ws = torch.empty(ops.tap_sums_workspace_bytes(g), dtype=torch.uint8, device=DEV)
    nbytes = ops.wgrad_workspace_bytes(dg, rcap)
    head = min(HEAD_BYTES, nbytes)
    whole = torch.zeros(nbytes + TAIL_BYTES, dtype=torch.uint8, device=DEV)
    whole[head:nbytes] = 0xFF
    whole[nbytes:] = TAIL_BYTE
    queue = torch.zeros(2, dtype=torch.int32, device=DEV)
    n = taps * C * C
    for rep in range(2):
        tap_ws.fill_(0xFF)
        S = torch.full((taps * C,), NAN, device=DEV)
        g_all = torch.full((C,), NAN, device=DEV)
        dW_all = torch.full((n + C * C,), NAN, device=DEV)
        dW = dW_all[:n].view(taps, C, C)
        dout = torch.full((cap + 1, C), SENTINEL, device=DEV)
        ops.tap_sums(g, dyd, S, tap_ws)
        ops.const_field_grads(Wd, S, None, taps, C, C, g_all=g_all)
        ops.conv_wgrad(dg, dyd, delta, dW, whole[:nbytes], transpose_out=True, rows=rows)
        ops.const_field_grads(None, S, vout, taps, C, C, dW=dW, cvec_row=info, cvec_row_max=cap)
        ops.conv_forward(dg, dyd, packed_t, dout, rows=rows, queue=queue)
        torch.cuda.synchronize()
        what = f"{name} run {rep}"
        assert np.array_equal(S.cpu().numpy().reshape(taps, C).astype(np.float64), ref["S"]), f"{what}: tap sums"
        assert np.array_equal(g_all.cpu().numpy().astype(np.float64), ref["g_all"]), f"{what}: g_all"
        got = dW_all.cpu().numpy()
        assert np.isnan(got[n:]).all(), f"{what}: written behind the weight gradient"
        bad = int((got[:n].reshape(taps, C, C).astype(np.float64) != ref["dW"]).sum())
        assert bad == 0, f"{what}: {bad} weight-gradient elements differ from the dense definition"
        rows_got = dout.cpu().numpy()
        bad = int((rows_got[:V].astype(np.float64) != ref["rows"]).sum())
        assert bad == 0, f"{what}: {bad} elements of the grid gradient at the occupied cells differ"
        assert np.array_equal(_bits(rows_got[V:]), _bits(np.full((cap + 1 - V, C), SENTINEL, np.float32))), f"{what}: rows >= V written"
        assert bool((whole[nbytes:] == TAIL_BYTE).all()), f"{what}: written behind the weight-gradient workspace"
        assert int(whole[:head].view(torch.int32).abs().sum().item()) == 0, f"{what}: arrival counters not back at zero"
        assert int(queue.abs().sum().item()) == 0, f"{what}: queue words not back at zero"
    print(f"{name}: V = {V}, largest sum of absolute values {ref['largest']:.0f} < 2^24")
