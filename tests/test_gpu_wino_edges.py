"""lisec_conv_forward_winograd, lisec_conv_wgrad_winograd and lisec_conv_pack_weights_winograd at the edge geometries of
tests/wino_edge_cases.py against fp64: oracle/conv_ref.py for the contraction, and the fp64 definitions of ACCUMULATE, the
gate, OUT_RELU (+ bias, + previous, gate, ReLU in that order), the tail product and the sink results that
tests/test_gpu_winograd.py and tests/test_gpu_lyft_layers.py spell out.  tests/test_wino_edge_cases.py asserts on the host
that every case has the launch structure it is listed for (interior and gated blocks, launches per tap count, zero-tap
launches, eight plane slots, column blocks, workgroup shares of the weight gradient).

Guards, in every call.  What the call must write completely starts as NaN; what it must leave alone starts as a sentinel and
is compared bit for bit afterwards: `out` and `tail_out` are views inside a larger tensor with one sentinel plane before and
behind and sentinel channels on both sides of a strided view; dW sits in front of one more tap-sized NaN block.  x, dy, the
gate and bwd_y have a NaN plane before and behind them in the same allocation (and NaN channels beside a strided view): a
read outside the tensor shows as NaN in the result.  The weight-gradient workspace has exactly the queried size, is filled
with 0xff bytes (NaN: a slab sum that reads a slab nobody wrote shows) and has a 4 KiB pattern tail behind it.  Every call
runs twice on the same buffers and sink: bit-identical results, sink.acc all zero after each call, the second call's
statistics equal to the first's and its moving statistics one step further.

Bounds (none comes from the code under test): relative L2 <= TOL = 2e-6 for out and tail_out, TOL_W = 3e-6 for the weight
gradient as a whole AND for every tap on its own; a tap whose reference is identically zero is exactly 0.0; an output plane
without a live depth tap is exactly the fp32 value of gate(bias + previous).  Sinks: batch mean atol 2e-6 max|y|, invstd and
scale rtol 2e-5, shift rtol 1e-4 + atol 1e-5, moving statistics 2^-23 |ref| + 1e-9 max(1, |ref|) (glue_ref.bn_finalize from
the moving statistics the call found); backward sums tol_s = 3e-6 sqrt(M) max|dz|, 3x for dgamma (4x with the tail), coef the
same divided by M.  Every case without a tail also runs through the direct form (ops.conv_forward, SMALL_TILE off) on the same
operands and guards: both forms within the same bounds of the same reference.

Largest error / bound seen on an MI355X, per entry point (printed by every test as `ratio <entry point>: ...`):
  forward out                      0.207
  data gradient out                0.185
  tail_out                         0.192
  forward sink                     0.458   (with moving statistics; 0.009 in the cases without them)
  backward sink                    0.065
  weight gradient, whole           0.137
  weight gradient, worst tap       0.170
  direct form (cross-check)        out 0.125, forward sink 0.428, backward sink 0.040
All 54 tests passed as the kernels stand: no case of the table showed a defect.

What each group would catch, by the line it pins (csrc/wino.hip unless said otherwise):
  * map ladder, both XF forms: `interior` (:230) with `16 by + 16 <= H` -- block (1, 1) of 32 x 32 would run ungated, its
    window row 32 is the clamped row 31 (real data; with BN on load and positive shifts nonzero even over zeros).  33 x 33 is
    the smallest map whose block (1, 1) takes the ungated loop next to gated neighbours; 2 x 2 .. 3 x 2 pin the clamp
    (:138-139), pmask (:120) and the store predicate (:478).
  * channels: `nok` (:424), the `full` test (:500), the sink's `ch < Cout` (:585), the U image index with nnb 4 and 32
    chunks per tap (:264, :324) and the chunk walk's wrap (:160).
  * strides: rg_off by in_stride (:140, NaN channels beside x), `mline` by out_stride against `yline` by Cout (:470-471),
    stores beside the payload channels (sentinels).
  * depth: the `kd < 4` loop (:103), the walk over a non-contiguous dmask (:161; KD 4 stride 2 in mode 1 reads taps 0 and 2),
    the launch loop down to `taps == 0` (:736; with `> 0` the dead planes stay NaN) and `nchunks == 0` (:155, :249), the
    eighth nibble of plane_list (:740), sink.total over all launches (:716).
  * statistics: positions outside the map or the column block kept out of the sums (:478-493), OUT_RELU ahead of them (:483),
    the gate on `dv` (:489), the finaliser's arithmetic and its zeroing of the accumulators (conv.h).
  * tail: zero rows of the tail's operand outside the map (:494-496), its store predicate (:535), the second 32 columns'
    sums (:557-571), the paths without bwd_y (:546) and without a sink.
  * weight gradient (csrc/wino_wgrad.hip): num_records of the plane descriptor and the column predicates (:137-149; a read
    one row over returns the NaN plane), the unit shares (:84, :116), the slab every workgroup stores even without a unit
    (:297) under a 0xff workspace, the dead-tap zeros (:332).
  * packing: the stride arguments and `flip` (:610-611), the zero padding (`k < K && n < N`)."""
import functools

import numpy as np
import pytest
import torch

import glue_ref as R
import wino_edge_cases as E
from test_gpu_lyft_layers import TOL, TOL_W, rel_l2

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -1234.5625
TAIL_BYTES, TAIL_BYTE = 4096, 0xA5
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A failed assertion lets the next case run; a device error ends the session: nothing more is started on that GPU."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further case is started: {e}", returncode=3)


def _dev():
    return torch.device("cuda")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(entry, value):
    print(f"ratio {entry}: {value:.3f}")
    return value


class Guarded:
    """A (planes, H, W, C) tensor as a view inside a larger allocation: one guard plane before and one behind, and with
    stride > C guard channels on both sides of the C payload channels (a multiple of four on the left: 16-byte alignment)."""

    def __init__(self, dims, C, stride=None, guard=NAN, data=None):
        planes, H, W = dims
        stride = stride or C
        off = (stride - C) // 2 // 4 * 4
        self.whole = torch.full((planes + 2, H, W, stride), guard, device=_dev())
        self.view = self.whole[1:-1, :, :, off:off + C]
        self.region = (slice(1, -1), slice(None), slice(None), slice(off, off + C))
        self.before = None
        if data is not None:
            self.set(data)

    def set(self, data):
        if isinstance(data, float):
            self.view.fill_(data)
        else:
            self.view.copy_(torch.from_numpy(data))

    def snapshot(self):
        self.before = self.whole.clone()

    def check(self, what):
        """everything outside the view holds the bits it held at the snapshot"""
        now, before = self.whole.clone(), self.before.clone()
        now[self.region] = 0
        before[self.region] = 0
        assert torch.equal(_bits(now), _bits(before)), f"{what}: written outside the tensor"

    def host(self):
        return self.view.cpu().numpy()


# ---- the fp64 definitions ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """Operands and fp64 results of a forward / data-gradient case, computed once and shared (never modified)."""
    from oracle import conv_ref
    c = E.fwd_by_name(name)
    o = E.draw_fwd(c)
    cin, cout = c["cin"], c["cout"]
    M = int(np.prod(c["outd"]))
    bn = (f64(o["in_bn"][:cin]), f64(o["in_bn"][cin:2 * cin])) if c["in_bn"] else None
    v = conv_ref.conv_forward(o["x"], o["W"], c["outd"], (c["kd"], 3, 3), (c["sd"], 1, 1), (c["pd"], 1, 1), mode=c["mode"],
                              bias=o.get("bias"), in_bn=bn, relu=bool(c["in_bn"])).reshape(*c["outd"], cout)
    if c["accumulate"]:
        v = v + f64(o["prev"])
    if c["gate"]:
        v = np.where(o["gate"] > 0, v, 0.0)
    if c["out_relu"]:
        v = np.maximum(v, 0.0)
    r = dict(o=o, out=v, M=M)
    z = v.reshape(M, cout)
    if c["tail"]:
        z = z @ f64(o["Wd"][0])
        r["tail"] = z.reshape(*c["outd"], 64)
    if c["sink"] == "bwd":
        C = z.shape[1]
        st = f64(o["y_bn"])
        y = f64(o["y"]).reshape(M, C)
        dz = np.where(y * st[:C] + st[C:2 * C] > 0, z, 0.0) if c["bwd_relu"] else z
        yhat = (y - st[2 * C:3 * C]) * st[3 * C:]
        r.update(db=dz.sum(0), dg=(dz * yhat).sum(0), tol_s=3e-6 * np.sqrt(M) * np.abs(dz).max())
    elif c["sink"]:
        r.update(sums=np.stack([z.sum(0), (z * z).sum(0)])[None], ymax=np.abs(z).max())
    # planes no depth tap reaches: gate(bias + previous) in fp32, exactly
    dead = {}
    for d, n in enumerate(E.structure(c)["live"]):
        if n == 0:
            e = np.zeros((*c["outd"][1:], cout), np.float32) + o.get("bias", np.float32(0))
            if c["accumulate"]:
                e = e + o["prev"][d]
            if c["gate"]:
                e = np.where(o["gate"][d] > 0, e, np.float32(0))
            if c["out_relu"]:
                e = np.maximum(e, np.float32(0))
            dead[d] = e.astype(np.float32)
    r["dead"] = dead
    return r


class _Call:
    """One lisec_conv_forward_winograd (or, direct=True, lisec_conv_forward) call of a case with every guard in place."""

    def __init__(self, c, r, direct=False):
        from lisec_amd import ops
        self.c, self.r, self.direct = c, r, direct
        o = r["o"]
        cin, cout, M = c["cin"], c["cout"], r["M"]
        taps = c["kd"] * 9
        self.g = E.geom_of(c)
        self.x = Guarded(c["ind"], cin, c["in_stride"], data=o["x"])
        self.out = Guarded(c["outd"], cout, c["out_stride"], guard=SENTINEL)
        self.kw = dict(flags=E.flags_of(c))
        if direct:
            self.w = ops.pack_weights(_t(o["W"]), taps, cin, cout, cin * cout, cout, 1)
        elif c["pack"] == "net":        # the forward layer's kernel (taps, cout, cin), read as LisecNet._pack_transposed reads it
            self.w = ops.pack_weights_winograd(_t(o["W"].transpose(0, 2, 1)), c["kd"], cin, cout, cin * cout, 1, cin, flip=True)
        else:
            self.w = ops.pack_weights_winograd(_t(o["W"]), c["kd"], cin, cout, cin * cout, cout, 1, flip=(c["mode"] == 1))
        if c["bias"]:
            self.kw["bias"] = _t(o["bias"])
        if c["in_bn"]:
            self.kw["in_bn"] = _t(o["in_bn"])
        self.guards = [("x", self.x), ("out", self.out)]
        if c["gate"]:
            self.gate = Guarded(c["outd"], cout, c["out_stride"], data=o["gate"])
            self.kw["out_mask"] = self.gate.view
            self.guards.append(("gate", self.gate))
        self.tail_out = None
        if c["tail"]:
            self.tail_out = Guarded(c["outd"], 64, guard=SENTINEL)
            self.kw["tail"] = (ops.pack_weights(_t(o["Wd"]), 1, 64, 64, 0, 64, 1), self.tail_out.view)
            self.guards.append(("tail_out", self.tail_out))
        self.written = {}                              # tensors the sink's finaliser must write completely
        self.sink = None
        if c["sink"] == "bwd":
            cy = 64 if c["tail"] else cout
            self.y = Guarded(c["outd"], cy, data=o["y"])
            self.guards.append(("bwd_y", self.y))
            self.kw["bwd"] = (self.y.view, _t(o["y_bn"]), c["bwd_relu"])
            self.written = dict(dgamma=torch.empty(cy, device=_dev()), dbeta=torch.empty(cy, device=_dev()))
            self.sink = ops.BnSink(cy, M, _dev(), dgamma=self.written["dgamma"], dbeta=self.written["dbeta"])
            self.written["coef"] = self.sink.coef
        elif c["sink"]:
            self.written = dict(bnstate=torch.empty(4 * cout, device=_dev()))
            self.moving = None
            if "moving" in c["sink"]:
                self.moving = (_t(o["moving_mean"]), _t(o["moving_var"]))
            mm, mv = self.moving or (None, None)
            self.sink = ops.BnSink(cout, M, _dev(), gamma=_t(o["gamma"]), beta=_t(o["beta"]), moving_mean=mm, moving_var=mv,
                                   unbiased=c["sink"].endswith("1"), bnstate=self.written["bnstate"])
        if self.sink is not None:
            self.kw["sink"] = self.sink

    def run(self, what):
        """arms the guards, calls, checks the guards; returns the host copies of everything the call wrote"""
        from lisec_amd import ops
        c, o = self.c, self.r["o"]
        self.out.set(o["prev"] if c["accumulate"] else NAN)
        if self.tail_out is not None:
            self.tail_out.set(NAN)
        for t in self.written.values():
            t.fill_(NAN)
        for _, gd in self.guards:
            gd.snapshot()
        got = {}
        if self.sink is not None and getattr(self, "moving", None):
            got["moving_before"] = tuple(m.cpu().numpy() for m in self.moving)
        if self.direct:
            ops.conv_forward(self.g, self.x.view, self.w, self.out.view, **self.kw)
        else:
            ops.conv_forward_winograd(self.g, self.x.view, self.w, self.out.view, **self.kw)
        torch.cuda.synchronize()
        for name, gd in self.guards:
            gd.check(f"{what}: {name}")
        got["out"] = self.out.host()
        if self.tail_out is not None:
            got["tail"] = self.tail_out.host()
        for k, t in self.written.items():
            got[k] = t.cpu().numpy()
        if self.sink is not None:
            assert int(self.sink.acc.abs().sum().item()) == 0, f"{what}: sink accumulators not back at zero"
            if getattr(self, "moving", None):
                got["moving"] = tuple(m.cpu().numpy() for m in self.moving)
        return got


def _within(got, ref, bound, what):
    """largest |got - ref| / bound, asserted <= 1 (a NaN fails)"""
    got = f64(got)
    assert np.isfinite(got).all(), f"{what}: not every element was written"
    worst = float((np.abs(got - ref) / bound).max())
    assert worst <= 1.0, f"{what}: err / bound {worst:.3f}"
    return worst


def check(c, r, got, what, exact_dead=True):
    """every result of one call against the fp64 definitions; returns {entry point: largest err / bound}"""
    cout, M = c["cout"], r["M"]
    ratios = {}
    assert np.isfinite(got["out"]).all(), f"{what}: {int((~np.isfinite(got['out'])).sum())} of {got['out'].size} outputs unwritten or NaN"
    e = rel_l2(got["out"], r["out"])
    assert e <= TOL, f"{what}: out relative L2 {e:.2e}"
    ratios["out"] = e / TOL
    if exact_dead:
        for d, want in r["dead"].items():
            assert np.array_equal(got["out"][d], want), f"{what}: plane {d} has no live tap and must be gate(bias + previous) exactly"
    if c["tail"]:
        assert np.isfinite(got["tail"]).all(), f"{what}: tail_out positions unwritten or NaN"
        e = rel_l2(got["tail"], r["tail"])
        assert e <= TOL, f"{what}: tail_out relative L2 {e:.2e}"
        ratios["tail"] = e / TOL
    if c["sink"] == "bwd":
        C = len(r["db"])
        k = 4 if c["tail"] else 3
        ts = r["tol_s"]
        ratios["bsink"] = max(_within(got["dbeta"], r["db"], ts, f"{what}: dbeta"),
                              _within(got["dgamma"], r["dg"], k * ts, f"{what}: dgamma"),
                              _within(got["coef"][:C], r["db"] / M, ts / M, f"{what}: coef (mean dz)"),
                              _within(got["coef"][C:], r["dg"] / M, k * ts / M, f"{what}: coef (mean dz yhat)"))
    elif c["sink"]:
        o = r["o"]
        mm0, mv0 = got.get("moving_before", (None, None))
        st, mm, mv = R.bn_finalize(r["sums"], M, o["gamma"], o["beta"], mm0, mv0, unbiased=c["sink"].endswith("1"))
        part = lambda a, i: f64(a[i * cout:(i + 1) * cout])
        gs = got["bnstate"]
        worst = max(_within(part(gs, 2), part(st, 2), 2e-6 * r["ymax"], f"{what}: batch mean"),
                    _within(part(gs, 3), part(st, 3), 2e-5 * np.abs(part(st, 3)), f"{what}: invstd"),
                    _within(part(gs, 0), part(st, 0), 2e-5 * np.abs(part(st, 0)), f"{what}: scale"),
                    _within(part(gs, 1), part(st, 1), 1e-4 * np.abs(part(st, 1)) + 1e-5, f"{what}: shift"))
        if mm0 is not None:
            bound = lambda ref: 2.0 ** -23 * np.abs(ref) + 1e-9 * np.maximum(1.0, np.abs(ref))
            worst = max(worst, _within(got["moving"][0], mm, bound(mm), f"{what}: moving mean"),
                        _within(got["moving"][1], mv, bound(mv), f"{what}: moving variance"))
        ratios["fsink"] = worst
    return ratios


@pytest.mark.parametrize("case", E.FWD, ids=[c["name"] for c in E.FWD])
def test_forward_edge(case):
    """One guarded lisec_conv_forward_winograd call per case of the table, twice, against fp64 -- see the module docstring --
    and the direct form on the same operands within the same bounds."""
    c = case
    r = reference(c["name"])
    call = _Call(c, r)
    first = call.run(f"{c['name']} call 0")
    ratios = check(c, r, first, f"{c['name']} call 0")
    second = call.run(f"{c['name']} call 1")
    for k in first:
        if k in ("moving", "moving_before"):
            continue
        assert np.array_equal(first[k].view(np.int32), second[k].view(np.int32)), f"{c['name']}: {k} of the second call differs"
    if "moving" in first:                              # the second call starts where the first one ended
        for a, b in zip(first["moving"], second["moving_before"]):
            assert np.array_equal(a, b)
    for k, v in check(c, r, second, f"{c['name']} call 1").items():
        ratios[k] = max(ratios[k], v)
    entry = "forward out" if c["mode"] == 0 else "data gradient out"
    _ratio(entry, ratios["out"])
    for k, label in (("tail", "tail_out"), ("fsink", "forward sink"), ("bsink", "backward sink")):
        if k in ratios:
            _ratio(label, ratios[k])
    if not c["tail"]:                                  # (the direct form carries a tail only in its two-line w-halo kernel)
        direct = _Call(c, r, direct=True)
        dr = check(c, r, direct.run(f"{c['name']} direct form"), f"{c['name']} direct form", exact_dead=False)
        _ratio("direct form out", dr["out"])
        for k, label in (("fsink", "direct form forward sink"), ("bsink", "direct form backward sink")):
            if k in dr:
                _ratio(label, dr[k])


# ---- weight gradient -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_reference(name):
    from oracle import conv_ref
    c = E.wgrad_by_name(name)
    x, dy = E.draw_wgrad(c)
    return x, dy, conv_ref.conv_wgrad(x, dy, c["outd"], (c["kd"], 3, 3), (c["sd"], 1, 1), (c["pd"], 1, 1), mode=0)


@pytest.mark.parametrize("case", E.WGRAD, ids=[c["name"] for c in E.WGRAD])
def test_weight_gradient_edge(case):
    """One guarded lisec_conv_wgrad_winograd call per case, twice on the same workspace, against fp64: the whole gradient and
    every tap on its own; taps that read no plane are exactly 0.0."""
    from lisec_amd import ops
    c = case
    name = c["name"]
    x, dy, ref = wgrad_reference(name)
    g = E.geom_of(c)
    ntaps = c["kd"] * 9
    xg, dyg = Guarded(c["ind"], 64, data=x), Guarded(c["outd"], 64, data=dy)
    n = ntaps * 4096
    dW_all = torch.empty(n + 4096, device=_dev())
    dW = dW_all[:n].view(ntaps, 64, 64)
    nbytes = ops.wgrad_winograd_workspace_bytes(g)
    whole = torch.full((nbytes + TAIL_BYTES,), 0xFF, dtype=torch.uint8, device=_dev())
    whole[nbytes:] = TAIL_BYTE
    results = []
    for rep in range(2):
        dW_all.fill_(NAN)
        xg.snapshot(), dyg.snapshot()
        ops.conv_wgrad_winograd(g, xg.view, dyg.view, dW, whole[:nbytes])
        torch.cuda.synchronize()
        xg.check(f"{name}: x"), dyg.check(f"{name}: dy")
        assert bool((whole[nbytes:] == TAIL_BYTE).all()), f"{name}: written behind the workspace"
        got = dW_all.cpu()
        assert not torch.isnan(got[:n]).any(), f"{name}: {int(torch.isnan(got[:n]).sum())} of {n} gradient elements not written (or NaN)"
        assert torch.isnan(got[n:]).all(), f"{name}: written behind the gradient"
        results.append(got[:n].view(ntaps, 64, 64).numpy().copy())
    assert np.array_equal(results[0].view(np.int32), results[1].view(np.int32)), f"{name}: the second run differs from the first"
    got = results[0]
    e = rel_l2(got, ref)
    worst, worst_tap, zero_taps = 0.0, -1, []
    for tap in range(ntaps):
        if not np.any(ref[tap]):
            assert not np.any(got[tap]), f"{name}: tap {tap} reads nothing and must be exactly 0.0, max |dW| {np.abs(got[tap]).max():.3e}"
            zero_taps.append(tap)
            continue
        et = rel_l2(got[tap], ref[tap])
        if et > worst:
            worst, worst_tap = et, tap
    dead_kd = [kd for kd in range(c["kd"]) if kd not in c["facts"]["live"]]
    assert set(zero_taps) >= {kd * 9 + t for kd in dead_kd for t in range(9)}, f"{name}: the reference of a dead tap is not zero"
    print(f"{name}: relative L2 {e:.3e}, worst tap {worst_tap}: {worst:.3e}, zero taps {zero_taps}")
    _ratio("weight gradient, whole", e / TOL_W)
    _ratio("weight gradient, worst tap", worst / TOL_W)
    assert e <= TOL_W, f"{name}: weight gradient relative L2 {e:.2e}"
    assert worst <= TOL_W, f"{name}: tap {worst_tap} relative L2 {worst:.2e}"


# ---- packing ---------------------------------------------------------------------------------------------------------------
def _pack(src, KD, K, N, strides, flip):
    """lisec_conv_pack_weights_winograd into a NaN image with a sentinel tail; returns the image's bits (tail checked)"""
    from lisec_amd import ops
    n = ops.winograd_packed_floats(KD, K, N)
    dst = torch.full((n + 64,), NAN, device=_dev())
    dst[n:] = SENTINEL
    ops.pack_weights_winograd(src, KD, K, N, *strides, flip=flip, out=dst[:n])
    torch.cuda.synchronize()
    assert bool((dst[n:] == SENTINEL).all()), "written behind the packed image"
    return dst[:n].cpu().numpy()


@pytest.mark.parametrize("shape", [(2, 48, 40), (4, 64, 64), (1, 16, 200)], ids=["KD2 48x40", "KD4 64x64", "KD1 16x200"])
def test_packing(shape):
    """The same logical kernel described K-major (tap stride K N, k stride N, n stride 1) and N-major (the transposed array:
    k stride 1, n stride K -- how LisecNet reads a forward kernel for its data gradient) packs to bit-identical images;
    flip = True equals packing the host-mirrored kernel; with K = 48, N = 40 (a partial column block) every float of the image
    is finite -- the padding is written, as zeros -- and nothing is written behind it.  Twice: the same bits.  The VALUES of the
    images are asserted by every case of test_forward_edge, which runs on them."""
    KD, K, N = shape
    rng = np.random.default_rng(E.seed_of(f"pack {shape}"))
    W = rng.normal(0, 1, (KD * 9, K, N)).astype(np.float32)
    mirrored = np.ascontiguousarray(W.reshape(KD, 3, 3, K, N)[:, ::-1, ::-1]).reshape(KD * 9, K, N)
    k_major, n_major = (K * N, N, 1), (K * N, 1, K)
    for flip in (False, True):
        a = _pack(_t(W), KD, K, N, k_major, flip)
        assert np.isfinite(a).all(), f"{int((~np.isfinite(a)).sum())} floats of the image were not written"
        assert np.any(a)
        assert np.array_equal(a.view(np.int32), _pack(_t(W), KD, K, N, k_major, flip).view(np.int32)), "second call differs"
        b = _pack(_t(W.transpose(0, 2, 1)), KD, K, N, n_major, flip)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"K-major and N-major images differ (flip={flip})"
        m = _pack(_t(mirrored), KD, K, N, k_major, not flip)
        assert np.array_equal(a.view(np.int32), m.view(np.int32)), "flip is not the mirrored kernel"
    if K % 8 == 0 and N % 64:                          # every float beyond column N is a zero
        assert np.count_nonzero(a) <= a.size * N // (-(-N // 64) * 64)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Argument errors are answered on the host: LisecError, `out` / dW / the sink keep the bits they had, and the stream goes
    on working (a valid call behind them gives the right answer)."""
    from lisec_amd import _lib, ops
    dev = _dev()
    c = E.fwd_by_name("tail 2x2 net")
    r = reference(c["name"])
    call = _Call(c, r)
    filled = lambda n, v=SENTINEL: torch.full((n,), v, device=dev)

    def refused(what, fn, *tensors):
        before = [t.clone() for t in tensors]
        with pytest.raises(_lib.LisecError):
            fn()
        torch.cuda.synchronize()
        for t, b in zip(tensors, before):
            assert torch.equal(_bits(t) if t.dtype == torch.float32 else t, _bits(b) if b.dtype == torch.float32 else b), what

    # Do = 9
    d9 = (9, 6, 10)
    g9 = ops.geom(0, d9, d9, (1, 3, 3), (1, 1, 1), (0, 1, 1), 16, 64)
    x9, out9, wu16 = torch.zeros(*d9, 16, device=dev), filled(9 * 60 * 64), torch.zeros(ops.winograd_packed_floats(1, 16, 64), device=dev)
    refused("Do = 9", lambda: ops.conv_forward_winograd(g9, x9, wu16, out9), out9)
    # `in` offset by 4 bytes, the kernel image offset by 8 bytes
    g1 = ops.geom(0, (1, 6, 10), (1, 6, 10), (1, 3, 3), (1, 1, 1), (0, 1, 1), 16, 64)
    x1, out1 = torch.zeros(60 * 16 + 4, device=dev), filled(60 * 64)
    wu_off = torch.zeros(wu16.numel() + 4, device=dev)
    refused("in offset by 4 bytes", lambda: ops.conv_forward_winograd(g1, x1[1:], wu16, out1), out1)
    refused("kernel image offset by 8 bytes", lambda: ops.conv_forward_winograd(g1, x1, wu_off[2:], out1), out1)
    # tail with ACCUMULATE (every other argument as in a call that is served)
    call.out.set(SENTINEL), call.tail_out.set(SENTINEL)
    sink_t = [call.sink.acc, call.sink.coef, call.written["dgamma"], call.written["dbeta"]]
    for t in sink_t[1:]:
        t.fill_(SENTINEL)
    kw = dict(call.kw, flags=ops.ACCUMULATE)
    refused("tail with ACCUMULATE", lambda: ops.conv_forward_winograd(call.g, call.x.view, call.w, call.out.view, **kw),
            call.out.whole, call.tail_out.whole, *sink_t)
    # a sink with n_rows = 0
    bnstate = filled(256)
    sink0 = ops.BnSink(64, 0, dev, gamma=torch.ones(64, device=dev), beta=torch.zeros(64, device=dev), bnstate=bnstate)
    refused("sink with n_rows = 0", lambda: ops.conv_forward_winograd(g1, x1, wu16, out1, sink=sink0), out1, bnstate, sink0.acc)
    # weight gradient: a workspace one byte short, dy misaligned
    gw = E.geom_of(E.wgrad_by_name("wgrad 2x2"))
    nbytes = ops.wgrad_winograd_workspace_bytes(gw)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    xw, dyw, dW = torch.zeros(4 * 64, device=dev), torch.zeros(4 * 64 + 4, device=dev), filled(9 * 4096)
    refused("workspace one byte short", lambda: ops.conv_wgrad_winograd(gw, xw, dyw, dW, ws[:nbytes - 1]), dW, ws)
    refused("dy misaligned", lambda: ops.conv_wgrad_winograd(gw, xw, dyw[1:], dW, ws), dW, ws)
    # the stream is usable: the served call gives the right answer
    check(c, r, call.run("after the refusals"), "after the refusals")
