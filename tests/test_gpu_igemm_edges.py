"""lisec_conv_forward_ex at the edge geometries of tests/igemm_edge_cases.py against fp64: oracle/conv_ref.py for the contraction,
and the fp64 definitions of + bias, + previous, gate, ReLU (in that order), the pixel-shuffle placement
(glue_ref.head_shuffle_index), the tail product, BatchNormalization backward on load as apply-then-contract, and the sink
results (glue_ref.bn_finalize and the formulas of tests/test_gpu_lyft_layers.py).  tests/test_igemm_edge_cases.py asserts on the
host that every case engages the plan it is listed for; every test here asserts it again on the device before it launches.

Guards, in every call.  What the call must fill starts as NaN (`out`, `tail_out`, a row list's rows below the count, the
statistics it finalises, the rows of a per-tile table that belong to a tile); what it must leave alone starts as a sentinel and
is compared bit for bit afterwards: a guard plane before and behind `out` / `tail_out`, guard channels on both sides of a
strided view (the other slices of a pixel-shuffle target among them), the rows at and above a row list's count, the table rows
behind the last tile.  x, in_y, bwd_y and the gate sit inside NaN planes and, where strided, NaN channels (`previous` is what
`out` holds before the call, inside out's sentinels); the row coordinates beyond the count and around the list lie one past
the map.  The kernels are packed over a 0xff-filled buffer and
the image is compared with a host repack, padding zeros included.  The K-slice workspace has exactly the queried size, slabs
0xff, counter head zero, and a 4 KiB pattern tail behind it.  Every call runs twice on the same buffers: outputs and statistics
bit-identical, arrival and pair counters zero, sink.acc zero, queue words zero, moving statistics one step further.

Bounds (none comes from the code under test).  Whole output: relative L2 <= TOL = 2e-6.  Every element:
|got - ref| <= 1.01 (taps cin + 4) 2^-24 A, the a-priori bound of a sum of n fp32 products in any order, A being the same fp64
contraction over |f(x)|, |W|, + |bias| + |previous| (the fold: |scale| (|g| + |m1| + |yhat| |m2|), 8 for 4; tail_out: the absolute
tile times |Wd|).  A gated-off element is exactly 0.0 and a plane without a live depth tap exactly the fp32 value of
gate(bias + previous).  Sinks and tables (summed over tiles): batch mean atol 2e-6 max|y|, invstd and scale rtol 2e-5, shift
rtol 1e-4 + atol 1e-5, moving statistics 2^-23 |ref| + 1e-9 max(1, |ref|); backward sums tol_s = 3e-6 sqrt(M) max|dz|, 3x for
dgamma (4x with the tail), coef the same divided by M -- the bounds of tests/test_gpu_wino_edges.py.  The Dense weight gradient
beside a dense64 data gradient: relative L2 <= TOL_W.  A row-list tile that holds no rows must leave its K-slice slabs as they
were (plan_conv: "workgroups past the device-side row count exit at once").

Largest error / bound seen on an MI355X, per entry point (printed by every test as `ratio <entry point>: ...`; the first
column is the element-wise bound, the second the relative L2 over TOL):
  forward out                      0.097    0.255
  data gradient out                0.031    0.258
  tail_out                         0.002    0.201
  row list                         0.002    0.257
  pixel shuffle                    0.029    0.074
  forward sink                     0.477    (with moving statistics)
  backward sink                    0.400
  forward table                    0.014
  backward table                   0.054
  dense_dw weight gradient         0.054    (relative L2 over TOL_W)
The element-wise figures are largest where the sums are short (4 channels x 4 live taps in "plain one row"); at 27 x 64 terms
they sit two orders of magnitude under the bound.  All 111 tests passed as the kernels stand: no case of the table showed a
defect, and csrc/ is unchanged.

What each group would catch, by the line it pins (csrc/igemm.hip unless said otherwise):
  * halo widths 64 .. 129, three-line cases: `a`, `nseg`, `nrows` (:559-562), the staging map `w_in` / `ok` (:571-578; with
    `w_in <= g.Wi` the halo column behind a line end holds the next line's first position -- under positive shifts and ReLU a
    positive value where the padding zero belongs: 49 cases fail), `segbits` (:579), `seg_ok` with `L < nlines` (:601),
    `seg_lane` and `aoff` (:679-680: row 127 of "halo3 W125 three lines" is the only row of a third segment), the slice bounds
    by whole A tiles (:686-687) and the fall-back to the plain kernel when there are more slices than A tiles (:1827).
  * half-N: `nB = g.Cout` of a half tile (:79; dropped, a workgroup stores bias-only values into its neighbour's 32 columns and
    adds them to the sums: 7 cases fail), no workgroup beyond Cout (:1856), the statistics index `half && q >= 2` (:222).
  * plain M129, one row, channel tails: `cok` and `tbits` for a slab beyond Cin (:334-336), the on-load constants read at
    `cs` beside it (:347-360), `nA < g.Cout` on bias, accumulate, gate and store (:100-101, :139-149), rows beyond M (:122).
  * plain 3D, dead planes: `tap_live` with `d_first != d_last` (:319), `dmask_first` (:297, :320), a tile all of whose taps
    are dead still stores gate(bias + previous) (:435 never entered, :469); on the halo kernels `group_live` / `settle` (:608-613,
    :691-698).
  * parity classes: `parity_decode` (conv.h:154-161), the wave's decode and its one-line wrap (:86-91, :126-127), `live_row`
    (:128; with `<=` the padding row of a class is stored into the guard plane behind `out`: all five parity cases fail), the
    live taps per class (:311-312), the refusals (:1429-1430, :1714).
  * plane pairs: the two tiles of a workgroup (:837-842), `plane_tiles` (:1764), bit-identical with pairing off.
  * whole rounds + sliced tail: `tile0` in the slab slot and the grid of the second launch (:464, :765, :1859-1864).
  * wide: `nseg` (:908), its staging map (:917-921), `seg_lane` (:1000), the two column halves' store and ONE sink arrival
    (:1059, :1804), the refusal of CoutP % 128 (:1650).
  * row lists and the queue: `row_limit` (conv.h:145-149), `m0 >= mlimit` (:260; with `>` the tile that starts AT the count runs
    and writes its slabs: "rows count 0" and "rows count 128" fail), rows at or above the count (conv.h:218, :122), the draw loop
    and the two counters left at zero (:507-521), bit-identical with one workgroup per tile.
  * dense64: the descriptor's `g.M * 256` bytes (:1112: the last tile holds two rows, the other 126 read zeros and their stores
    are dropped), `ok` in the sums (:1198), the rows of y beyond the layer in the weight gradient (:1173-1188), the threshold
    (:1816).
  * pixel shuffle: `ps_tap`, `ncA` and the placement (:81-83, :132-135) into one slice of a wider map.
  * tail: the zero rows of the tail's operand beyond M (:163-164), phase 1 / 2 of store_tile (:94-95, :777-807), the dead plane.
  * fold: `bn_fold` on load (tile_parts.h:26-30) with invalid pieces kept at zero (`ok`), constants beside a ragged slab.
  * epilogue families: bias, ACCUMULATE, gate, OUT_RELU in that order (:137-149), sums after the ReLU (:160) or gated by
    bwd_relu (:155-158), table rows by tile (:225), sink totals per plan (:1741, :1804, :1841, :1855).
Two of the one-line mutations tried leave every RESULT as it is and are caught through a side effect or not at all:
`m0 > mlimit` (:260) only runs an empty tile (caught by its slab), and `q <= g.pc_rows` in parity_decode (conv.h:160) only
un-prunes the loads of a padding row whose h lies outside the map (mask 0) and which store_tile never stores (:128).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import glue_ref as R
import igemm_edge_cases as E
from test_gpu_lyft_layers import TOL, TOL_W, rel_l2
from test_gpu_wino_edges import NAN, SENTINEL, TAIL_BYTE, TAIL_BYTES, Guarded, _bits, _dev, _ratio, _t, _within, f64
from test_gpu_wino_edges import stop_at_a_device_error          # noqa: F401  (autouse: a device error ends the session)

pytestmark = pytest.mark.gpu

HEAD_BYTES = 4096 * 4                # arrival and pair counters at the head of the K-slice workspace
SLAB_BYTES = 128 * 64 * 4            # one K slice's partial tile (splitk.h: kSlabF4 float4)
GAMMA = 1.01 * 2.0 ** -24
IDS = [c["name"] for c in E.CASES]


# ---- the fp64 definitions ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(key):
    """Operands and fp64 results of the case(s) whose operands are named `key`, computed once and shared (never modified):
    out and its absolute companion A, which elements the gate closes, the planes without a live tap, tail, sums."""
    from oracle import conv_ref
    c = E.by_name(key)
    o = E.draw(c)
    cin, cout = c["cin"], c["cout"]
    taps = int(np.prod(c["k"]))
    M = int(np.prod(c["outd"]))
    extra = 4
    if c["fold"]:
        st, y, gq, coef = f64(o["fold_bn"]), f64(o["fold_y"]), f64(o["x"]), f64(o["fold_coef"])
        scale, shift, mean, invstd = (st[i * cin:(i + 1) * cin] for i in range(4))
        dz = np.where(y * scale + shift > 0, gq, 0.0) if c["fold"] == "relu" else gq
        yhat = (y - mean) * invstd
        xf = scale * (dz - coef[:cin] - yhat * coef[cin:])             # what lisec_bn_backward_apply_coef writes
        xa = np.abs(scale) * (np.abs(dz) + np.abs(coef[:cin]) + np.abs(yhat) * np.abs(coef[cin:]))
        extra = 8
    else:
        bn = (f64(o["in_bn"][:cin]), f64(o["in_bn"][cin:2 * cin])) if c["in_bn"] else None
        xf = conv_ref.transform_input(o["x"], bn, c["in_relu"])
        xa = np.abs(xf)
    W = f64(o["W"])
    geo = (c["outd"], c["k"], c["s"], c["p"])
    v = conv_ref.conv_forward(xf, W, *geo, mode=c["mode"])
    A = conv_ref.conv_forward(xa, np.abs(W), *geo, mode=c["mode"])
    if c["rows"]:
        q = o["coords"][:c["rows"][1]]
        v, A = v[q[:, 0], q[:, 1], q[:, 2]][None, None], A[q[:, 0], q[:, 1], q[:, 2]][None, None]
    if c["bias"]:
        b = np.tile(f64(o["bias"]), cout // len(o["bias"]))            # pixel shuffle: one bias per channel, whatever the tap
        v, A = v + b, A + np.abs(b)
    if c["ps"]:
        Do, Ho, Wo = c["outd"]
        pos, tap = R.head_shuffle_index(Ho * c["ps"], Wo * c["ps"], c["ps"])
        place = lambda a: a.reshape(Ho * Wo, c["ps"] ** 2, c["ps_channels"])[pos, tap].reshape(1, Ho * c["ps"], Wo * c["ps"], -1)
        v, A = place(v), place(A)
    if c["accumulate"]:
        v, A = v + f64(o["prev"]), A + np.abs(f64(o["prev"]))
    closed = np.zeros(v.shape, bool)
    if c["gate"]:
        closed = ~(o["gate"] > 0)
        v, A = np.where(closed, 0.0, v), np.where(closed, 0.0, A)
    if c["out_relu"]:
        v = np.maximum(v, 0.0)
    r = dict(o=o, out=v, bound=GAMMA * (taps * cin + extra) * A, closed=closed, M=M)
    z = v.reshape(-1, v.shape[-1])
    if c["tail"]:
        z = z @ f64(o["Wd"][0])
        r["tail"] = z.reshape(*c["outd"], 64)
        r["tail_bound"] = GAMMA * (taps * cin + extra) * (A.reshape(-1, 64) @ np.abs(f64(o["Wd"][0]))).reshape(*c["outd"], 64)
    stats = c["stats"] or ""
    if stats.startswith("bwd"):
        C = z.shape[1]
        st = f64(o["y_bn"])
        y = f64(o["y"]).reshape(M, C)
        dz = np.where(y * st[:C] + st[C:2 * C] > 0, z, 0.0) if c["bwd_relu"] else z
        yhat = (y - st[2 * C:3 * C]) * st[3 * C:]
        r.update(db=dz.sum(0), dg=(dz * yhat).sum(0), tol_s=3e-6 * np.sqrt(M) * np.abs(dz).max())
        if c["dense_dw"]:
            r["dW"] = conv_ref.conv_wgrad(o["y"], o["x"], c["outd"], c["k"], c["s"], c["p"], in_bn=(st[:C], st[C:2 * C]),
                                          relu=c["bwd_relu"])
    elif stats:
        r.update(sums=np.stack([z.sum(0), (z * z).sum(0)])[None], ymax=np.abs(z).max())
    # planes no depth tap reaches: gate(bias + previous) in fp32, exactly
    dead = {}
    if not c["rows"] and not c["ps"]:
        for d, n in enumerate(E.facts_of(c)["depth_taps"]):
            if n == 0:
                e = np.zeros((*c["outd"][1:], cout), np.float32) + (o["bias"] if c["bias"] else np.float32(0))
                if c["accumulate"]:
                    e = e + o["prev"][d]
                if c["gate"]:
                    e = np.where(o["gate"][d] > 0, e, np.float32(0))
                if c["out_relu"]:
                    e = np.maximum(e, np.float32(0))
                dead[d] = e.astype(np.float32)
    r["dead"] = dead
    return r


# ---- buffers ---------------------------------------------------------------------------------------------------------------
def _packed(W, what):
    """lisec_conv_pack_weights of a (taps, K, N) kernel into a 0xff-filled buffer: the image equals the host repack bit for bit,
    padding zeros included, and nothing behind it is touched"""
    from lisec_amd import ops
    taps, K, N = W.shape
    n = ops.packed_floats(taps, K, N)
    buf = torch.full(((n + 64) * 4,), 0xFF, dtype=torch.uint8, device=_dev()).view(torch.float32)
    ops.pack_weights(_t(W), taps, K, N, K * N, N, 1, out=buf[:n])
    torch.cuda.synchronize()
    want = R.packed_layout(W, 4)
    assert n == want.size, f"{what}: packed size {n}, host layout {want.size}"
    assert np.array_equal(buf[:n].cpu().numpy().view(np.int32), want.view(np.int32)), f"{what}: packed image differs from the host repack"
    assert bool((buf[n:].view(torch.uint8) == 0xFF).all()), f"{what}: written behind the packed image"
    return buf[:n]


def _workspace_bytes(c, g):
    from lisec_amd import _lib
    lib = _lib.load()
    if c["rows"]:
        return lib.lisec_conv_forward_rows_workspace_bytes(ctypes.byref(g), c["rows"][0])
    return lib.lisec_conv_forward_workspace_bytes(ctypes.byref(g))


class _Call:
    """One lisec_conv_forward_ex call of a case with every guard in place (built and run under the case's knobs)."""

    def __init__(self, c, r):
        from lisec_amd import ops
        self.c, self.r = c, r
        o = r["o"]
        cin, cout, M = c["cin"], c["cout"], r["M"]
        dev = _dev()
        stats = c["stats"] or ""
        self.g = E.geom_of(c)
        self.x = Guarded(c["ind"], cin, c["in_stride"], data=o["x"])
        dims, ch = E.out_shape(c)
        self.out = Guarded(dims, ch, c["out_stride"], guard=SENTINEL)
        self.w = _packed(o["W"], c["name"])
        self.kw = dict(flags=E.flags_of(c))
        self.guards = [("x", self.x), ("out", self.out)]
        if c["bias"]:
            self.kw["bias"] = _t(o["bias"])
        if c["in_bn"]:
            self.kw["in_bn"] = _t(o["in_bn"])
        if c["gate"]:
            self.gate = Guarded(dims, ch, c["out_stride"], data=o["gate"])
            self.kw["out_mask"] = self.gate.view
            self.guards.append(("gate", self.gate))
        if c["fold"]:
            self.fold_y = Guarded(c["ind"], cin, c["in_stride"], data=o["fold_y"])
            self.kw["fold"] = (self.fold_y.view, _t(o["fold_bn"]), _t(o["fold_coef"]), c["fold"] == "relu")
            self.guards.append(("in_y", self.fold_y))
        self.tail_out = None
        if c["tail"]:
            self.tail_out = Guarded(c["outd"], 64, guard=SENTINEL)
            self.kw["tail"] = (_packed(o["Wd"], c["name"] + " tail"), self.tail_out.view)
            self.guards.append(("tail_out", self.tail_out))
        # statistics: what the call (or its finaliser) must write completely starts as NaN
        self.written, self.sink, self.moving, self.table, self.slabs = {}, None, None, None, None
        cy = 64 if c["tail"] else cout
        if stats.startswith("bwd"):
            self.y = Guarded(c["outd"], cy, data=o["y"])
            self.guards.append(("bwd_y", self.y))
            self.kw["bwd"] = (self.y.view, _t(o["y_bn"]), c["bwd_relu"])
        if stats == "bwd sink":
            self.written = dict(dgamma=torch.empty(cy, device=dev), dbeta=torch.empty(cy, device=dev))
            self.sink = ops.BnSink(cy, M, dev, dgamma=self.written["dgamma"], dbeta=self.written["dbeta"])
            self.written["coef"] = self.sink.coef
        elif stats == "sink":
            self.written = dict(bnstate=torch.empty(4 * cout, device=dev))
            self.moving = (_t(o["moving_mean"]), _t(o["moving_var"]))
            self.sink = ops.BnSink(cout, M, dev, gamma=_t(o["gamma"]), beta=_t(o["beta"]), moving_mean=self.moving[0],
                                   moving_var=self.moving[1], unbiased=True, bnstate=self.written["bnstate"])
        elif stats:
            self.nb = ops.num_mblocks_bwd(self.g) if stats.startswith("bwd") else ops.num_mblocks(self.g)
            self.table = torch.empty((self.nb + 2, 2, cout), dtype=torch.float64, device=dev)
            self.kw["stats"] = self.table
        if self.sink is not None:
            self.kw["sink"] = self.sink
        if c["dense_dw"]:
            self.n_slabs = ops.dense_dw_slabs()
            self.slabs = torch.empty((self.n_slabs + 1) * 4096, device=dev)
            self.dW = torch.empty(64 * 64 + 64, device=dev)
            self.kw["dense_dw"] = self.slabs
        # row list: the coordinates lie between two guard rows; rows at and above the count hold positions one past the map
        self.count = None
        if c["rows"]:
            cap, n = c["rows"]
            beyond = torch.tensor(c["outd"], dtype=torch.int32, device=dev)
            self.coords = beyond.repeat(cap + 2, 1).contiguous()
            self.coords[1:1 + n] = _t(o["coords"][:n])
            self.count = n
            self.kw["rows"] = (self.coords[1:1 + cap], torch.tensor([n, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev), cap)
        self.queue = None
        if c["queue"]:
            self.queue = torch.zeros(8, dtype=torch.int32, device=dev)
            self.queue[2:] = 0x5A5A5A5A
            self.kw["queue"] = self.queue
        # the K-slice workspace: exactly the queried size, [zero head][0xff slabs][pattern tail]
        self.ws_bytes = _workspace_bytes(c, self.g) if c["splitk"] else 0
        self.ws_whole = None
        if self.ws_bytes:
            assert self.ws_bytes >= HEAD_BYTES
            self.ws_whole = torch.zeros(self.ws_bytes + TAIL_BYTES, dtype=torch.uint8, device=dev)
            self.ws_whole[HEAD_BYTES:self.ws_bytes] = 0xFF
            self.ws_whole[self.ws_bytes:] = TAIL_BYTE
            self.kw["workspace"] = self.ws_whole[:self.ws_bytes]
        else:
            self.kw["splitk"] = False

    def plan(self):
        from lisec_amd import ops
        kw = {k: v for k, v in self.kw.items() if k in ("out_mask", "bwd", "sink", "queue", "tail", "fold", "dense_dw")}
        self.listed_plan = ops.conv_plan(self.g, in_bn="in_bn" in self.kw, flags=self.kw["flags"], stats=self.table is not None,
                                         splitk=self.ws_bytes > 0, rows_capacity=self.c["rows"][0] if self.c["rows"] else 0, **kw)
        return self.listed_plan

    def run(self, what):
        """arms the guards, calls, checks the guards; returns the host copies of everything the call wrote"""
        from lisec_amd import ops
        c, o = self.c, self.r["o"]
        self.out.set(o["prev"] if c["accumulate"] else NAN)
        if self.count is not None:
            self.out.view[0, 0, self.count:] = SENTINEL
        if self.tail_out is not None:
            self.tail_out.set(NAN)
        for t in self.written.values():
            t.fill_(NAN)
        if self.table is not None:
            self.table[:self.nb] = NAN
            self.table[self.nb:] = SENTINEL
        if self.slabs is not None:
            self.slabs.fill_(NAN)
            self.slabs[self.n_slabs * 4096:] = SENTINEL
            self.dW.fill_(NAN)
            self.dW[4096:] = SENTINEL
        for _, gd in self.guards:
            gd.snapshot()
        got = {}
        if self.moving:
            got["moving_before"] = tuple(m.cpu().numpy() for m in self.moving)
        ops.conv_forward(self.g, self.x.view, self.w, self.out.view, **self.kw)
        if self.slabs is not None:
            ops.dense_dw_reduce(self.slabs[:self.n_slabs * 4096], self.dW[:4096])
        torch.cuda.synchronize()
        for name, gd in self.guards:
            gd.check(f"{what}: {name}")
        got["out"] = self.out.host()
        if self.count is not None:
            above = self.out.view[0, 0, self.count:]
            assert torch.equal(_bits(above), _bits(torch.full_like(above, SENTINEL))), f"{what}: a row at or above the count was written"
            got["out"] = got["out"][:, :, :self.count]
        if self.tail_out is not None:
            got["tail"] = self.tail_out.host()
        for k, t in self.written.items():
            got[k] = t.cpu().numpy()
        if self.table is not None:
            tab = self.table.cpu().numpy()
            assert np.array_equal(tab[self.nb:], np.full_like(tab[self.nb:], SENTINEL)), f"{what}: a table row that belongs to no tile was written"
            got["table"] = tab[:self.nb]
        if self.slabs is not None:
            assert bool((self.slabs[self.n_slabs * 4096:] == SENTINEL).all()) and bool((self.dW[4096:] == SENTINEL).all()), f"{what}: written behind the slabs / dW"
            got["dW"] = self.dW[:4096].cpu().numpy().reshape(1, 64, 64)
        if self.sink is not None:
            assert int(self.sink.acc.abs().sum().item()) == 0, f"{what}: sink accumulators not back at zero"
            if self.moving:
                got["moving"] = tuple(m.cpu().numpy() for m in self.moving)
        if self.queue is not None:
            q = self.queue.cpu().numpy()
            assert not q[:2].any() and (q[2:] == 0x5A5A5A5A).all(), f"{what}: queue words {q}"
        if self.ws_whole is not None:
            assert bool((self.ws_whole[self.ws_bytes:] == TAIL_BYTE).all()), f"{what}: written behind the workspace"
            assert int(self.ws_whole[:HEAD_BYTES].view(torch.int32).abs().sum().item()) == 0, f"{what}: arrival / pair counters not back at zero"
            if self.count is not None:
                # tiles at or above the device count exit at once (plan_conv: "K slicing is planned for the capacity; workgroups
                # past the device-side row count exit at once"): their slabs [slice][tile] of 128 x 64 floats stay 0xff
                tiles, slices = self.listed_plan["tiles"], self.listed_plan["k_slices"]
                assert c["cout"] <= 64 and HEAD_BYTES + slices * tiles * SLAB_BYTES <= self.ws_bytes
                slabs = self.ws_whole[HEAD_BYTES:HEAD_BYTES + slices * tiles * SLAB_BYTES].view(slices, tiles, SLAB_BYTES)
                idle = slabs[:, -(-self.count // 128):]
                assert bool((idle == 0xFF).all()), f"{what}: a tile that holds no rows wrote its K-slice slab"
        return got


# ---- checks ------------------------------------------------------------------------------------------------------------------
def _elementwise(got, ref, bound, closed, what):
    """every element written; closed gates exactly 0.0; |got - ref| <= bound everywhere; returns the largest err / bound"""
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements unwritten or NaN"
    assert not np.any(got[closed]), f"{what}: a gated-off element is not exactly 0.0"
    err = np.abs(f64(got) - ref)
    over = err > bound
    assert not over.any(), (f"{what}: {int(over.sum())} elements beyond the a-priori bound, worst err {err[over].max():.3e} at "
                            f"{np.argwhere(over)[0].tolist()} (bound {bound[over][np.argmax(err[over])]:.3e})")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check(c, r, got, what):
    """every result of one call against the fp64 definitions; returns {entry point: largest err / bound}"""
    M = r["M"]
    stats = c["stats"] or ""
    ratios = {}
    ratios["out"] = _elementwise(got["out"], r["out"], r["bound"], r["closed"], f"{what}: out")
    if r["out"].size and np.any(r["out"]):
        e = rel_l2(got["out"], r["out"])
        assert e <= TOL, f"{what}: out relative L2 {e:.2e}"
        ratios["out L2"] = e / TOL
    for d, want in r["dead"].items():
        assert np.array_equal(got["out"][d], want), f"{what}: plane {d} has no live tap and must be gate(bias + previous) exactly"
        if c["tail"]:
            assert not np.any(got["tail"][d]), f"{what}: tail_out of the dead plane {d} must be exactly 0.0"
    if c["tail"]:
        ratios["tail"] = _elementwise(got["tail"], r["tail"], r["tail_bound"], np.zeros(r["tail"].shape, bool), f"{what}: tail_out")
        e = rel_l2(got["tail"], r["tail"])
        assert e <= TOL, f"{what}: tail_out relative L2 {e:.2e}"
        ratios["tail L2"] = e / TOL
    if stats.startswith("bwd"):
        C = len(r["db"])
        k = 4 if c["tail"] else 3
        ts = r["tol_s"]
        if stats == "bwd sink":
            ratios["bsink"] = max(_within(got["dbeta"], r["db"], ts, f"{what}: dbeta"),
                                  _within(got["dgamma"], r["dg"], k * ts, f"{what}: dgamma"),
                                  _within(got["coef"][:C], r["db"] / M, ts / M, f"{what}: coef (mean dz)"),
                                  _within(got["coef"][C:], r["dg"] / M, k * ts / M, f"{what}: coef (mean dz yhat)"))
        else:
            assert np.isfinite(got["table"]).all(), f"{what}: a table row of a tile was not written"
            ratios["btable"] = max(_within(got["table"][:, 0].sum(0), r["db"], ts, f"{what}: table sum dz"),
                                   _within(got["table"][:, 1].sum(0), r["dg"], k * ts, f"{what}: table sum dz yhat"))
        if c["dense_dw"]:
            e = rel_l2(got["dW"], r["dW"])
            assert e <= TOL_W, f"{what}: Dense weight gradient relative L2 {e:.2e}"
            ratios["dense_dw"] = e / TOL_W
    elif stats:
        o, cout = r["o"], c["cout"]
        part = lambda a, i: f64(a[i * cout:(i + 1) * cout])
        if stats == "sink":
            mm0, mv0 = got["moving_before"]
            st, mm, mv = R.bn_finalize(r["sums"], M, o["gamma"], o["beta"], mm0, mv0, unbiased=True)
            gs = got["bnstate"]
        else:
            assert np.isfinite(got["table"]).all(), f"{what}: a table row of a tile was not written"
            st = R.bn_finalize(r["sums"], M, o["gamma"], o["beta"])[0]
            gs = R.bn_finalize(got["table"], M, o["gamma"], o["beta"])[0]       # the finaliser's arithmetic in fp64 on the kernel's partials
        worst = max(_within(part(gs, 2), part(st, 2), 2e-6 * r["ymax"], f"{what}: batch mean"),
                    _within(part(gs, 3), part(st, 3), 2e-5 * np.abs(part(st, 3)), f"{what}: invstd"),
                    _within(part(gs, 0), part(st, 0), 2e-5 * np.abs(part(st, 0)), f"{what}: scale"),
                    _within(part(gs, 1), part(st, 1), 1e-4 * np.abs(part(st, 1)) + 1e-5, f"{what}: shift"))
        if stats == "sink":
            bound = lambda ref: 2.0 ** -23 * np.abs(ref) + 1e-9 * np.maximum(1.0, np.abs(ref))
            worst = max(worst, _within(got["moving"][0], mm, bound(mm), f"{what}: moving mean"),
                        _within(got["moving"][1], mv, bound(mv), f"{what}: moving variance"))
        ratios["fsink" if stats == "sink" else "ftable"] = worst
    return ratios


def _entry(c):
    if c["rows"]:
        return "row list"
    if c["ps"]:
        return "pixel shuffle"
    return "forward out" if c["mode"] == 0 else "data gradient out"


LABELS = (("tail", "tail_out"), ("tail L2", "tail_out, relative L2"), ("fsink", "forward sink"), ("bsink", "backward sink"),
          ("ftable", "forward table"), ("btable", "backward table"), ("dense_dw", "dense_dw weight gradient"))


def _same_bits(a, b, what):
    for k in a:
        if k in ("moving", "moving_before"):
            continue
        bits = lambda v: np.ascontiguousarray(v).view(np.int64 if v.dtype == np.float64 else np.int32)
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("case", E.CASES, ids=IDS)
def test_edge(case):
    """One guarded lisec_conv_forward_ex call per case of the table, on the plan the table lists, twice, against fp64 -- see
    the module docstring."""
    c = case
    r = reference(E.operands_of(c))
    with E.tuning(**c["knobs"]):
        call = _Call(c, r)
        plan = call.plan()
        listed = {k: plan[k] for k in c["plan"]}
        assert listed == c["plan"], f"{c['name']}: plan on the device {listed}, listed {c['plan']} ({plan})"
        first = call.run(f"{c['name']} call 0")
        second = call.run(f"{c['name']} call 1")
    ratios = check(c, r, first, f"{c['name']} call 0")
    _same_bits(first, second, f"{c['name']}: second call")
    if "moving" in first:                              # the second call starts where the first one ended
        for a, b in zip(first["moving"], second["moving_before"]):
            assert np.array_equal(a, b)
    for k, v in check(c, r, second, f"{c['name']} call 1").items():
        ratios[k] = max(ratios[k], v)
    _ratio(_entry(c), ratios["out"])
    if "out L2" in ratios:
        _ratio(_entry(c) + ", relative L2", ratios["out L2"])
    for k, label in LABELS:
        if k in ratios:
            _ratio(label, ratios[k])


@pytest.mark.parametrize("pair", E.IDENTICAL, ids=[f"{a} == {b}" for a, b in E.IDENTICAL])
def test_forms_of_the_same_arithmetic_are_bit_identical(pair):
    """The tile queue against one workgroup per tile, plane pairs on against off, 64-row against 128-row tiles at equal
    slicing: the code documents each pair as the same sums in the same order, so the same operands give the same bits."""
    results = []
    for name in pair:
        c = E.by_name(name)
        r = reference(E.operands_of(c))
        with E.tuning(**c["knobs"]):
            call = _Call(c, r)
            plan = call.plan()
            assert {k: plan[k] for k in c["plan"]} == c["plan"], (name, plan)
            results.append(call.run(name))
    _same_bits(results[0], results[1], f"{pair[0]} against {pair[1]}")


def test_pack_table_over_a_dirty_buffer():
    """lisec_conv_pack_weights_batched: three ragged kernels (68 x 65, 4 x 1, 20 x 256 with 9 taps) in one launch into ONE
    0xff-filled buffer equal the host repacks, padding zeros included; the 64 floats behind the last image stay 0xff."""
    from lisec_amd import ops
    rng = np.random.default_rng(E.seed_of("pack table"))
    kernels = [rng.normal(0, 1, shape).astype(np.float32) for shape in ((9, 68, 65), (9, 4, 1), (9, 20, 256))]
    sizes = [ops.packed_floats(*w.shape) for w in kernels]
    buf = torch.full(((sum(sizes) + 64) * 4,), 0xFF, dtype=torch.uint8, device=_dev()).view(torch.float32)
    entries, start = [], 0
    for w, n in zip(kernels, sizes):
        taps, K, N = w.shape
        entries.append((_t(w), buf[start:start + n], taps, K, N, K * N, N, 1))
        start += n
    table = ops.PackTable(entries, _dev())
    for rep in range(2):
        table.run()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        start = 0
        for w, n in zip(kernels, sizes):
            want = R.packed_layout(w, 4)
            assert want.size == n and np.array_equal(host[start:start + n].view(np.int32), want.view(np.int32)), w.shape
            start += n
        assert bool((buf[start:].view(torch.uint8) == 0xFF).all()), "written behind the last image"
