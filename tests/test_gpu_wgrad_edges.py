"""lisec_conv_wgrad / lisec_conv_wgrad_batched at the edge geometries of tests/wgrad_edge_cases.py against the fp64 restatement
oracle/conv_ref.conv_wgrad: every contraction kernel variant of csrc/wgrad.hip (ring 3 / 5 / 6 passes, w-halo 7 / 9, plain,
row list), every reduce form (in the kernel, k_wgrad_ring_reduce, k_wgrad_reduce_lanes, k_wgrad_reduce) and the edges the
Lyft maps never produce: remainder tiles, partial channel blocks, strided operands, tap groups that read nothing, mirrored
taps, uneven runs, slabs that cross line ends, batches of unlike items.  tests/test_wgrad_edge_plans.py asserts on the host
that every case engages the plan it is listed for.

Each call runs with guards around everything it writes: the gradient sits in front of one more tap-sized block, both filled
with NaN; the workspace has exactly the queried size (queried under the default knobs, as the network sizes its own) and a
4 KiB tail of a fixed byte pattern behind it; its head -- the arrival counters -- is zero, as the ABI asks, and the slabs
behind the head are filled with 0xff bytes (NaN), the state a workspace shared between layers is in: a slab sum that reads
a slab nobody wrote gives NaN here instead of a zero it did not earn.  The call runs twice on the same workspace: bit-identical
results, counters back at zero.

Bound: relative L2 <= TOL_W = 3e-6 over the whole gradient AND over every tap on its own (one wrong tap cannot hide among 26
right ones); the sums here are at most ~5 000 rows long, the Lyft layers hold the same bound over 20 000 - 320 000.  A tap
whose reference is identically zero (no output position reads it) must be exactly 0.0."""
import numpy as np
import pytest
import torch

import wgrad_edge_cases as E
from test_gpu_lyft_layers import TOL_W, rel_l2

pytestmark = pytest.mark.gpu

HEAD_BYTES = 4096 * 4                # the arrival counters at the head of every weight-gradient workspace
TAIL_BYTES, TAIL_BYTE = 4096, 0xA5


def _strided(a, stride, dev):
    """a (..., C) as the last C channels of a (..., stride) device tensor whose other channels are NaN: the view ends
    exactly where the allocation ends."""
    if stride is None:
        return torch.from_numpy(a).to(dev)
    full = torch.full((*a.shape[:-1], stride), float("nan"), device=dev)
    view = full[..., stride - a.shape[-1]:]
    view.copy_(torch.from_numpy(a))
    return view


class _Operands:
    """Device tensors, guards and the fp64 reference of one contraction."""

    def __init__(self, c, dev, name=None):
        from lisec_amd import ops
        from oracle import conv_ref
        self.c, self.name = c, name or c["name"]
        x, dy, st, coords = E.draw(c, self.name)
        self.g = E.geom_of(c)
        self.flags = E.flags_of(c)
        self.x = _strided(x, c.get("in_stride"), dev)
        self.st = torch.from_numpy(st).to(dev) if st is not None else None
        self.in_bn = self.st if c.get("in_bn") else None
        self.dy_bn = self.st if c.get("dy_bn") else None
        self.rows, nrows = None, None
        if c.get("rows"):
            cap, nrows = c["rows"]
            dy[nrows:] = np.nan                              # rows at or above the device count are void
            count = torch.tensor([nrows, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            self.rows = (torch.from_numpy(coords).to(dev), count, cap)
        self.dy = _strided(dy, c.get("out_stride"), dev)
        cin, cout = c["cin"], c["cout"]
        self.ntaps = c["k"][0] * c["k"][1] * c["k"][2]
        self.transpose = bool(c.get("transpose_out"))
        n = self.ntaps * cin * cout
        self.dW_all = torch.empty(n + cin * cout, device=dev)
        self.dW = self.dW_all[:n].view((self.ntaps, cout, cin) if self.transpose else (self.ntaps, cin, cout))
        c64 = lambda v: v.astype(np.float64)
        bn_ref = (c64(st[:cin]), c64(st[cin:2 * cin])) if c.get("in_bn") else None
        dy_ref = dy
        if c.get("dy_bn"):                                   # the dY operand's affine + ReLU, before the contraction
            dy_ref = np.maximum(c64(dy) * c64(st[:cout]) + c64(st[cout:2 * cout]), 0.0)
        if nrows is not None:
            dy_ref, coords = dy_ref[:nrows], coords[:nrows]
        self.ref = conv_ref.conv_wgrad(x, dy_ref, c["outd"], c["k"], c["s"], c["p"], mode=c["mode"], in_bn=bn_ref,
                                       relu=bool(c.get("relu")), rows=coords)

    def arm(self):
        self.dW_all.fill_(float("nan"))

    def gradient(self):
        """the guards hold; the gradient as (taps, Cin, Cout) on the host"""
        n = self.dW.numel()
        got = self.dW_all.cpu()
        assert not torch.isnan(got[:n]).any(), f"{self.name}: {int(torch.isnan(got[:n]).sum())} of {n} gradient elements not written (or NaN)"
        assert torch.isnan(got[n:]).all(), f"{self.name}: written behind the gradient"
        got = got[:n].view(self.dW.shape).numpy()
        return np.transpose(got, (0, 2, 1)) if self.transpose else got

    def check(self, got, note):
        ref = self.ref
        e = rel_l2(got, ref, note=f"weight gradient edge {note}") if np.any(ref) else 0.0
        worst, worst_tap = 0.0, -1
        for tap in range(self.ntaps):
            if not np.any(ref[tap]):
                assert not np.any(got[tap]), f"{self.name}: tap {tap} reads nothing and must be exactly 0.0, max |dW| {np.abs(got[tap]).max():.3e}"
                continue
            et = rel_l2(got[tap], ref[tap])
            if et > worst:
                worst, worst_tap = et, tap
        if worst_tap >= 0:
            rel_l2(got[worst_tap], ref[worst_tap], note=f"weight gradient edge {note}, worst tap {worst_tap}")
        print(f"{note}: relative L2 {e:.3e}, worst tap {worst_tap}: {worst:.3e}")
        assert e <= TOL_W, f"{self.name}: weight gradient relative L2 {e:.2e}"
        assert worst <= TOL_W, f"{self.name}: tap {worst_tap} relative L2 {worst:.2e}"


def _workspace(nbytes, dev):
    """[zero head][0xff slabs][guard tail]; returns (workspace of exactly nbytes, the whole allocation)"""
    assert nbytes >= HEAD_BYTES
    whole = torch.zeros(nbytes + TAIL_BYTES, dtype=torch.uint8, device=dev)
    whole[HEAD_BYTES:nbytes] = 0xFF
    whole[nbytes:] = TAIL_BYTE
    return whole[:nbytes], whole


def _check_workspace(whole, nbytes, name):
    assert bool((whole[nbytes:] == TAIL_BYTE).all()), f"{name}: written behind the workspace"
    assert int(whole[:HEAD_BYTES].view(torch.int32).abs().sum().item()) == 0, f"{name}: arrival counters not back at zero"


def _prime_lds(dev):
    """An ATTEMPT to leave NaN where H1's A image lies in every CU's LDS: H3's geometry over 600 lines (600 workgroups of the
    nine-pass w-halo kernel, more than two per CU) with x all NaN, output discarded.  Its A image -- 130 rows from the start
    of the dynamic LDS, where H1's starts too -- is NaN throughout.  Whether H1's workgroups then get the same LDS ranges is
    up to the CU's allocator: the priming makes a stale-LDS read likely to show, it cannot promise it."""
    from lisec_amd import ops
    dims = (1, 600, 127)
    g = ops.geom(0, dims, dims, E.K113, E.S1, (0, 0, 1), 64, 64)
    plan = ops.wgrad_plan(g)
    assert plan["halo"] == 1 and plan["staging_passes"] == 9 and plan["workgroups"] >= 600, plan
    x = torch.full((*dims, 64), float("nan"), device=dev)
    dy = torch.ones((*dims, 64), device=dev)
    ws = torch.zeros(ops.wgrad_workspace_bytes(g), dtype=torch.uint8, device=dev)
    ops.conv_wgrad(g, x, dy, torch.empty(3, 64, 64, device=dev), ws)
    torch.cuda.synchronize()


SINGLE = E.CASES


@pytest.mark.parametrize("case", SINGLE, ids=[c["name"] for c in SINGLE])
def test_weight_gradient_edge(case):
    """One lisec_conv_wgrad call per case of the table, guarded, twice, against fp64 -- see the module docstring.
    H1 (tiles of 108 rows: DR = 112, an A image of 114 rows) is run behind _prime_lds: with seven staging passes its last
    chunk read rows 112 and 113 of the image, which nothing had written; the nine-pass variant it takes now stages them.
    The case passes with or without the priming."""
    from lisec_amd import ops
    dev = torch.device("cuda")
    c = case
    o = _Operands(c, dev)
    cap = c["rows"][0] if c.get("rows") else 0
    nbytes = ops.wgrad_workspace_bytes(o.g, cap)             # default knobs
    ws, whole = _workspace(nbytes, dev)
    results = []
    with E.tuning(**c["knobs"]):
        for rep in range(2):
            o.arm()
            if c["name"].startswith("H1") and rep == 0:
                _prime_lds(dev)
            ops.conv_wgrad(o.g, o.x, o.dy, o.dW, ws, in_bn=o.in_bn, flags=o.flags, transpose_out=o.transpose, dy_bn=o.dy_bn,
                           rows=o.rows)
            torch.cuda.synchronize()
            results.append(o.gradient())
            _check_workspace(whole, nbytes, c["name"])
    assert np.array_equal(results[0], results[1]), f"{c['name']}: the second run differs from the first"
    o.check(results[0], c["name"])


@pytest.mark.parametrize("batch", E.BATCHES, ids=[b[0] for b in E.BATCHES])
def test_batched_weight_gradient_edge(batch):
    """lisec_conv_wgrad_batched over UNLIKE items: three ring items of different maps and channel blocks in one launch (B1),
    the same three in one launch of k_wgrad_halo_batch (B2: the grids differ per item), and two items whose staging variants
    differ, which run one by one in the shared workspace (B3).  The workspace is what batch.workspace_bytes() says for the
    knobs the batch runs under, and not a byte more."""
    from lisec_amd import ops
    dev = torch.device("cuda")
    name, items, knobs, _ = batch
    ops_ = [_Operands(c, dev, name=f"{name}.{i}") for i, c in enumerate(items)]
    b = ops.WgradBatch([(o.g, o.x, o.dy, o.dW, o.in_bn, o.flags, o.transpose) for o in ops_])
    results = []
    with E.tuning(**knobs):
        nbytes = b.workspace_bytes()
        ws, whole = _workspace(nbytes, dev)
        for rep in range(2):
            for o in ops_:
                o.arm()
            b.run(ws)
            torch.cuda.synchronize()
            results.append([o.gradient() for o in ops_])
            _check_workspace(whole, nbytes, name)
    for i, o in enumerate(ops_):
        assert np.array_equal(results[0][i], results[1][i]), f"{name} item {i}: the second run differs from the first"
        o.check(results[0][i], f"{name} item {i}")
