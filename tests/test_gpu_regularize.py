"""lisec_regularize alone (csrc/regularize.hip) against an fp64 numpy oracle of the Keras semantics:
    grad' = grad + 2*l2*w + l1*sign(w), sign(0) = 0;     P = sum over chunks of l1*sum|w| + l2*sum w^2  (math.fsum).
Segments of 4, 4092, 4096, 4100 and 3*4096+8 floats (one chunk below, at and above LISEC_REG_CHUNK; several chunks; a
single float4), an unregularised gap between the first two and behind the last, one segment with (0, 0); weights of
both signs with exact zeros.  A buffer of 24 604 floats, 24 588 of them in chunks."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 4096
L1, L2 = np.float32(0.0123), np.float32(3.7e-4)
# (offset, length, l1, l2): l1 only, [gap of 8], l2 only, both, (0, 0), both
SEGMENTS = [(0, 4, L1, 0.0), (12, 4092, 0.0, L2), (4104, 4096, L1, L2), (8200, 4100, 0.0, 0.0),
            (12300, 3 * 4096 + 8, np.float32(0.5), np.float32(0.25))]
N = 12300 + 3 * 4096 + 8 + 8                                   # 8 unregularised floats behind the last segment
U = 2.0 ** -24


def _chunks():
    rows = []
    for off, n, l1, l2 in SEGMENTS:
        for s in range(0, n, CHUNK):
            rows.append((off + s, min(CHUNK, n - s), float(l1), float(l2)))
    return rows


@pytest.fixture(scope="module")
def case():
    """Inputs and the fp64 oracle, computed once and left unchanged."""
    rng = np.random.default_rng(5)
    w = rng.normal(0, 0.3, N).astype(np.float32)
    w[rng.random(N) < 0.1] = 0.0                               # exact zeros: sign(0) = 0
    w[::7] *= -1.0
    w[1], w[13], w[4104] = 0.0, -0.0, 0.0
    g = rng.normal(0, 1e-2, N).astype(np.float32)
    rows = _chunks()
    assert len(rows) == 1 + 1 + 1 + 2 + 4 and sum(r[1] for r in rows) <= 65536
    ref, bound, terms = g.astype(np.float64), np.zeros(N), []
    touched = np.zeros(N, bool)
    for off, n, l1, l2 in rows:
        ww = w[off:off + n].astype(np.float64)
        if l1 != 0 or l2 != 0:
            ref[off:off + n] += 2.0 * l2 * ww + l1 * np.sign(ww)
            bound[off:off + n] = 4 * U * (np.abs(g[off:off + n].astype(np.float64)) + np.abs(2.0 * l2 * ww) + abs(l1))
            touched[off:off + n] = True
        terms.extend((l1 * np.abs(ww)).tolist())
        terms.extend((l2 * ww * ww).tolist())
    w.setflags(write=False)
    g.setflags(write=False)
    return dict(w=w, g=g, rows=rows, ref=ref, bound=bound, touched=touched, P=math.fsum(terms),
                P_by_chunk=[math.fsum((l1 * np.abs(w[o:o + n].astype(np.float64))).tolist()
                                      + (l2 * w[o:o + n].astype(np.float64) ** 2).tolist()) for o, n, l1, l2 in rows])


class Dev:
    """Device copies of a case and the buffers of one call."""

    def __init__(self, case):
        import torch
        from lisec_amd import _lib, ops
        self.dev = _lib.require_gpu()
        self.theta = torch.from_numpy(case["w"].copy()).to(self.dev)
        self.grad = torch.from_numpy(case["g"].copy()).to(self.dev)
        self.table = ops.reg_table(case["rows"], self.dev)
        self.ws = ops.reg_workspace(len(case["rows"]), self.dev)
        self.penalty = torch.full((1,), -7.0, dtype=torch.float64, device=self.dev)

    def run(self, n=None, first=0, grad=True, **kw):
        import torch
        from lisec_amd import ops
        n = self.table.numel() // 24 - first if n is None else n
        ops.regularize(self.theta, self.grad if grad else None, self.table, n, self.penalty, self.ws, first=first, **kw)
        torch.cuda.synchronize()
        return self.grad.cpu().numpy(), float(self.penalty.item())


def test_gradient_and_penalty_match_the_oracle(case):
    d = Dev(case)
    got, P = d.run()
    err = np.abs(got.astype(np.float64) - case["ref"])
    t = case["touched"]
    worst = float((err[t] / case["bound"][t]).max())
    print(f"gradient: worst error / bound = {worst:.3f}; P = {P!r}, oracle {case['P']!r}, "
          f"relative {abs(P - case['P']) / case['P']:.3e}")
    assert np.all(err[t] <= case["bound"][t]), worst
    # outside every chunk, and inside the (0, 0) segment: the very bits
    assert t.sum() == 4 + 4092 + 4096 + 3 * 4096 + 8
    assert np.array_equal(got[~t].view(np.uint32), case["g"][~t].view(np.uint32))
    assert not np.array_equal(got[t], case["g"][t])
    assert abs(P - case["P"]) <= 1e-11 * case["P"]
    assert np.array_equal(d.theta.cpu().numpy().view(np.uint32), case["w"].view(np.uint32))      # theta is only read


def test_sign_of_zero_is_zero(case):
    d = Dev(case)
    got, _ = d.run()
    zero = (case["w"] == 0) & case["touched"]
    assert zero.sum() > 1000
    assert np.array_equal(got[zero], case["g"][zero])           # 2*l2*0 + l1*0


def test_two_runs_give_the_same_bits(case):
    a, b = Dev(case), Dev(case)
    ga, Pa = a.run()
    gb, Pb = b.run()
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    assert np.float64(Pa).view(np.uint64) == np.float64(Pb).view(np.uint64)


@pytest.mark.parametrize("split", [1, 3, 6])
def test_a_sub_range_then_the_rest_accumulated(case, split):
    whole, parts = Dev(case), Dev(case)
    gw, Pw = whole.run()
    _, P_head = parts.run(n=split)
    want_head = math.fsum(case["P_by_chunk"][:split])
    assert abs(P_head - want_head) <= 1e-11 * max(want_head, 1e-300)
    gp, Pp = parts.run(first=split, accumulate=True)
    assert np.array_equal(gw.view(np.uint32), gp.view(np.uint32))
    assert abs(Pp - case["P"]) <= 1e-11 * case["P"] and abs(Pp - Pw) <= 1e-11 * case["P"]


def test_grad_is_zero_chunks_store_the_term(case):
    """LISEC_REG_GRAD_IS_ZERO: what the slot held is not read -- the term alone is stored, within the same bound with
    g = 0 -- so a second pass over the same weights leaves the same bits instead of adding the term again.  The other
    chunks, the (0, 0) segment (flagged too: still no store) and P are those of the plain table."""
    import torch
    from lisec_amd import ops
    plain = Dev(case)
    gp, Pp = plain.run()
    flagged = {4104, 8200, 8200 + CHUNK}                       # the 4096-float segment with both, and the (0, 0) one
    d = Dev(case)
    d.table = ops.reg_table([r + (1 if r[0] in flagged else 0,) for r in case["rows"]], d.dev)
    got, P = d.run()
    seg = slice(4104, 4104 + 4096)
    w = case["w"][seg].astype(np.float64)
    l1, l2 = float(L1), float(L2)
    term = 2.0 * l2 * w + l1 * np.sign(w)
    assert np.all(np.abs(got[seg].astype(np.float64) - term) <= 4 * U * (np.abs(2.0 * l2 * w) + abs(l1)))
    assert not np.array_equal(got[seg], gp[seg])               # the plain table added the term to g there
    rest = np.ones(N, bool)
    rest[seg] = False
    assert np.array_equal(got[rest].view(np.uint32), gp[rest].view(np.uint32))
    assert np.float64(P).view(np.uint64) == np.float64(Pp).view(np.uint64)
    again, _ = d.run()                                          # the step after: stored again, not accumulated
    assert np.array_equal(again[seg].view(np.uint32), got[seg].view(np.uint32))
    assert not np.array_equal(again[:4], got[:4])               # an ordinary chunk adds its term once more
    torch.cuda.synchronize()


def test_penalty_only_writes_nothing_else(case):
    with_grad, alone = Dev(case), Dev(case)
    _, P = with_grad.run()
    got, Pa = alone.run(grad=False)
    assert np.float64(P).view(np.uint64) == np.float64(Pa).view(np.uint64)
    assert np.array_equal(got.view(np.uint32), case["g"].view(np.uint32))
    assert np.array_equal(alone.theta.cpu().numpy().view(np.uint32), case["w"].view(np.uint32))


def test_loss_total_is_folded_once_float32_rounded(case):
    import torch
    d = Dev(case)
    loss = torch.tensor([3.25, 7.0, 9.0], dtype=torch.float32, device=d.dev)
    _, P = d.run(loss_total=loss)
    assert loss.cpu().tolist() == [float(np.float32(3.25 + P)), 7.0, 9.0]
    # an accumulating call folds the SUM of both parts, once
    d2 = Dev(case)
    loss2 = torch.tensor([3.25, 7.0, 9.0], dtype=torch.float32, device=d.dev)
    d2.run(n=4)
    _, P2 = d2.run(first=4, accumulate=True, loss_total=loss2)
    assert loss2.cpu().tolist() == [float(np.float32(3.25 + P2)), 7.0, 9.0]


def test_no_chunks(case):
    import torch
    d = Dev(case)
    loss = torch.tensor([1.5], dtype=torch.float32, device=d.dev)
    got, P = d.run(n=0)
    assert P == 0.0 and np.array_equal(got.view(np.uint32), case["g"].view(np.uint32))
    d.penalty.fill_(0.375)
    _, P = d.run(n=0, accumulate=True, loss_total=loss)
    assert P == 0.375 and loss.item() == 1.875                  # kept, and the fold still happens
    _, P = d.run(n=0, first=len(case["rows"]), loss_total=loss)
    assert P == 0.0 and loss.item() == 1.875


def test_bad_arguments_return_einval_before_any_launch(case):
    import torch
    from lisec_amd import _lib
    d = Dev(case)
    lib = _lib.load()
    n = len(case["rows"])
    loss = torch.tensor([1.5], dtype=torch.float32, device=d.dev)
    T, G, C, P, W, Lo = (_lib.ptr(t) for t in (d.theta, d.grad, d.table, d.penalty, d.ws, loss))
    nb, s = d.ws.numel(), _lib.current_stream()
    assert lib.lisec_regularize_workspace_bytes(n) == 8 * n and nb >= 8 * n
    odd = ctypes.c_void_p(d.theta.data_ptr() + 4)
    bad = [
        lib.lisec_regularize(None, G, C, n, P, 0, Lo, W, nb, s),
        lib.lisec_regularize(T, G, None, n, P, 0, Lo, W, nb, s),
        lib.lisec_regularize(T, G, C, n, None, 0, Lo, W, nb, s),
        lib.lisec_regularize(T, G, C, n, P, 0, Lo, None, nb, s),
        lib.lisec_regularize(T, G, C, -1, P, 0, Lo, W, nb, s),                   # negative count
        lib.lisec_regularize(T, G, C, n, P, 0, Lo, W, 8 * n - 1, s),             # short workspace
        lib.lisec_regularize(T, G, C, n, P, 2, Lo, W, nb, s),                    # accumulate not 0/1
        lib.lisec_regularize(odd, G, C, n, P, 0, Lo, W, nb, s),                  # theta not 16-byte aligned
        lib.lisec_regularize(T, G, None, 0, P, 0, Lo, W, nb, s),                 # NULL table, even for no chunks
    ]
    assert all(r == -1 for r in bad), bad                        # LISEC_EINVAL
    assert b"regularize" in lib.lisec_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.grad.cpu().numpy().view(np.uint32), case["g"].view(np.uint32))
    assert d.penalty.item() == -7.0 and loss.item() == 1.5
