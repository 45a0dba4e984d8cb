"""lisec_weight_decay / lisec_weight_decay_eval on the GPU, through the C ABI, bit for bit against the numpy definition of
tests/weight_decay_ref.py: whole buffers and tables with gaps, every kind of coefficient the issue names, a table longer
than the kernel's grid, canaries around the buffer, every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import weight_decay_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
PAD = 64                                   # canary floats on each side (a multiple of 4: the buffer stays 16-byte aligned)
CANARY = F(-7.25)
CHUNK = 4096                               # LISEC_REG_CHUNK
GRID = 2048                                # kDecayBlocks of csrc/weight_decay.hip: past it the workgroups stride over the table
# the "variables" of a table with gaps, cycled: every second one is left out, so the decayed ones are 64 floats (one chunk)
# and 4200 (a full chunk and a short one)
CYCLE = (64, 32, 4200, 16)
# floats whose table with gaps has GRID + 1 chunks or more: 3 chunks per cycle
ABOVE_GRID = -(-(GRID + 1) // 3) * sum(CYCLE) + 4
SIZES = [0, 4, 1020, 4100, ABOVE_GRID]

_INPUTS = {}


def _inputs(n):
    """The n floats of the shared inputs, made once and left unchanged."""
    if n not in _INPUTS:
        w = R.make_inputs(n, R.SEED)
        w.setflags(write=False)
        _INPUTS[n] = w
    return _INPUTS[n]


def _ranges(n, gaps):
    """The decayed ranges [(start, stop)] of a buffer of n floats: the whole of it, or every second "variable"."""
    if not gaps:
        return [(0, n)] if n else []
    out, at, k = [], 0, 0
    while at < n:
        stop = min(n, at + CYCLE[k % len(CYCLE)])
        if k % 2 == 0:
            out.append((at, stop))
        at, k = stop, k + 1
    return out


def _chunks(ranges):
    """The host table of the ranges: each cut into chunks of at most CHUNK floats, as ops.decay_chunks cuts a variable."""
    return [(a + start, min(CHUNK, b - a - start)) for a, b in ranges for start in range(0, b - a, CHUNK)]


def _coefficient_buffer(weight_decay):
    import torch
    from lisec_amd import _lib, lr_schedules, ops
    buf = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device="cuda")
    ops.lr_schedule_set(buf, lr_schedules.descriptor(weight_decay, 0.0))
    return buf


def _run(n, gaps, weight_decay, s):
    """The pass on the shared inputs with canaries on both sides; returns (the padded buffer after it, the ranges)."""
    import torch
    from lisec_amd import _lib, ops
    w = _inputs(n)
    buf = np.full(n + 2 * PAD, CANARY, F)
    buf[PAD:PAD + n] = w
    theta = torch.from_numpy(buf).cuda()
    ranges = _ranges(n, gaps)
    rows = _chunks(ranges)
    table = ops.decay_table(rows, "cuda")
    coeff = _coefficient_buffer(weight_decay)
    state = torch.tensor([s, 0], dtype=torch.int64, device="cuda")
    inner = ctypes.c_void_p(theta.data_ptr() + 4 * PAD)     # (an int: an empty view has no address)
    _lib.check(_lib.load().lisec_weight_decay(inner, _lib.ptr(table), len(rows), _lib.ptr(coeff), _lib.ptr(state),
                                              _lib.current_stream()))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [s, 0]                   # the count is read, never advanced; no ticket is taken
    return theta.cpu().numpy(), ranges


def _check(n, gaps, weight_decay, s):
    w = _inputs(n)
    got, ranges = _run(n, gaps, weight_decay, s)
    wd_t = R.coefficient(weight_decay, s)
    want, decayed = w.copy(), np.zeros(n, bool)
    for a, b in ranges:
        want[a:b] = R.step(w[a:b], wd_t)
        decayed[a:b] = True
    inner = got[PAD:PAD + n]
    assert R.same(inner, want), (n, gaps, s, int((R.bits(inner) != R.bits(want)).sum()))
    if wd_t == 0:
        decayed[:] = False
    # the floats outside every chunk, the canaries and, at a coefficient of 0, everything: the very bits, NaNs included
    assert np.array_equal(R.bits(inner[~decayed]), R.bits(w[~decayed])), (n, gaps, s)
    assert np.array_equal(R.bits(got[:PAD]), R.bits(np.full(PAD, CANARY, F)))
    assert np.array_equal(R.bits(got[PAD + n:]), R.bits(np.full(PAD, CANARY, F)))
    if n >= 16 and wd_t != 0:
        changed = R.bits(inner) != R.bits(w)
        assert changed[decayed].any() and not changed[~decayed].any()
    return got


def test_the_table_above_the_grid_is_longer_than_the_grid():
    rows = _chunks(_ranges(ABOVE_GRID, True))
    assert GRID < len(rows) <= GRID + 4
    assert {c for _, c in rows} == {64, CHUNK, 4200 - CHUNK, 4}
    assert all(o % 4 == 0 and c % 4 == 0 and 0 < c <= CHUNK for o, c in rows)
    assert _chunks(_ranges(4100, False)) == [(0, 4096), (4096, 4)]
    assert _ranges(1020, True)[:3] == [(0, 64), (96, 1020)] and _ranges(0, True) == [] and _ranges(0, False) == []


@pytest.mark.parametrize("gaps", [False, True], ids=["whole", "gaps"])
@pytest.mark.parametrize("n", SIZES)
def test_constant(n, gaps):
    wd, counts = R.cases()["constant"]
    first = _check(n, gaps, wd, counts[0])
    again = _check(n, gaps, wd, counts[1])                  # a constant does not depend on the count ...
    assert np.array_equal(R.bits(first), R.bits(again))     # ... and the bits are the same from run to run


@pytest.mark.parametrize("gaps", [False, True], ids=["whole", "gaps"])
@pytest.mark.parametrize("n", SIZES)
def test_piecewise_across_a_boundary(n, gaps):
    wd, counts = R.cases()["piecewise"]
    assert R.coefficient(wd, counts[0]) != R.coefficient(wd, counts[1])
    for s in counts:
        _check(n, gaps, wd, s)


@pytest.mark.parametrize("gaps", [False, True], ids=["whole", "gaps"])
@pytest.mark.parametrize("n", SIZES)
def test_cosine_at_the_start_mid_way_and_past_the_end(n, gaps):
    wd, counts = R.cases()["cosine"]
    assert counts[0] == 0 and 2 * counts[1] == wd.decay_steps and counts[2] > wd.decay_steps
    assert [float(R.coefficient(wd, s)) for s in counts] == [float(F(0.1)), float(F(0.055)), float(F(0.01))]
    for s in counts:
        _check(n, gaps, wd, s)


@pytest.mark.parametrize("gaps", [False, True], ids=["whole", "gaps"])
@pytest.mark.parametrize("n", SIZES)
def test_a_coefficient_of_zero_keeps_every_bit(n, gaps):
    """Also the sign of a -0, which (-0) - (0 * -0) would turn into +0, and the payload of a NaN."""
    from lisec_amd import lr_schedules
    w = _inputs(n)
    if n >= 16:
        assert (np.signbit(w) & (w == 0)).any() and np.isnan(w).any()
        with np.errstate(all="ignore"):
            assert not np.array_equal(R.bits(np.subtract(w, np.multiply(F(0.0), w, dtype=F), dtype=F)), R.bits(w))
    _check(n, gaps, 0.0, 3)
    sched = lr_schedules.PiecewiseConstantDecay([5], [0.3, 0.0])        # 0 only past the boundary: the host cannot know
    _check(n, gaps, sched, 6)
    _check(n, gaps, sched, 5)


def test_eval_matches_the_reference_coefficients():
    import torch
    from lisec_amd import ops
    k = 64
    for name, (wd, counts) in R.cases().items():
        coeff = _coefficient_buffer(wd)
        for s0 in (0, 30, 1 << 33):                         # across the piecewise boundary (5) and the cosine's end (40)
            state = torch.tensor([s0, 0], dtype=torch.int64, device="cuda")
            out = torch.full((k,), -1.0, dtype=torch.float32, device="cuda")
            ops.weight_decay_eval(coeff, state, k, out)
            got = out.cpu().numpy()
            want = np.array([R.coefficient(wd, s0 + j) for j in range(k)], F)
            print(name, s0, "eval differs in", int((R.bits(got) != R.bits(want)).sum()), "of", k)
            assert np.array_equal(R.bits(got), R.bits(want)), (name, s0)
            assert state.cpu().tolist() == [s0, 0]
    # k = 0 is valid and writes nothing
    out = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    ops.weight_decay_eval(coeff, state, 0, out)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-1.0] * 4


def test_refusals_enqueue_nothing():
    import torch
    from lisec_amd import _lib, ops
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    assert lib.lisec_abi_version() == 14                    # entries are only added
    n = 1020
    buf = np.full(n + 2 * PAD, CANARY, F)
    buf[PAD:PAD + n] = _inputs(n)
    theta = torch.from_numpy(buf).cuda()
    before = theta.cpu().numpy().copy()
    rows = _chunks(_ranges(n - 4, True))
    table = ops.decay_table(rows, "cuda")
    coeff = _coefficient_buffer(0.3)
    state = torch.tensor([6, 0, 9], dtype=torch.int64, device="cuda")
    inner = theta.data_ptr() + 4 * PAD
    V = ctypes.c_void_p
    EINVAL = -1                                             # LISEC_EINVAL

    def decay(theta_=V(inner), chunks=P(table), n_chunks=len(rows), coeff_=P(coeff), state_=P(state)):
        return lib.lisec_weight_decay(theta_, chunks, n_chunks, coeff_, state_, st)

    assert decay(theta_=None) == EINVAL                     # NULL pointers
    assert decay(chunks=None) == EINVAL
    assert decay(coeff_=None) == EINVAL
    assert decay(state_=None) == EINVAL
    assert decay(n_chunks=-1) == EINVAL
    assert decay(theta_=V(inner + 4)) == EINVAL             # theta not 16-byte aligned
    assert decay(theta_=V(inner + 8)) == EINVAL
    assert decay(state_=V(state.data_ptr() + 4)) == EINVAL  # state not 8-byte aligned
    assert b"weight_decay" in lib.lisec_last_error()
    out = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    assert lib.lisec_weight_decay_eval(None, P(state), 4, P(out), st) == EINVAL
    assert lib.lisec_weight_decay_eval(P(coeff), None, 4, P(out), st) == EINVAL
    assert lib.lisec_weight_decay_eval(P(coeff), P(state), 4, None, st) == EINVAL
    assert lib.lisec_weight_decay_eval(P(coeff), P(state), -1, P(out), st) == EINVAL
    with pytest.raises(ValueError):
        ops.weight_decay(theta[PAD:PAD + n], table, len(rows) + 1, coeff, state)         # past the table
    with pytest.raises(ValueError):
        ops.weight_decay(theta[PAD:PAD + n], table, 1, coeff, state, first=-1)
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(theta.cpu().numpy()), R.bits(before))
    assert out.cpu().tolist() == [-1.0] * 4 and state.cpu().tolist() == [6, 0, 9]
    # n_chunks == 0 is valid and enqueues nothing; then the entry of lisec_amd.ops on a view, with `first`
    assert decay(n_chunks=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(theta.cpu().numpy()), R.bits(before))
    ops.weight_decay(theta[PAD:PAD + n], table, len(rows) - 1, coeff, state, first=1)
    torch.cuda.synchronize()
    want = before.copy()
    for a, b in _ranges(n - 4, True)[1:]:
        want[PAD + a:PAD + b] = R.step(before[PAD + a:PAD + b], R.coefficient(0.3, 6))
    got = theta.cpu().numpy()
    assert R.same(got, want) and np.array_equal(R.bits(got[:PAD + 96]), R.bits(before[:PAD + 96]))
