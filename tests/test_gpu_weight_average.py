"""lisec_weight_average / lisec_weight_swap / lisec_weight_average_eval on the GPU, bit for bit against the numpy
definition of tests/weight_average_ref.py: both kinds on and off their special steps, both placements of the pass
against the update (state_bias), the grid-stride loop's second trip, canaries around the buffers, every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import weight_average_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
PAD = 64                                   # canary floats on each side (a multiple of 4: the buffers stay 16-byte aligned)
FULL_TRIP = 2048 * 256 * 4                 # floats one trip of the kernel's grid covers (kAvgBlocks * kAvgThreads * 4)
SIZES = [0, 4, 1020, 4100, FULL_TRIP + 4]  # the last: a second, partial trip of the grid-stride loop
SEED = 20

_INPUTS = {}


def _inputs(n):
    """(a, w) for n floats, made once and left unchanged."""
    if n not in _INPUTS:
        a, w = R.make_inputs(n, SEED)
        a.setflags(write=False)
        w.setflags(write=False)
        _INPUTS[n] = (a, w)
    return _INPUTS[n]


def _desc(kind, decay=0.0, dynamic=False, start=0, period=1):
    from lisec_amd import _lib
    return _lib.WeightAverage(_lib.AVG_EMA if kind == "ema" else _lib.AVG_SWA, int(dynamic), start, period, decay)


def _padded(x, canary):
    import torch
    buf = np.full(len(x) + 2 * PAD, canary, F)
    buf[PAD:PAD + len(x)] = x
    return torch.from_numpy(buf).cuda()


def _inner(t):
    """The address of the floats between the canaries (an int: an empty torch view has no address, and n = 0 with real
    addresses is what the entry must accept)."""
    return t.data_ptr() + 4 * PAD


def _run_pass(n, desc, count, bias):
    """The pass on the shared inputs with canaries on both sides; returns (avg bits, theta bits) of the padded buffers."""
    import torch
    from lisec_amd import _lib
    a, w = _inputs(n)
    ta, tw = _padded(a, F(-7.25)), _padded(w, F(3.5))
    state = torch.tensor([count, 0], dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().lisec_weight_average(_inner(tw), _inner(ta), n, ctypes.byref(desc), _lib.ptr(state), bias,
                                                _lib.current_stream()))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [count, 0]                       # the count is read, never advanced
    return ta.cpu().numpy(), tw.cpu().numpy()


def _check(n, desc, s, want):
    a, w = _inputs(n)
    for bias in (0, -1):                                            # in front of / behind the update that advances the count
        ga, gw = _run_pass(n, desc, s - bias, bias)
        assert np.array_equal(R.bits(ga[PAD:PAD + n]), R.bits(want)), (n, bias)
        assert np.array_equal(R.bits(gw[PAD:PAD + n]), R.bits(w))                        # theta keeps its bits
        for buf, canary in ((ga, F(-7.25)), (gw, F(3.5))):
            assert np.array_equal(R.bits(buf[:PAD]), R.bits(np.full(PAD, canary, F)))
            assert np.array_equal(R.bits(buf[PAD + n:]), R.bits(np.full(PAD, canary, F)))


def test_the_inputs_are_not_vacuous():
    """The shared inputs hold +-0, denormals and pairs of very different magnitude, and tell the definition from the
    forms the kernel must not compute: an fma, the distributed a*(1 - c) + w*c, a reciprocal multiply (at a divisor
    that is no power of two).  (a + (w - a)*c is bit for bit the SAME function under round-to-nearest: see the ref.)"""
    for n in (1020, 4100):
        a, w = _inputs(n)
        tiny = np.finfo(F).tiny
        assert (np.signbit(w) & (w == 0)).any() and ((a == 0) & ~np.signbit(a)).any()
        assert ((np.abs(a) < tiny) & (a != 0)).any() and ((np.abs(w) < tiny) & (w != 0)).any()
        assert (np.abs(a) >= 1e8 * np.abs(w)).any() and (np.abs(w) >= 1e8 * np.abs(a)).any()
        c = R.ema_coefficient(50, 0.9)
        want = R.ema_step(a, w, 50, 0.9)
        assert not np.array_equal(R.bits(want), R.bits(R.ema_step_fma(a, w, c)))
        assert not np.array_equal(R.bits(want), R.bits(R.ema_step_reassociated(a, w, c)))
        assert not np.array_equal(R.bits(R.swa_step(a, w, 4, 0, 2)), R.bits(R.swa_step_reciprocal(a, w, 2)))
        assert not np.array_equal(R.bits(want), R.bits(a)) and not np.array_equal(R.bits(want), R.bits(w))


@pytest.mark.parametrize("n", SIZES)
def test_ema_constant(n):
    a, w = _inputs(n)
    _check(n, _desc("ema", decay=0.9), 50, R.ema_step(a, w, 50, 0.9))
    _check(n, _desc("ema", decay=0.0), 50, w)                       # c == 1: the store
    _check(n, _desc("ema", decay=1.0), 50, R.ema_step(a, w, 50, 1.0))      # c == 0: still a - (a - w)*0, in fp32


@pytest.mark.parametrize("n", SIZES)
def test_ema_dynamic(n):
    a, w = _inputs(n)
    for s in (3, 12, 5000):                                         # k = 0 (decay 0.1), k = 9, the cap
        want = R.ema_step(a, w, s, 0.99, start_step=3, dynamic_decay=True)
        _check(n, _desc("ema", decay=0.99, dynamic=True, start=3), s, want)


@pytest.mark.parametrize("n", SIZES)
def test_ema_before_start_step_stores(n):
    a, w = _inputs(n)
    for dynamic in (False, True):
        _check(n, _desc("ema", decay=0.99, dynamic=dynamic, start=10), 9, w)
    assert R.ema_step(np.array([1e8], F), np.array([1.0], F), 9, 0.99, start_step=10)[0] == F(1.0)


@pytest.mark.parametrize("n", SIZES)
def test_swa_snapshots(n):
    a, w = _inputs(n)
    start, period = 5, 2
    d = _desc("swa", start=start, period=period)
    for s, m in ((5, 0), (9, 2), (11, 3)):
        assert R.swa_m(s, start, period) == m
        _check(n, d, s, R.swa_step(a, w, s, start, period))
    _check(n, d, 5, w)                                              # m = 0: a <- w


@pytest.mark.parametrize("n", SIZES)
def test_swa_off_a_snapshot_keeps_the_bits(n):
    a, w = _inputs(n)
    d = _desc("swa", start=5, period=2)
    for s in (0, 4, 6, 10):
        assert R.swa_m(s, 5, 2) == -1
        _check(n, d, s, a)


def test_eval_matches_the_reference_coefficients():
    import torch
    from lisec_amd import ops
    k = 4096
    state = torch.tensor([0, 0], dtype=torch.int64, device="cuda")
    for decay, dynamic, start in ((0.99, False, 0), (0.99, True, 0), (0.9, True, 100), (0.5, False, 4000), (1.0, False, 0),
                                  (0.0, True, 0)):
        out = torch.full((k,), -1.0, dtype=torch.float32, device="cuda")
        ops.weight_average_eval(_desc("ema", decay=decay, dynamic=dynamic, start=start), state, k, c_out=out)
        want = np.array([R.ema_coefficient(s, decay, start, dynamic) for s in range(k)], F)
        assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(want)), (decay, dynamic, start)
    for start, period in ((0, 1), (0, 10), (7, 3), (4095, 2), (5000, 1)):
        out = torch.full((k,), -5, dtype=torch.int64, device="cuda")
        ops.weight_average_eval(_desc("swa", start=start, period=period), state, k, m_out=out)
        want = np.array([R.swa_m(s, start, period) for s in range(k)], np.int64)
        assert np.array_equal(out.cpu().numpy(), want), (start, period)
    state.fill_(0)
    state[0] = 1000                                                  # s = state[0] + j
    out = torch.empty(8, dtype=torch.float32, device="cuda")
    ops.weight_average_eval(_desc("ema", decay=0.99, dynamic=True), state, 8, c_out=out)
    want = np.array([R.ema_coefficient(1000 + j, 0.99, 0, True) for j in range(8)], F)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(want))


@pytest.mark.parametrize("n", SIZES)
def test_two_swaps_restore_both_buffers(n):
    import torch
    from lisec_amd import _lib, ops
    a, w = _inputs(n)
    ta, tw = _padded(a, F(-7.25)), _padded(w, F(3.5))
    a0, w0 = ta.cpu().numpy().copy(), tw.cpu().numpy().copy()
    _lib.check(_lib.load().lisec_weight_swap(_inner(ta), _inner(tw), n, _lib.current_stream()))
    torch.cuda.synchronize()
    ga, gw = ta.cpu().numpy(), tw.cpu().numpy()
    assert np.array_equal(R.bits(ga[PAD:PAD + n]), R.bits(w)) and np.array_equal(R.bits(gw[PAD:PAD + n]), R.bits(a))
    for got, was in ((ga, a0), (gw, w0)):                           # the canaries stay
        assert np.array_equal(R.bits(got[:PAD]), R.bits(was[:PAD])) and np.array_equal(R.bits(got[PAD + n:]), R.bits(was[PAD + n:]))
    if n:
        ops.weight_swap(ta[PAD:PAD + n], tw[PAD:PAD + n])             # the wrapper of lisec_amd.ops, on views
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(ta.cpu().numpy()), R.bits(a0)) and np.array_equal(R.bits(tw.cpu().numpy()), R.bits(w0))


def test_refusals_enqueue_nothing():
    import torch
    from lisec_amd import _lib
    lib, P, st = _lib.load(), _lib.ptr, _lib.current_stream()
    n = 1020
    a, w = _inputs(n)
    ta, tw = _padded(a, F(-7.25)), _padded(w, F(3.5))
    a0, w0 = ta.cpu().numpy().copy(), tw.cpu().numpy().copy()
    va, vw = ta[PAD:PAD + n], tw[PAD:PAD + n]
    state = torch.tensor([6, 0], dtype=torch.int64, device="cuda")
    good = _desc("ema", decay=0.9)
    ref = ctypes.byref
    EINVAL = -1                                                      # LISEC_EINVAL

    def avg(theta, avg_, n_, desc, state_=state):
        return lib.lisec_weight_average(theta, avg_, n_, desc, P(state_) if state_ is not None else None, 0, st)

    assert avg(None, P(va), n, ref(good)) == EINVAL                 # NULL pointers
    assert avg(P(vw), None, n, ref(good)) == EINVAL
    assert avg(P(vw), P(va), n, None) == EINVAL
    assert avg(P(vw), P(va), n, ref(good), None) == EINVAL
    assert avg(P(va), P(va), n, ref(good)) == EINVAL                # theta == avg
    assert avg(P(vw), P(va), -4, ref(good)) == EINVAL               # n < 0
    assert avg(P(vw), P(va), n - 2, ref(good)) == EINVAL            # n % 4
    assert avg(P(tw[PAD + 1:]), P(va), n - 4, ref(good)) == EINVAL  # not 16-byte aligned
    assert avg(P(vw), P(ta[PAD + 2:]), n - 4, ref(good)) == EINVAL
    bad = [_lib.WeightAverage(2, 0, 0, 1, 0.5), _lib.WeightAverage(-1, 0, 0, 1, 0.5),       # unknown kind
           _desc("ema", decay=-0.01), _desc("ema", decay=1.01), _desc("ema", decay=float("nan")),
           _desc("ema", decay=0.5, start=-1), _desc("swa", start=-1, period=2),
           _desc("swa", start=0, period=0), _desc("swa", start=0, period=-3)]
    for d in bad:
        assert avg(P(vw), P(va), n, ref(d)) == EINVAL, (d.kind, d.start, d.period, d.decay)
    assert b"weight_average" in lib.lisec_last_error()
    assert lib.lisec_weight_swap(None, P(vw), n, st) == EINVAL
    assert lib.lisec_weight_swap(P(va), None, n, st) == EINVAL
    assert lib.lisec_weight_swap(P(va), P(va), n, st) == EINVAL      # a == b
    assert lib.lisec_weight_swap(P(va), P(vw), -4, st) == EINVAL
    assert lib.lisec_weight_swap(P(va), P(vw), n - 1, st) == EINVAL
    assert lib.lisec_weight_swap(P(ta[PAD + 1:]), P(vw), n - 4, st) == EINVAL
    out = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    assert lib.lisec_weight_average_eval(ref(bad[0]), P(state), 4, P(out), None, st) == EINVAL
    assert lib.lisec_weight_average_eval(ref(good), P(state), 4, None, None, st) == EINVAL
    assert lib.lisec_weight_average_eval(None, P(state), 4, P(out), None, st) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(ta.cpu().numpy()), R.bits(a0)) and np.array_equal(R.bits(tw.cpu().numpy()), R.bits(w0))
    assert np.array_equal(out.cpu().numpy(), np.full(4, -1.0, F)) and state.cpu().tolist() == [6, 0]
    # a period the EMA kind does not use, and a decay the SWA kind does not use, are ignored
    assert avg(P(vw), P(va), n, ref(_lib.WeightAverage(0, 0, 0, 0, 0.9))) == 0
    assert avg(P(vw), P(va), n, ref(_lib.WeightAverage(1, 0, 0, 1, 7.0))) == 0
    torch.cuda.synchronize()
