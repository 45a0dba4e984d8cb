"""lisec_bn_recalibrate_take / lisec_bn_recalibrate_finish on the GPU over synthetic buffers, bit for bit against the
numpy definition of tests/bn_recalibrate_ref.py: three records (C = 1, 5, 64) with both coefficient values and offsets
padded to 4 floats, pads that hold a sentinel, K = 3 takes over states that include 0, a negative mean, a denormal
statistic and one whose quotient by the coefficient is still tiny; both rules; every refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_recalibrate_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.5)
#        mean_off var_off  C   coef          (floats; every range padded to a multiple of 4)
TABLE = [(0, 4, 1, R.COEF_VFE), (8, 16, 5, R.COEF_CONV), (24, 88, 64, R.COEF_VFE)]
N_STATE = 156                                      # 152 used, one more group of pads at the end
K = 3


def _states():
    """K states as a training forward leaves them in a zeroed buffer: fl32(batch * coef).  Batch values chosen for the
    edges: 0, a negative mean, 1e-38 as the STATISTIC ITSELF (a float32 denormal), a batch value of 2e-37 whose product
    with coef is denormal, and ordinary values of both signs and many magnitudes."""
    rng = np.random.default_rng(11)
    out = []
    for k in range(K):
        s = np.full(N_STATE, SENTINEL, dtype=np.float32)
        for mean_off, var_off, C, coef in TABLE:
            mean = rng.normal(0, 1, C) * 10.0 ** rng.integers(-6, 6, C)
            var = rng.uniform(0, 2, C) * 10.0 ** rng.integers(-6, 6, C)
            s[mean_off:mean_off + C] = (mean * coef).astype(np.float32)
            s[var_off:var_off + C] = (var * coef).astype(np.float32)
        s[0] = np.float32([0.0, -3.25 * R.COEF_VFE, 1e-38][k])          # C = 1: zero, a negative mean, a denormal
        s[4] = np.float32([1e-38, 0.0, 2e-37 * R.COEF_VFE][k])
        s[8:11] = np.float32([0.0, -1.5 * R.COEF_CONV, 2e-37 * R.COEF_CONV])
        s[24 + 63] = np.float32(1e-38)                                   # the last channel of the widest record
        s[88 + 63] = np.float32(2e-37 * R.COEF_VFE)
        out.append(s)
    assert 0 < abs(out[2][4]) < np.finfo(np.float32).tiny                # denormal indeed
    return out


def _pads():
    used = np.zeros(N_STATE, dtype=bool)
    for mean_off, var_off, C, _ in TABLE:
        used[mean_off:mean_off + C] = True
        used[var_off:var_off + C] = True
    return ~used


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


@pytest.mark.parametrize("statistics", ["mean", "pooled"])
def test_takes_and_finish_are_the_definition_bit_for_bit(statistics):
    import torch
    from lisec_amd import ops
    table = ops.BnRecalTable(TABLE)
    assert table.channels == 70 and table.n_entries == 3
    pads = _pads()
    dev = torch.device("cuda")
    acc = torch.full((3 * 70 + 2,), 99.0, dtype=torch.float64, device=dev)      # two doubles behind the planes
    acc[:210].zero_()
    state = torch.empty(N_STATE, dtype=torch.float32, device=dev)
    want_acc = R.new_acc(TABLE)
    for s in _states():
        state.copy_(torch.from_numpy(s))
        ops.bn_recalibrate_take(state, table, acc)
        work = s.copy()
        R.take(work, TABLE, want_acc)
        got = _host(state)
        assert np.array_equal(R.bits(got), R.bits(work))                        # +0 in every record, pads untouched
        assert not R.bits(got[~pads]).any() and (got[pads] == SENTINEL).all()
        assert np.array_equal(R.bits(_host(acc)[:210]), R.bits(want_acc))
    assert np.abs(want_acc).max() > 0 and np.isfinite(want_acc).all()
    ops.bn_recalibrate_finish(state, table, acc, K, statistics)
    want = np.full(N_STATE, SENTINEL, dtype=np.float32)
    R.finish(want, TABLE, want_acc, K, statistics)
    got = _host(state)
    assert np.array_equal(R.bits(got), R.bits(want))
    assert (got[pads] == SENTINEL).all()
    a = _host(acc)
    assert np.array_equal(R.bits(a[:210]), R.bits(want_acc)) and (a[210:] == 99.0).all()     # finish only reads acc


def test_the_rules_differ_and_the_library_holds_the_constants():
    from lisec_amd import _lib
    lib = _lib.load()
    assert lib.lisec_bn_recalibrate_coef(_lib.BN_FINALIZER_CONV) == R.COEF_CONV
    assert lib.lisec_bn_recalibrate_coef(_lib.BN_FINALIZER_VFE) == R.COEF_VFE
    assert lib.lisec_bn_recalibrate_coef(2) == 0.0 and R.COEF_CONV != R.COEF_VFE
    states = _states()
    a, _ = R.recalibrate(states, TABLE, "mean")
    b, _ = R.recalibrate(states, TABLE, "pooled")
    assert np.array_equal(R.bits(a[24:88]), R.bits(b[24:88])) and not np.array_equal(R.bits(a[88:152]), R.bits(b[88:152]))


def test_invalid_arguments_are_refused_without_a_launch():
    import torch
    from lisec_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    dev = torch.device("cuda")
    state = torch.from_numpy(_states()[0]).to(dev)
    acc = torch.full((210,), 3.0, dtype=torch.float64, device=dev)
    before_s, before_a = R.bits(_host(state)), R.bits(_host(acc))
    st = _lib.current_stream()
    P = _lib.ptr

    def table(rows):
        arr = (_lib.BnRecalEntry * len(rows))()
        for rec, (m, v, C, coef) in zip(arr, rows):
            rec.mean_off, rec.var_off, rec.C, rec.coef = m, v, C, coef
        return arr

    good = table(TABLE)

    def take(s=state, t=good, n=3, a=acc):
        return lib.lisec_bn_recalibrate_take(P(s), t, n, P(a), st)

    def finish(s=state, t=good, n=3, a=acc, sweeps=K, rule=0):
        return lib.lisec_bn_recalibrate_finish(P(s), t, n, P(a), sweeps, rule, st)

    bad_tables = [table([(0, 4, 0, 0.01)]), table([(0, 4, -1, 0.01)]), table([(0, 4, 1, 0.0)]), table([(0, 4, 1, 1.0)]),
                  table([(0, 4, 1, -0.01)]), table([(0, 4, 1, float("nan"))]), table([(0, 4, 1, 1.5)]),
                  table([(2, 4, 1, 0.01)]), table([(0, 5, 1, 0.01)]), table([(-4, 4, 1, 0.01)]), table([(0, -4, 1, 0.01)])]
    for entry in (take, finish):
        assert entry(s=None) == EINVAL and entry(t=None) == EINVAL and entry(a=None) == EINVAL
        assert entry(n=0) == EINVAL and entry(n=-1) == EINVAL
        assert entry(t=(_lib.BnRecalEntry * 65)(), n=65) == EINVAL
        for t in bad_tables:
            assert entry(t=t, n=1) == EINVAL
        # a bad record behind good ones is found too
        assert entry(t=table(TABLE[:2] + [(24, 88, 64, 1.0)]), n=3) == EINVAL
        assert b"bn_recalibrate" in lib.lisec_last_error()
    assert finish(sweeps=0) == EINVAL and finish(sweeps=-3) == EINVAL
    assert finish(rule=2) == EINVAL and finish(rule=-1) == EINVAL
    assert np.array_equal(R.bits(_host(state)), before_s) and np.array_equal(R.bits(_host(acc)), before_a)
    # and the good calls do launch
    assert take() == 0 and finish(rule=1) == 0
    assert not np.array_equal(R.bits(_host(state)), before_s)


def test_the_wrappers_refuse_buffers_the_table_does_not_fit():
    import torch
    from lisec_amd import ops
    table = ops.BnRecalTable(TABLE)
    dev = torch.device("cuda")
    state = torch.zeros(N_STATE, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="acc"):
        ops.bn_recalibrate_take(state, table, torch.zeros(209, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="outside"):
        ops.bn_recalibrate_take(state[:151], table, ops.bn_recal_acc(table, dev))
    with pytest.raises(ValueError, match="statistics"):
        ops.bn_recalibrate_finish(state, table, ops.bn_recal_acc(table, dev), 1, "median")
