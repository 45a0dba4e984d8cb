"""BatchNormalization recalibration without a GPU: the numpy definition (tests/bn_recalibrate_ref.py) against
torch.nn.BatchNorm1d(momentum=None) for the 'mean' rule and against the variance of the concatenated rows for the
'pooled' rule, and the refusals that need no device."""
import numpy as np
import pytest
import torch

import bn_recalibrate_ref as R

K, ROWS, C = 4, 7, 5
U = 2.0 ** -24                                       # half a float32 ulp, relative: one rounding to nearest


def _batches():
    """K batches of ROWS x C float32 values in [1, 2): every batch mean has the same sign, so a relative bound on the
    mean of the means is a bound on each term's rounding (no cancellation between sweeps)."""
    rng = np.random.default_rng(5)
    return [rng.uniform(1.0, 2.0, (ROWS, C)).astype(np.float32) for _ in range(K)]


@pytest.mark.parametrize("coef", [R.COEF_CONV, R.COEF_VFE])
def test_mean_rule_is_torch_batchnorm_with_momentum_none(coef):
    """What a finaliser leaves in a zeroed buffer is fl32(batch * c); the definition over K of them is torch's
    cumulative average of the batch statistics (running_var: the unbiased batch variance, as the conv sinks give it).
    torch runs in float64 on the float32 rows, so its running statistics carry no rounding of their own to speak of
    and the bound is the definition's alone: one rounding of batch * c, one of the result, both 2^-24 relative on
    same-signed terms, the fp64 operations 2^-53 each -- under the 3 * 2^-24 of the issue."""
    bn = torch.nn.BatchNorm1d(C, momentum=None).double()
    bn.train()
    table = [(0, 8, C, coef)]
    states = []
    for x in _batches():
        xd = torch.from_numpy(x).double()
        bn(xd)
        s = np.full(16, np.nan, dtype=np.float32)
        s[0:C] = (xd.mean(0).numpy() * coef).astype(np.float32)
        s[8:8 + C] = (xd.var(0, unbiased=True).numpy() * coef).astype(np.float32)
        states.append(s)
    assert int(bn.num_batches_tracked) == K
    out, _ = R.recalibrate(states, table, "mean")
    want_mean, want_var = bn.running_mean.numpy(), bn.running_var.numpy()
    err_mean = np.abs(out[0:C].astype(np.float64) - want_mean) / np.abs(want_mean)
    err_var = np.abs(out[8:8 + C].astype(np.float64) - want_var) / np.abs(want_var)
    print("relative errors against torch: mean", err_mean.max(), "variance", err_var.max(), "bound", 3 * U)
    assert err_mean.max() <= 3 * U and err_var.max() <= 3 * U
    assert np.isnan(out[C:8]).all() and np.isnan(out[8 + C:]).all()          # the pads are never written


def test_pooled_rule_is_the_variance_of_the_concatenated_rows():
    """Equal-sized batches with BIASED batch variances: mean(var_i) + mean(m_i^2) - mean(m_i)^2 is the biased variance
    of all K * ROWS rows.  In fp64 throughout (a float64 state: the rule without the float32 roundings)."""
    coef = R.COEF_CONV
    table = [(0, 8, C, coef)]
    xs = [x.astype(np.float64) for x in _batches()]
    states = []
    for x in xs:
        s = np.zeros(16, dtype=np.float64)
        s[0:C] = x.mean(0) * coef
        s[8:8 + C] = x.var(0) * coef
        states.append(s)
    out, _ = R.recalibrate(states, table, "pooled")
    rows = np.concatenate(xs)
    assert np.allclose(out[0:C], rows.mean(0), rtol=1e-12, atol=0)
    assert np.allclose(out[8:8 + C], rows.var(0), rtol=1e-12, atol=0)
    # and it is not the 'mean' rule: the batch means differ
    plain, _ = R.recalibrate(states, table, "mean")
    assert not np.allclose(plain[8:8 + C], rows.var(0), rtol=1e-6, atol=0)


def test_take_zeroes_the_statistics_and_leaves_the_pads():
    table = [(0, 4, 1, R.COEF_VFE), (8, 12, 3, R.COEF_CONV)]
    s = np.arange(1, 17, dtype=np.float32)
    acc = R.new_acc(table)
    R.take(s, table, acc)
    assert s.tolist() == [0, 2, 3, 4, 0, 6, 7, 8, 0, 0, 0, 12, 0, 0, 0, 16]
    assert acc[0] == np.float64(np.float32(1)) / R.COEF_VFE and acc[4 + 1] == 13.0 / R.COEF_CONV
    assert acc[8 + 3] == (11.0 / R.COEF_CONV) * (11.0 / R.COEF_CONV)


def test_the_two_coefficients_differ_as_documented():
    assert abs(R.COEF_CONV / R.COEF_VFE - 1) == pytest.approx(9.5e-7, rel=0.02)


def test_refusals_that_need_no_device():
    from lisec_amd import callbacks, ops
    boxes = [np.array([[0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0]])]
    sweeps = [np.zeros((4, 3), dtype=np.float32)]
    with pytest.raises(ValueError, match="statistics"):
        R.finish(np.zeros(8, np.float32), [(0, 4, 1, 0.5)], np.zeros(3), 1, "median")
    with pytest.raises(ValueError, match="statistics"):
        ops.bn_statistics("median")
    with pytest.raises(ValueError, match="statistics"):
        callbacks.PreciseBatchNorm(sweeps, statistics="median")
    with pytest.raises(ValueError, match="statistics"):
        callbacks.AverageModelCheckpoint(False, "never.h5", update_bn=sweeps, statistics="median")
    with pytest.raises(ValueError, match="average_weights"):
        callbacks.DetectionEvaluation(sweeps, boxes, update_bn=sweeps)
    with pytest.raises(ValueError, match="period"):
        callbacks.PreciseBatchNorm(sweeps, period=0)
    # the valid forms are constructible without a device
    cb = callbacks.PreciseBatchNorm(sweeps, period=2, steps=1)
    assert (cb.period, cb.steps, cb.statistics) == (2, 1, "pooled")
    ev = callbacks.DetectionEvaluation(sweeps, boxes, average_weights=True, update_bn=sweeps)
    assert ev.update_bn is sweeps and ev.statistics == "mean"


def test_the_table_of_the_network_names_every_layer_once():
    """ops.bn_recal_rows on the ParamStore layout (host arithmetic): 3 + 3 + 16 layers, the three VFE layers in the
    VFE family, offsets 4-float aligned and disjoint."""
    from types import SimpleNamespace
    from lisec_amd import _lib, ops
    from lisec_amd.params import TRAINABLE_KINDS, param_specs
    specs, offsets, ns = param_specs(1), {}, 0
    for name, shape, kind in specs:
        if kind not in TRAINABLE_KINDS:
            offsets[name] = ("state", ns, shape)
            ns += (int(np.prod(shape)) + 3) // 4 * 4
    rows = ops.bn_recal_rows(SimpleNamespace(specs=specs, offsets=offsets))
    assert len(rows) == 22 and [r[3] for r in rows].count(_lib.BN_FINALIZER_VFE) == 3
    assert [r[3] for r in rows[:3]] == [_lib.BN_FINALIZER_VFE] * 3 and [r[2] for r in rows[:3]] == [16, 32, 64]
    seen = np.zeros(ns, dtype=int)
    for mean_off, var_off, C, _ in rows:
        assert mean_off % 4 == 0 and var_off % 4 == 0
        seen[mean_off:mean_off + C] += 1
        seen[var_off:var_off + C] += 1
    assert seen.max() == 1 and seen.sum() == 2 * sum(r[2] for r in rows)
